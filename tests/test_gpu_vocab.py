"""GPU: vocabulary restriction in place (SetVocabulary / ResetVocabulary on a
loaded processor and spm_hip_model_set_piece_types on a handle) and the
device piece count (spm_hip_count_ids).

Reference of a restricted encode: the CPU oracle on the proto with the same
types written into it (vocab_ref.retype).  The oracle takes min_score /
max_score from the NORMAL pieces it sees, the restricted processor keeps the
load-time ones, so the vocabularies here always keep a NORMAL piece with the
model's minimum and one with its maximum score; the case where the two differ
is test_frozen_min_score.  The processor is driven through lib/vocab_selftest
(one process per test, several steps each)."""
import os
import subprocess

import numpy as np
import pytest

import bpe_cases as C
import nbest_ref as NB
import oracle_lib as O
import sample_ref
import spm_amd as S
import vocab_ref as V
from model_builder import NORMAL, UNIGRAM, UNUSED, base_pieces, model
from model_reader import read_pieces
from test_vocab_cpu import FROZEN_PIECES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SELFTEST = os.path.join(ROOT, "sentencepiece-comments_amd", "lib", "vocab_selftest")
pytestmark = pytest.mark.gpu


def _run(model_path, commands):
    p = subprocess.run([SELFTEST, str(model_path)], input=b"".join(c + b"\n" for c in commands),
                       capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    return p.stdout.split(b"\n")[:-1]


def _cmd(*fields):
    return b"\t".join(f if isinstance(f, bytes) else str(f).encode() for f in fields)


def _ids(line):
    assert line.startswith(b"ids"), line
    return [int(x) for x in line.split()[1:]]


def _golden_ids(name, count):
    rows = open(os.path.join(GOLD, name)).read().split("\n")[:count]
    return [list(map(int, r.split())) for r in rows]


def _counted_vocabulary(pieces, rows, at_least):
    """Pieces seen at least `at_least` times in the id rows, plus the NORMAL
    pieces with the minimum and with the maximum score.  One-char pieces
    and pieces with a tab or line break are left out of the list (the former
    stay NORMAL anyway, the latter cannot be written into a command)."""
    counts = np.bincount(np.concatenate([np.asarray(r, dtype=np.int64) for r in rows]), minlength=len(pieces))
    normal = [i for i, (_, _, t) in enumerate(pieces) if t == NORMAL]
    keep = {i for i in normal if counts[i] >= at_least}
    scores = [pieces[i][1] for i in normal]
    keep |= {i for i in normal if pieces[i][1] in (min(scores), max(scores))}
    return [pieces[i][0] for i in sorted(keep)
            if not V.one_char(pieces[i][0]) and not set(pieces[i][0]) & set(b"\t\n\r")]


class _Restricted:
    """A golden model, its counted vocabulary and the oracle's ids of the
    first `lines` corpus lines under the restriction."""

    def __init__(self, model_name, text, golden, lines, count_lines):
        self.model_path = os.path.join(GOLD, model_name)
        self.text_path = os.path.join(GOLD, text)
        self.mb = open(self.model_path, "rb").read()
        self.pieces = read_pieces(self.mb)
        self.lines = O.read_lines_binary(self.text_path)[:lines]
        self.golden = _golden_ids(golden, lines)
        self.vocab = _counted_vocabulary(self.pieces, self.golden[:count_lines], 5)
        self.types = V.set_vocabulary(self.pieces, self.vocab)
        assert UNUSED in self.types
        self.retyped = V.retype(self.mb, self.types)
        self.want = O.OracleModel(self.retyped).encode_lines(self.lines)
        assert self.want != self.golden   # the restriction changes the segmentation


_CASES = {
    "unigram_byte": ("test_model.model", "botchan.txt", "botchan_test_model.ids", 2000, 1000),
    "unigram_wide": ("test_ja_model.model", "wagahaiwa_nekodearu.txt", "wagahaiwa_test_ja_model.ids", 500, 250),
    "bpe": ("botchan_bpe1k.model", "botchan.txt", "botchan_bpe1k.ids", 2000, 1000),
}
_cache = {}


def _case(name):
    if name not in _cache:
        _cache[name] = _Restricted(*_CASES[name])
    return _cache[name]


def test_reference_answer(tmp_path):
    """sentencepiece_processor_test.cc:1016-1031: without "ab", "abc" is "▁ a b c"."""
    pieces = base_pieces() + [("a", 0.0, NORMAL), ("b", 0.3, NORMAL), ("c", 0.2, NORMAL), ("ab", 1.0, NORMAL),
                              ("▁", 3.0, NORMAL)]
    path = tmp_path / "m.model"
    path.write_bytes(model(pieces))
    out = _run(path, [_cmd("encode", "abc"), _cmd("set", "a", "b", "c"), _cmd("pieces", "abc"), _cmd("encode", "abc"),
                      _cmd("unused"), _cmd("reset"), _cmd("encode", "abc")])
    assert out == [b"ids 7 6 5", b"ok", "pieces ▁ a b c".encode(), b"ids 7 3 4 5", b"unused 0 0 0 0 0 0 1 0", b"ok",
                   b"ids 7 6 5"]


def test_frozen_min_score(tmp_path):
    """SetVocabulary({"xa"}) makes "zz" (-20, the minimum score) UNUSED.  In
    place the unknown score stays -20 - 10, so "xa" (-2) beats <unk> a (-30 +
    12); a reload of the retyped proto takes -3 - 10 and answers <unk> a."""
    mb = model(FROZEN_PIECES, UNIGRAM, add_dummy_prefix=False)
    types = V.set_vocabulary(FROZEN_PIECES, ["xa"])
    assert V.viterbi(FROZEN_PIECES, types, b"xa", -30.0) == [5]
    path = tmp_path / "m.model"
    path.write_bytes(mb)
    out = _run(path, [_cmd("set", "xa"), _cmd("encode", "xa"), _cmd("batch", _write(tmp_path, [b"xa"] * 40), 0, 40),
                      _cmd("nbest", _write(tmp_path, [b"xa"]), 0, 1, 2)])
    assert out[:2] == [b"ok", b"ids 5"]
    assert out[2:42] == [b"ids 5"] * 40
    assert out[42:] == [b"paths 2", b"ids 5", b"ids 0 3"]
    # The oracle on the retyped proto says otherwise: the case tests something.
    assert O.OracleModel(V.retype(mb, types)).encode_lines([b"xa"]) == [[0, 3]]
    assert V.viterbi(FROZEN_PIECES, types, b"xa", -13.0) == [0, 3]


def _write(tmp_path, lines, name="lines.txt"):
    p = tmp_path / ("%d_%s" % (len(lines), name))
    p.write_bytes(b"".join(l + b"\n" for l in lines))
    return str(p)


@pytest.mark.parametrize("name", list(_CASES))
def test_restricted_encode(name):
    """EncodeBatch under the restriction equals the oracle on the retyped
    proto, and the golden ids again after ResetVocabulary; 50 lines one at a
    time (the small path and its resident server) with the restriction
    changing between two such calls."""
    c = _case(name)
    n = len(c.lines)
    out = _run(c.model_path, [
        _cmd("set", *c.vocab), _cmd("unused"), _cmd("batch", c.text_path, 0, n), _cmd("single", c.text_path, 0, 25),
        _cmd("reset"), _cmd("single", c.text_path, 25, 15), _cmd("batch", c.text_path, 0, n),
        _cmd("set", *c.vocab), _cmd("single", c.text_path, 40, 10)])
    assert out[0] == b"ok"
    assert [int(x) for x in out[1].split()[1:]] == [int(t == UNUSED) for t in c.types]
    at = 2
    assert [_ids(l) for l in out[at:at + n]] == c.want
    at += n
    assert [_ids(l) for l in out[at:at + 25]] == c.want[:25]
    at += 25
    assert out[at] == b"ok"
    assert [_ids(l) for l in out[at + 1:at + 16]] == c.golden[25:40]
    at += 16
    assert [_ids(l) for l in out[at:at + n]] == c.golden
    at += n
    assert out[at] == b"ok"
    assert [_ids(l) for l in out[at + 1:]] == c.want[40:50]


def test_restricted_handle_kernels():
    """The C-ABI level on test_ja_model (wide-char kernel, cooperative kernel
    for the long lines, general kernel when forced): ids and piece lengths of
    normalized sentences against the oracle on the retyped proto."""
    c = _case("unigram_wide")
    dm = S.DeviceModel(c.mb)
    dm.set_vocabulary(c.vocab)
    assert dm.piece_types().tolist() == c.types
    norm = dm.normalize(c.lines)
    assert max(len(s) for s in norm) >= 128   # the cooperative kernel's share
    buf, off = S.to_csr(norm)
    want = O.OracleModel(c.retyped).encode_normalized_csr(buf, off, threads=8, with_lens=True)
    for force in (False, True):
        dm.set_force_general(force)
        got = dm.encode_csr_host(buf, off, with_lens=True)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
    dm.set_force_general(False)
    dm.reset_vocabulary()
    got = dm.encode_csr_host(buf, off, with_lens=True)
    for g, w in zip(got, O.OracleModel(c.mb).encode_normalized_csr(buf, off, threads=8, with_lens=True)):
        assert np.array_equal(g, w)


BPE_TIERS = {
    "affine": (dict(), C.TIER_LANE_AFFINE),
    "table": (dict(order="shuffled"), C.TIER_LANE_TABLE),
    "words": (dict(ties=True), C.TIER_LANE_WORDS),
    "half32768": (dict(pad_to=32768), C.TIER_HALF),
    "half65600": (dict(pad_to=65600), C.TIER_HALF),
    "general": (dict(user_defined=True), C.TIER_GENERAL),
}


@pytest.mark.parametrize("name", list(BPE_TIERS))
def test_bpe_tiers_restricted(name):
    """Half of the merged pieces UNUSED on every BPE tier: the pair entries'
    unused bit and the per-piece kinds are re-tagged in place, and the
    resegmentation of UNUSED pushes must be the oracle's."""
    kw, tier = BPE_TIERS[name]
    spec = C.build_model(**kw)
    dm = S.DeviceModel(spec.blob)
    assert dm.info().fast_variant == tier
    vocab = C.MERGES[::2]
    dm.set_vocabulary(vocab)
    types = V.set_vocabulary(spec.pieces, vocab)
    assert dm.piece_types().tolist() == types and types.count(UNUSED) == len(C.MERGES) - len(vocab)
    assert dm.info().fast_variant == tier
    sents = C.batch("shuffled") + C.batch("refused_tile", 257)
    buf, off = S.to_csr(sents)
    for blob in (V.retype(spec.blob, types), spec.blob):
        want = O.OracleModel(blob).encode_normalized_csr(buf, off, threads=8, with_lens=True)
        got = dm.encode_csr_host(buf, off, with_lens=True)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
        dm.reset_vocabulary()


def test_sample_and_nbest_restricted(tmp_path):
    """Under a restriction SampleEncode and NBestEncode (N = 4) emit no UNUSED
    id on 200 lines, and the n-best rows are nbest_ref's on a model object
    with the same types and the load-time scores."""
    c = _case("unigram_byte")
    n = 200
    out = _run(c.model_path, [_cmd("set", *c.vocab), _cmd("sample", c.text_path, 0, n, 0.5),
                              _cmd("nbest", c.text_path, 0, n, 4)])
    assert out[0] == b"ok"
    unused = {i for i, t in enumerate(c.types) if t == UNUSED}
    sampled = [_ids(l) for l in out[1:1 + n]]
    assert len(sampled) == n and not unused & {i for row in sampled for i in row}
    ref = sample_ref.Model(c.retyped)
    load = sample_ref.Model(c.mb)
    ref.max_score, ref.unk_score = load.max_score, load.unk_score
    norm = S.DeviceModel(c.mb, host_only=True).normalize(c.lines[:n])
    at = 1 + n
    for s in norm:
        paths, _ = NB.nbest(ref, s, 4)
        want = [NB.merge_unknown(ids, ref.unk_id) for ids, _, _ in paths]
        assert out[at] == b"paths %d" % len(want)
        got = [_ids(l) for l in out[at + 1:at + 1 + len(want)]]
        assert got == want
        assert not unused & {i for row in got for i in row}
        at += 1 + len(want)
    assert at == len(out)


def test_nbest_host_tier_restricted():
    """The host search (csrc/host_nbest.h) reads the host copy of the trie
    values: with the device arenas cut down so that sentences reach it, its
    paths under a restriction are those of the device tiers, score bits included."""
    c = _case("unigram_byte")
    dm = S.DeviceModel(c.mb)
    dm.set_vocabulary(c.vocab)
    buf, off = S.to_csr(dm.normalize(c.lines[:60]))
    want = dm.nbest_encode_csr_host(buf, off, 8, with_lens=True)
    assert dm.nbest_stats()[1] == 0
    dm.set_nbest_max_hyps(64, 200)
    got = dm.nbest_encode_csr_host(buf, off, 8, with_lens=True)
    assert dm.nbest_stats()[1] > 0
    for g, w in zip(got, want):
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8))
    unused = {i for i, t in enumerate(c.types) if t == UNUSED}
    assert not unused & set(got[0].tolist())


# ---- spm_hip_count_ids ----

TILE = 4096   # kCountTile (csrc/kernels.h)


@pytest.fixture(scope="module")
def counters():
    return {"lds": S.DeviceModel(open(os.path.join(GOLD, "test_model.model"), "rb").read()),  # 1000 pieces
            "lds32768": S.DeviceModel(C.build_model(pad_to=32768).blob),   # the most pieces the LDS bins take
            "wave32769": S.DeviceModel(C.build_model(pad_to=32769).blob),  # one more: no bins
            "wave": S.DeviceModel(C.build_model(pad_to=65600).blob)}


def _streams(v):
    rng = np.random.default_rng(5)
    zipf = np.minimum(rng.zipf(1.3, 50000) - 1, v - 1).astype(np.int32)
    return {
        "empty": np.zeros(0, np.int32),
        "one": np.array([v - 1], np.int32),
        "tile": rng.integers(0, v, TILE, dtype=np.int32),
        "tile_plus_one": rng.integers(0, v, TILE + 1, dtype=np.int32),
        "one_id": np.full(100000, 7, np.int32),
        "every_id": np.arange(v, dtype=np.int32)[::-1].copy(),
        "zipf": zipf,
        "blocks": rng.integers(0, v, 3 * TILE * 300 + 17, dtype=np.int32),   # more tiles than workgroups
    }


@pytest.mark.parametrize("path", ["lds", "lds32768", "wave32769", "wave"])
def test_count_ids(counters, path):
    dm = counters[path]
    v = dm.info().piece_size
    assert (v <= 32768) == path.startswith("lds")   # kCountLdsMaxPieces (csrc/kernels.h)
    for name, ids in _streams(v).items():
        got, status = dm.count_ids_host(ids)
        assert status == 0, name
        assert np.array_equal(got, np.bincount(ids, minlength=v).astype(np.uint64)), name
    # Ids outside [0, v) are skipped and flagged.
    ids = np.array([3, -1, v, 3, v - 1, 2 ** 31 - 1, -2 ** 31, 0], np.int32)
    got, status = dm.count_ids_host(ids)
    assert status == 1
    want = np.zeros(v, np.uint64)
    want[[3, v - 1, 0]] = [2, 1, 1]
    assert np.array_equal(got, want)
    # Accumulation over two calls, from counters past 32 bits.
    start = np.full(v, 1 << 40, np.uint64)
    a, b = _streams(v)["zipf"], _streams(v)["tile_plus_one"]
    got, _ = dm.count_ids_host(a, start)
    got, _ = dm.count_ids_host(b, got)
    assert np.array_equal(got, start + np.bincount(np.concatenate([a, b]), minlength=v).astype(np.uint64))


def test_count_ids_device_entry(counters):
    """The stream entry on device buffers: accumulates into d_counts, ORs the status word."""
    import torch
    dm = counters["lds"]
    v = dm.info().piece_size
    ids = _streams(v)["zipf"]
    bad = np.concatenate([ids[:100], [-5]]).astype(np.int32)
    d_ids, d_bad = torch.from_numpy(ids).cuda(), torch.from_numpy(bad).cuda()
    d_counts = torch.zeros(v, dtype=torch.int64, device="cuda")
    d_status = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dm.count_ids_device(d_ids.data_ptr(), len(ids), d_counts.data_ptr(), d_status.data_ptr())
    dm.count_ids_device(d_ids.data_ptr(), len(ids), d_counts.data_ptr(), None)
    torch.cuda.synchronize()
    assert int(d_status.item()) == 0
    dm.count_ids_device(d_bad.data_ptr(), len(bad), d_counts.data_ptr(), d_status.data_ptr())
    torch.cuda.synchronize()
    assert int(d_status.item()) == 1
    want = 2 * np.bincount(ids, minlength=v) + np.bincount(ids[:100], minlength=v)
    assert np.array_equal(d_counts.cpu().numpy(), want)


def test_count_pieces(tmp_path):
    """CountPieces: the counts of the golden id rows, accumulated over two calls."""
    c = _case("unigram_byte")
    out = _run(c.model_path, [_cmd("count", c.text_path, 0, 300), _cmd("count", c.text_path, 300, 700)])
    want = np.bincount(np.concatenate([np.asarray(r, np.int64) for r in c.golden[:1000]]), minlength=len(c.pieces))
    got = dict(tuple(map(int, kv.split(b":"))) for kv in out[1].split()[1:])
    assert got == {i: int(x) for i, x in enumerate(want) if x}
    first = np.bincount(np.concatenate([np.asarray(r, np.int64) for r in c.golden[:300]]), minlength=len(c.pieces))
    assert dict(tuple(map(int, kv.split(b":"))) for kv in out[0].split()[1:]) == {i: int(x) for i, x in enumerate(first) if x}
