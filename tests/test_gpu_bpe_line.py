"""GPU: BPE models on the one-launch per-line path (csrc/bpe_line.hip:
bpe_raw_kernel behind spm_hip_encode_raw_small_host, bpe_small_kernel behind
spm_hip_encode_batch_host for <= 16 sentences, which SPM_HIP_BPE_SMALL_HOST=1
switches on -- every test here runs with it), against the CPU oracle, which
restates the reference's bpe::Model::Encode and Encode(line, &ids).

Which path served a call is read from the call's stats: a call the line
kernel took has general_path == 0 and coop_rest == 0 whatever its length; a
call it handed back has coop_rest == n; the staged path it then takes sends
every sentence past the batch kernels' 64 bytes to the general kernel
(general_path), so a long sentence tells a taken call from a skipped one.
For the processor and the CLI, SPM_HIP_SMALL_STATS=1 prints the handle's
counts when it is freed."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import bpe_cases as C
import byte_fallback_ref as R
import oracle_lib as O
import spm_amd as S
import vocab_ref as V
from model_builder import BPE, model
from model_reader import read_pieces

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CLI = os.path.join(ROOT, "sentencepiece-comments_amd", "lib", "spm_encode")
LINE_MAX = 1024  # kBpeLineMaxBytes, and the raw bytes one line may have (kRawMaxBytes)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _small_host_on(monkeypatch):
    monkeypatch.setenv("SPM_HIP_BPE_SMALL_HOST", "1")

EDGE_LINES = [b"", b"   ", b"\t a  b \t", b"  lead", b"trail   ", b"\xff\xfe", b"a\x00b", b"\xe3\x81",
              "☃ ♞ 𝄞 ∀".encode(), b"x" * 1000, "▁▁ ▁".encode()]


def _rows(x):
    return [list(map(int, r)) for r in x]


class _Botchan:
    """botchan_bpe1k.model, its corpus and the oracle's answers to the raw
    calls of test 1 (shared: the restriction test ends on the same calls)."""

    def __init__(self):
        self.mb = open(os.path.join(GOLD, "botchan_bpe1k.model"), "rb").read()
        self.lines = O.read_lines_binary(os.path.join(GOLD, "botchan.txt"))
        self.om = O.OracleModel(self.mb)
        pool = self.lines + EDGE_LINES
        rng = np.random.default_rng(8)
        self.calls = []
        for t in range(300):
            n = 1 if t % 2 else int(rng.integers(1, 17))
            batch = [pool[int(x)] for x in rng.integers(0, len(self.lines), n)]
            if t < len(EDGE_LINES):
                batch = [pool[-1 - t]]
            self.calls.append(batch)
        self.want = [_rows(self.om.encode_lines(b)) for b in self.calls]


_botchan = []


def _bc():
    if not _botchan:
        _botchan.append(_Botchan())
    return _botchan[0]


def _csr_check(dm, om, sents, what):
    """One encode_csr_host call: ids, piece lengths and token offsets equal
    the oracle's.  Returns the call's stats."""
    buf, off = S.to_csr(sents)
    ids, lens, tok = dm.encode_csr_host(buf, off, with_lens=True)
    rids, rlens, rtok = om.encode_normalized_csr(buf, off, with_lens=True)
    assert np.array_equal(tok, rtok) and np.array_equal(ids, rids) and np.array_equal(lens, rlens), what
    return dm.stats()


def _cli_ids(model_bytes, lines, tmp_path, name):
    """lib/spm_encode, one Encode(line) per line: (ids rows, counts of the
    handle's BPE small calls by outcome)."""
    mp, tp = tmp_path / (name + ".model"), tmp_path / (name + ".txt")
    mp.write_bytes(model_bytes)
    tp.write_bytes(b"".join(l + b"\n" for l in lines))
    p = subprocess.run([CLI, "--model=%s" % mp, "--output_format=id", "--batch_lines=1", str(tp)],
                       capture_output=True, timeout=120, env=dict(os.environ, SPM_HIP_SMALL_STATS="1"))
    assert p.returncode == 0, p.stderr.decode()
    rows = [list(map(int, r.split())) for r in p.stdout.decode().split("\n")[:-1]]
    m = re.search(r"bpe line calls taken=(\d+) refused=(\d+) skipped=(\d+)", p.stderr.decode())
    assert m, p.stderr.decode()
    return rows, tuple(int(x) for x in m.groups())


def test_raw_lines_botchan():
    """1. Raw lines on a real model: 300 calls of 1 line or 1-16 lines of
    botchan.txt and the edge lines; every call is taken and equals the
    oracle.  (Before bpe_raw_kernel every one of them returned None.)"""
    bc = _bc()
    assert max(len(l) for l in bc.lines) <= LINE_MAX
    dm = S.DeviceModel(bc.mb)
    for t, (batch, want) in enumerate(zip(bc.calls, bc.want)):
        got = dm.encode_raw_small(batch)
        assert got is not None, (t, batch)
        assert _rows(got) == want, (t, batch)
        st = dm.stats()
        assert st.sentences == len(batch) and st.coop_rest == 0 and st.tokens == sum(len(w) for w in want)
    assert dm.encode_raw_small([b"y" * 1500]) is None  # past the normalizer's prefix table: not taken
    assert dm.stats().coop_rest == 1
    dm.close()


def _merge_order_sentences():
    out = [b"a" * L for L in (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024)]
    for k in (31, 32, 33, 63, 64, 65, 511, 512):        # 62 .. 1024 bytes
        out.append(b"ab" * k)
    for k in (21, 22, 42, 43, 341):                      # 63, 66, 126, 129, 1023 bytes
        out.append("あ".encode() * k)
    rng = np.random.default_rng(20240)
    for _ in range(40):
        want = int(rng.integers(200, 1001))
        s = b""
        while True:
            c = C.ALPHABET[int(rng.integers(0, len(C.ALPHABET)))].encode()
            if len(s) + len(c) > want:
                break
            s += c
        out.append(s)
    return out


@pytest.mark.parametrize("ties", [False, True])
def test_merge_order_lane_ownership(ties):
    """2. The merge order on every ownership boundary (a lane owns ceil(nb /
    64) positions): runs of one letter, where every pair ties and the left
    index decides, two-char and three-byte runs on both sides of 64, 128 and
    1024 bytes, random sentences of 200-1000 bytes, the edge and malformed
    sentences.  One normalized sentence per call."""
    spec = C.build_model(ties=ties)
    dm, om = S.DeviceModel(spec.blob), O.OracleModel(spec.blob)
    for s in _merge_order_sentences():
        st = _csr_check(dm, om, [s], s)
        assert len(s) <= LINE_MAX and st.general_path == 0 and st.coop_rest == 0, (s, st.general_path, st.coop_rest)
    for s in C.malformed() + [b"ab" * 513, "あ".encode() * 342]:
        st = _csr_check(dm, om, [s], s)
        assert st.coop_rest == (1 if len(s) > LINE_MAX else 0), s
    # One byte past the bound: handed back, and the staged path's general
    # kernel gives the oracle's result.
    st = _csr_check(dm, om, [b"a" * 1025], "1025")
    assert st.coop_rest == 1 and st.general_path == 1
    dm.close()


def _differs(om_a, om_b, cands, raw):
    """The first candidate the two oracles segment differently."""
    for s in cands:
        a = om_a.encode_lines([s]) if raw else om_a.encode_normalized([s])
        b = om_b.encode_lines([s]) if raw else om_b.encode_normalized([s])
        if _rows(a) != _rows(b):
            return s
    raise AssertionError("no candidate pushes an UNUSED piece")


def test_refusals(tmp_path):
    """3. What the line kernel refuses, and that the answer stays the
    oracle's: a pushed UNUSED piece, a char outside an irregular model's
    vocabulary, a USER_DEFINED model, a byte-fallback model."""
    plain = O.OracleModel(C.build_model().blob)
    cands = [p.encode() for p in C.UNUSED_PIECES]
    # unused: where the oracle's segmentation changes, an UNUSED piece was pushed.
    spec = C.build_model(unused=True)
    dm, om = S.DeviceModel(spec.blob), O.OracleModel(spec.blob)
    s_norm, s_raw = _differs(om, plain, cands, False), _differs(om, plain, cands, True)
    assert _csr_check(dm, om, [s_norm], s_norm).coop_rest == 1
    assert dm.encode_raw_small([s_raw]) is None and dm.stats().coop_rest == 1
    rows, (taken, refused, skipped) = _cli_ids(spec.blob, [s_raw, b"zz", s_raw], tmp_path, "unused")
    assert rows == _rows(om.encode_lines([s_raw, b"zz", s_raw])) and (taken, refused, skipped) == (1, 2, 0)
    dm.close()
    # irregular: "l" and "ö" are no pieces of their own.
    spec = C.build_model(irregular=True)
    dm, om = S.DeviceModel(spec.blob), O.OracleModel(spec.blob)
    for d in C.DROPPED:
        s = ("ab" + d + "ab").encode()
        assert _csr_check(dm, om, [s], s).coop_rest == 1
        assert dm.encode_raw_small([s]) is None and dm.stats().coop_rest == 1
    assert _csr_check(dm, om, [b"abab"], "abab").coop_rest == 0
    assert _rows(dm.encode_raw_small([b"abab"])) == _rows(om.encode_lines([b"abab"]))
    lines = ["abl".encode(), b"abab", "öa".encode()]
    rows, counts = _cli_ids(spec.blob, lines, tmp_path, "irregular")
    assert rows == _rows(om.encode_lines(lines)) and counts == (1, 2, 0)
    dm.close()
    # USER_DEFINED pieces: the general kernel only; the line kernel is never tried.
    spec = C.build_model(user_defined=True)
    dm, om = S.DeviceModel(spec.blob), O.OracleModel(spec.blob)
    assert dm.info().fast_variant == C.TIER_GENERAL
    st = _csr_check(dm, om, [b"ab<tag>ab"], "user_defined")
    assert st.coop_rest == 0 and st.general_path == 1   # (host-sized general path: every sentence)
    assert dm.encode_raw_small([b"ab<tag>ab"]) is None
    lines = [b"ab<tag>ab", b"abab"]
    rows, counts = _cli_ids(spec.blob, lines, tmp_path, "user_defined")
    assert rows == _rows(om.encode_lines(lines)) and counts == (0, 0, 0)
    dm.close()
    # Byte fallback: unknown runs expand to bytes in the id epilogue, which the fused raw launch has not.
    mb = open(os.path.join(GOLD, "botchan_bf_bpe1k.model"), "rb").read()
    dm, om = S.DeviceModel(mb), O.OracleModel(mb)
    lines = _bc().lines[:20]
    assert dm.encode_raw_small(lines[:3]) is None
    _csr_check(dm, om, om.normalize(lines[:8]), "byte fallback")   # (model-level tokens: unknown chars stay <unk>)
    off, ids, _, _ = R.recorded_spt("botchan", "botchan_bf_bpe1k")   # the reference's ids, bytes expanded
    rows, counts = _cli_ids(mb, lines, tmp_path, "bf")
    assert rows == [ids[int(off[i]):int(off[i + 1])].tolist() for i in range(20)] and counts == (0, 0, 0)
    dm.close()


def test_back_off():
    """3 (continued). 8 refusals in a row switch the line kernel off, every
    64th call tries it again, and a call it takes resets the count."""
    spec = C.build_model(unused=True)
    dm, om = S.DeviceModel(spec.blob), O.OracleModel(spec.blob)
    plain = O.OracleModel(C.build_model().blob)
    refused = _differs(om, plain, [p.encode() for p in C.UNUSED_PIECES], False)
    free = b"z" * 300  # no pair at all: always taken; the staged path sends it to the general kernel
    for k in range(8):
        assert _csr_check(dm, om, [refused], k).coop_rest == 1
    assert _csr_check(dm, om, [refused], 8).coop_rest == 0         # the 9th: skipped
    for k in range(55):                                              # rejects 9 .. 63: skipped
        st = _csr_check(dm, om, [free], k)
        assert st.coop_rest == 0 and st.general_path == 1, k
    st = _csr_check(dm, om, [free], "retry")                         # rejects == 64: tried, and taken
    assert st.coop_rest == 0 and st.general_path == 0
    assert _csr_check(dm, om, [refused], "after reset").coop_rest == 1
    assert dm.encode_raw_small([refused]) is None and dm.stats().coop_rest == 1  # raw calls share the count
    dm.close()


def _ws_fuzz_lines(seed, n):
    """Whitespace-heavy raw lines: runs of spaces and tabs, leading and
    trailing runs, literal U+2581, ideographic spaces, chars inside and
    outside the mini vocabulary, lines long enough to cross the normalizer's
    64-position blocks."""
    rng = np.random.default_rng(seed)
    toks = [" ", "  ", "   ", "\t", "a", "bc", "hello", "é", "▁", "▁▁", "　", "¨", "ﬁ", "ＡＢ", "x" * 70,
            "the", "q", "é" * 5, "abab", "あい", "😀"]
    out = [b"", b" ", b"  \t ", "▁".encode(), " ▁ ".encode(), "　a　".encode(), "¨".encode(),
           " ¨ ".encode(), ("a" + " " * 130 + "b").encode(), (" " * 64 + "x").encode(), ("x" + " " * 64).encode()]
    for _ in range(n):
        s = "".join(toks[int(k)] for k in rng.integers(0, len(toks), int(rng.integers(1, 40))))
        out.append(s.encode()[:1000])
    return out


@pytest.mark.parametrize("flags", [
    dict(),
    dict(remove_extra_whitespaces=False),
    dict(add_dummy_prefix=False),
    dict(treat_ws_as_suffix=True),
    dict(escape_whitespaces=False),
    dict(remove_extra_whitespaces=False, add_dummy_prefix=False, treat_ws_as_suffix=True)])
def test_normalizer_flags(flags):
    """4. The raw-line normalizer in front of the BPE encode on every flag
    combination of the spec.  The model is regular, so every call whose lines
    have at most 1024 bytes, raw and normalized, is taken."""
    mb = model(C.build_model().pieces, BPE, **flags)
    dm, om = S.DeviceModel(mb), O.OracleModel(mb)
    lines = _ws_fuzz_lines(11, 240)
    for i in range(0, len(lines), 4):
        batch = lines[i:i + 4] if (i // 4) % 2 else lines[i:i + 1]
        got = dm.encode_raw_small(batch)
        fits = all(len(r) <= LINE_MAX and len(x) <= LINE_MAX for r, x in zip(batch, om.normalize(batch)))
        assert (got is not None) == fits, (flags, batch)
        if got is not None:
            assert _rows(got) == _rows(om.encode_lines(batch)), (flags, batch)
    dm.close()


def test_vocabulary_restriction():
    """5. SetVocabulary with the 300 most frequent pieces: the pair entries'
    unused bits change in place, so a call is either handed back or equals the
    oracle on the proto with the same types; after ResetVocabulary every call
    is taken again."""
    bc = _bc()
    pieces = read_pieces(bc.mb)
    rows = open(os.path.join(GOLD, "botchan_bpe1k.ids")).read().split("\n")
    counts = np.bincount(np.array([int(x) for r in rows for x in r.split()], dtype=np.int64), minlength=len(pieces))
    vocab = [pieces[int(i)][0] for i in np.argsort(-counts, kind="stable")[:300]]
    dm = S.DeviceModel(bc.mb)
    dm.set_vocabulary(vocab)
    types = V.set_vocabulary(pieces, vocab)
    assert dm.piece_types().tolist() == types
    om = O.OracleModel(V.retype(bc.mb, types))
    taken = 0
    for line in bc.lines[:100]:
        got = dm.encode_raw_small([line])
        if got is not None:
            taken += 1
            assert _rows(got) == _rows(om.encode_lines([line])), line
    assert taken < 100   # the restriction makes merges push UNUSED pieces
    dm.reset_vocabulary()
    for t, (batch, want) in enumerate(zip(bc.calls[:100], bc.want)):
        got = dm.encode_raw_small(batch)
        assert got is not None and _rows(got) == want, t
    dm.close()


def test_one_workspace_mixed_traffic():
    """6. Raw small calls, 3000-sentence batches and 5-sentence normalized
    small calls interleaved on one handle; call 40 grows the staged image."""
    bc = _bc()
    dm = S.DeviceModel(bc.mb)
    norm = bc.om.normalize(bc.lines[:3000])
    big_buf, big_off = S.to_csr(norm)
    big_want = bc.om.encode_normalized_csr(big_buf, big_off, threads=8, with_lens=True)
    rng = np.random.default_rng(31)
    for t in range(60):
        k = int(rng.integers(0, 3000))
        if t == 40:
            grow = ["▁".encode() + b"abcdefghi" * 110] * 16   # 16 x 993 bytes of input: a larger pinned image
            assert _csr_check(dm, bc.om, grow, t).coop_rest == 0
        elif t % 3 == 0:
            got = dm.encode_raw_small([bc.lines[k]])
            assert got is not None and _rows(got) == _rows(bc.om.encode_lines([bc.lines[k]])), t
        elif t % 3 == 1:
            got = dm.encode_csr_host(big_buf, big_off, with_lens=True)
            for g, w in zip(got, big_want):
                assert np.array_equal(g, w), t
        else:
            st = _csr_check(dm, bc.om, [norm[(k + j) % 3000] for j in range(5)], t)
            assert st.coop_rest == 0 and st.sentences == 5
    dm.close()


def test_threads_share_one_handle():
    """7. 4 host threads (one hardware queue each) make 100 single-line raw
    calls each on one handle."""
    bc = _bc()
    dm = S.DeviceModel(bc.mb)
    want = [_rows(bc.om.encode_lines([l]))[0] for l in bc.lines[:400]]
    errors = []

    def work(tid):
        try:
            for k in range(tid * 100, tid * 100 + 100):
                got = dm.encode_raw_small([bc.lines[k]])
                if got is None or _rows(got)[0] != want[k]:
                    errors.append((tid, k))
        except Exception as e:  # noqa: BLE001 (reported below)
            errors.append((tid, repr(e)))

    threads = [threading.Thread(target=work, args=(t,), daemon=True) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(60)
    assert not any(th.is_alive() for th in threads), "a thread is still running after 60 s"
    assert not errors, errors[:5]
    dm.close()


def test_cli_per_line_and_batch(tmp_path):
    """8. lib/spm_encode on the first 300 lines of botchan.txt equals the
    fixture, as one batch and with one Encode(line) per line; the per-line
    run's 300 calls all went through bpe_raw_kernel."""
    bc = _bc()
    golden = open(os.path.join(GOLD, "botchan_bpe1k.ids"), "rb").read().split(b"\n")[:300]
    tp = tmp_path / "first300.txt"
    tp.write_bytes(b"".join(l + b"\n" for l in bc.lines[:300]))
    out = subprocess.run([CLI, "--model=" + os.path.join(GOLD, "botchan_bpe1k.model"), "--output_format=id", str(tp)],
                         capture_output=True, timeout=120)
    assert out.returncode == 0 and out.stdout.split(b"\n")[:-1] == golden
    rows, counts = _cli_ids(bc.mb, bc.lines[:300], tmp_path, "perline")
    assert rows == [list(map(int, g.split())) for g in golden] and counts == (300, 0, 0)
