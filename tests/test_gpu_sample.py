"""GPU: unigram SampleEncode (spm_hip_sample_encode_batch) against the Python
restatement tests/sample_ref.py and against exact path probabilities."""
import math
import os

import numpy as np
import pytest

import model_reader
import oracle_lib as O
import sample_ref as R
import spm_amd as S
from model_builder import NORMAL, UNIGRAM, UNUSED, USER_DEFINED, model
from sample_ref import ABC_THETAS, abc_expected, abc_model, abc_name

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

pytestmark = pytest.mark.gpu

THETA = 0.5
SEED = 20240611
MARGIN = 1e-3  # a sentence may differ from the restatement only below this margin


def _read(name):
    return open(os.path.join(GOLD, name), "rb").read()


def _sample(dm, sents, theta=THETA, seed=SEED, index_base=0):
    buf, off = S.to_csr(sents)
    ids, lens, to = dm.sample_encode_csr_host(buf, off, theta, seed, index_base=index_base, with_lens=True)
    return ids, lens, to


def _rows(ids, lens, to):
    return [(ids[int(to[i]):int(to[i + 1])].tolist(), lens[int(to[i]):int(to[i + 1])].tolist())
            for i in range(len(to) - 1)]


def _must_flag(rm, s):
    """What the fast tier hands to the exact tier (include/spm_hip.h): a walk
    still alive after 64 bytes, a trie leaf inside a UTF-8 char, more than 16
    nodes ending at one position."""
    lat = rm.lattice(s)
    starts = set(lat.cs)
    if any(len(x) > 16 for x in lat.end_nodes):
        return True
    for p in range(lat.nc):
        for q in range(lat.cs[p], len(s)):
            key = s[lat.cs[p]:q + 1]
            if s[q] == 0 or key not in rm.prefixes:
                break
            if len(key) > 64:
                return True
            if key in rm.table and q + 1 not in starts:
                return True
    return False


def _check_against_ref(rm, sents, got, theta, seed, index_base=0, max_differ=0.005):
    """Every output is a path; a sentence differs from the restatement only
    when its margin there is below MARGIN; at most max_differ of them do."""
    differ = 0
    for i, s in enumerate(sents):
        ids, lens = got[i]
        assert rm.is_path(s, ids, lens) if s else (ids, lens) == ([], []), i
        wids, wlens, margin = rm.sample(s, theta, seed, index_base + i)
        if (ids, lens) != (wids, wlens):
            assert margin < MARGIN, (i, margin, ids, wids)
            differ += 1
    assert differ <= max_differ * len(sents), differ
    return differ


@pytest.fixture(scope="module")
def botchan():
    """2 000 normalized botchan lines, test_model.model, and their samples at
    THETA on the device (default tiers), computed once."""
    mb = _read("test_model.model")
    lines = O.read_lines_binary(os.path.join(GOLD, "botchan.txt"))[:2000]
    dm = S.DeviceModel(mb)
    norm = dm.normalize(lines)
    got = _sample(dm, norm)
    stats = dm.stats()
    return mb, dm, norm, got, stats


def test_reference_kat_abc():
    """LatticeTest.SampleTest (unigram_model_test.cc:317-357) on the device:
    100 000 copies of "ABC", the reference's five thetas and its 0.02."""
    dm = S.DeviceModel(abc_model())
    n = 100000
    for t, theta in enumerate(ABC_THETAS):
        ids, lens, to = _sample(dm, [b"ABC"] * n, theta=theta, seed=77 + t)
        freq = {}
        for r_ids, r_lens in _rows(ids, lens, to):
            k = abc_name(r_ids)
            freq[k] = freq.get(k, 0) + 1
        want = abc_expected(theta)
        assert set(freq) == set(want), (theta, freq)
        for k in want:
            print("theta %.2f %-6s device %.5f exact %.5f" % (theta, k, freq[k] / n, want[k]))
            assert abs(freq[k] / n - want[k]) < 0.02, (theta, k)


def _distribution_cases():
    mb = _read("test_model.model")
    pcs = model_reader.read_pieces(mb)
    ud = model(pcs + [("<tag>", 0.0, USER_DEFINED)], UNIGRAM)
    un = model([(p, s, UNUSED if p == "▁the".encode() else t) for p, s, t in pcs], UNIGRAM)
    return [("plain", mb, "▁hello"), ("plain", mb, "▁a▁b"), ("plain", mb, "▁in▁a"), ("unk", mb, "▁a☃b"),
            ("user_defined", ud, "▁a<tag>b"), ("unused", un, "▁the▁a")]


@pytest.mark.parametrize("case", range(6))
def test_exact_distribution(case):
    """200 000 draws of a short sentence at theta 0 (uniform over paths), 0.5
    and 1.0: every path's frequency within 5 sqrt(p (1 - p) / N) of its exact
    probability, no other path.

    The sentences are chosen (before any device run, from the exact
    probabilities alone) so that the normal bound means something for every
    path: a path with N p of 0.001 .. 0.1 fails it with probability about N p
    under an exact sampler, since one occurrence is already outside.  For
    these six the summed false-alarm probability over all paths and thetas,
    from the Poisson tails, is below 1e-3; the seed is fixed."""
    name, mb, text = _distribution_cases()[case]
    s = text.encode()
    dm, rm = S.DeviceModel(mb), R.Model(mb)
    n = 200000
    for t, theta in enumerate((0.0, 0.5, 1.0)):
        ids, lens, to = _sample(dm, [s] * n, theta=theta, seed=1000 * case + t)
        cnt = np.diff(to).astype(np.int64)
        kmax = int(cnt.max())
        table = np.full((n, 2 * kmax), -1, dtype=np.int64)
        col = np.arange(int(to[-1])) - np.repeat(to[:-1].astype(np.int64), cnt)
        row = np.repeat(np.arange(n), cnt)
        table[row, col] = ids
        table[row, kmax + col] = lens
        uniq, counts = np.unique(table, axis=0, return_counts=True)
        freq = {}
        for u, c in zip(uniq, counts):
            k = int((u[:kmax] >= 0).sum())
            freq[(tuple(int(x) for x in u[:k]), tuple(int(x) for x in u[kmax:kmax + k]))] = int(c)
        want = rm.enumerate_paths(s, theta)
        assert set(freq) <= set(want), (name, theta)
        for path, p in want.items():
            f = freq.get(path, 0) / n
            assert abs(f - p) <= 5 * math.sqrt(p * (1 - p) / n), (name, theta, path, f, p)


def test_draw_parity_botchan(botchan):
    """Draw-level parity with the restatement on 2 000 botchan lines.

    Share of these sentences whose margin under the restatement is below
    1e-3 (the only ones the comparison could excuse), computed on the CPU:
    90 of 2 000 (4.5 %)."""
    mb, dm, norm, got, stats = botchan
    rm = R.Model(mb)
    differ = _check_against_ref(rm, norm, _rows(*got), THETA, SEED)
    print("botchan: %d of %d sentences differ from the restatement" % (differ, len(norm)))
    assert stats.sentences == len(norm)
    assert stats.general_path == sum(_must_flag(rm, s) for s in norm)


def test_draw_parity_japanese():
    """500 wagahaiwa lines on test_ja_model.model (3-byte chars, pieces of up
    to 9 chars).  Share of sentences with margin below 1e-3 under the
    restatement, computed on the CPU: 48 of 500 (9.6 %; these lines average
    780 bytes, some 250 draws each)."""
    mb = _read("test_ja_model.model")
    lines = O.read_lines_binary(os.path.join(GOLD, "wagahaiwa_nekodearu.txt"))[:500]
    dm = S.DeviceModel(mb)
    norm = dm.normalize(lines)
    rm = R.Model(mb)
    got = _sample(dm, norm)
    differ = _check_against_ref(rm, norm, _rows(*got), THETA, SEED)
    print("wagahaiwa: %d of %d sentences differ from the restatement" % (differ, len(norm)))
    assert dm.stats().general_path == sum(_must_flag(rm, s) for s in norm)
    dm.set_force_general(True)
    forced = _sample(dm, norm)
    assert all(np.array_equal(a, b) for a, b in zip(got, forced))


def test_tier_identity(botchan):
    """The exact tier over every sentence gives the fast tier's arrays bit for bit."""
    mb, dm, norm, got, stats = botchan
    dm.set_force_general(True)
    try:
        forced = _sample(dm, norm)
        assert dm.stats().general_path == len(norm)
    finally:
        dm.set_force_general(False)
    for a, b in zip(got, forced):
        assert np.array_equal(a, b)
    assert stats.general_path < len(norm) // 10


def _edge_model(half=False):
    pcs = model_reader.read_pieces(_read("test_model.model"))
    p20 = "▁".encode() + b"q" * 17   # 20 bytes
    p70 = "▁".encode() + b"z" * 67   # 70 bytes: beyond the fast tier's 64
    extra = [(p20, -9.0, NORMAL), (p70, -9.5, NORMAL)]
    if half:
        extra.append((b"\xe2\x96", -8.0, NORMAL))  # a piece that ends inside the char "▁"
    return model(pcs + extra, UNIGRAM), p20, p70


def _edge_sentences(p20, p70):
    long_text = ("▁the▁quick▁brown▁fox▁jumps▁over▁the▁lazy▁dog" * 100)[:4096].encode()
    return [b"", b"a", b"\x80", "▁ab".encode() + b"\xe2\x96", b"ab\x00cd", b"a\xffb", long_text,
            p20, p20 + b"qq", b"x" + p20, p70, p70 + b"zz", b"the" + p70 + b"s", "▁".encode(),
            b"", "▁a☃b".encode(), b"\xf0\x9f", b"\x00", b"\x00\x00a"]


def _edge_run(mb, sents, want_flags):
    dm, rm = S.DeviceModel(mb), R.Model(mb)
    got = _sample(dm, sents)
    st = dm.stats()
    _check_against_ref(rm, sents, _rows(*got), THETA, SEED, max_differ=1.0)
    flags = [_must_flag(rm, s) for s in sents]
    assert [i for i, f in enumerate(flags) if f] == want_flags
    assert st.general_path == len(want_flags)
    dm.set_force_general(True)
    forced = _sample(dm, sents)
    assert dm.stats().general_path == len(sents)
    for a, b in zip(got, forced):
        assert np.array_equal(a, b)


def test_edge_inputs():
    """Empty, one char, a lone continuation byte, a truncated lead byte at
    the end, an embedded NUL, 0xFF, 4 096 chars, pieces of 20 and 70 bytes."""
    mb, p20, p70 = _edge_model()
    sents = _edge_sentences(p20, p70)
    assert len(sents[6].decode()) == 4096
    # The fast tier hands on exactly the walks that pass 64 bytes.
    _edge_run(mb, sents, [10, 11, 12])


def test_edge_leaf_inside_char():
    """A piece that ends inside a UTF-8 char: the reference rounds its node up
    to the char's end (get_chars_length); such sentences take the exact tier."""
    mb, p20, p70 = _edge_model(half=True)
    sents = ["▁".encode(), "▁ab".encode() + b"\xe2\x96", "a▁b▁".encode(), b"ab", b"\xe2\x96", b""]
    _edge_run(mb, sents, [0, 1, 2])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257])
def test_shapes(botchan, n):
    """A call of the first n sentences gives what they got in the call of all."""
    mb, dm, norm, got, stats = botchan
    part = _rows(*_sample(dm, norm[:n]))
    assert part == _rows(*got)[:n]


def test_stream_properties(botchan):
    mb, dm, norm, got, stats = botchan
    sents = norm[:1000]
    whole = _rows(*got)[:1000]
    assert _rows(*_sample(dm, sents)) == whole                       # same seed twice
    assert _rows(*_sample(dm, sents, seed=SEED + 1)) != whole        # another seed
    a = _rows(*_sample(dm, sents[:300], index_base=0))
    b = _rows(*_sample(dm, sents[300:], index_base=300))
    assert a + b == whole                                            # split calls
    # A result depends on the sentence and its global index only: sentence
    # 700 at index 700 of a different batch.
    other = [sents[700]] * 5 + [b"filler"]
    r = _rows(*_sample(dm, other, index_base=696))
    assert r[4] == whole[700]


def test_device_pointer_call(botchan):
    import torch
    mb, dm, norm, got, stats = botchan
    sents = norm[:300]
    buf, off = S.to_csr(sents)
    dev = torch.device("cuda", 0)
    d_b = torch.from_numpy(buf).to(dev)
    d_o = torch.from_numpy(off.view(np.int64)).to(dev)
    cap = max(int(off[-1]), 1)
    d_ids = torch.empty(cap, dtype=torch.int32, device=dev)
    d_len = torch.empty(cap, dtype=torch.int32, device=dev)
    d_tok = torch.empty(len(sents) + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    dm.sample_encode_device(d_b.data_ptr(), d_o.data_ptr(), len(sents), THETA, SEED, d_ids.data_ptr(),
                            d_tok.data_ptr(), d_len=d_len.data_ptr())
    to = d_tok.cpu().numpy().view(np.uint64)
    k = int(to[-1])
    rows = _rows(d_ids.cpu().numpy()[:k], d_len.cpu().numpy()[:k].view(np.uint32), to)
    assert rows == _rows(*got)[:300]


def test_status_codes():
    bpe = S.DeviceModel(_read("botchan_bpe1k.model"))
    buf, off = S.to_csr(["▁hello".encode()])
    with pytest.raises(S.SpmError) as e:
        bpe.sample_encode_csr_host(buf, off, THETA, SEED)
    assert e.value.code == 12  # SPM_UNIMPLEMENTED
    dm = S.DeviceModel(_read("test_model.model"))
    with pytest.raises(S.SpmError) as e:
        dm.sample_encode_csr_host(buf, off, float("nan"), SEED)
    assert e.value.code == 3  # SPM_INVALID_ARGUMENT
    ids, to = dm.sample_encode_csr_host(*S.to_csr([]), THETA, SEED)
    assert ids.size == 0 and to.tolist() == [0]
