"""GPU: spm_hip_nbest_encode_batch against the Python restatement of the
reference's n-best search (tests/nbest_ref.py), bit for bit: ids, piece
lengths, both offset levels and the scores' float32 bit patterns."""
import os

import numpy as np
import pytest

import model_reader
import nbest_ref as NB
import oracle_lib as O
import sample_ref as R
import spm_amd as S
from model_builder import NORMAL, UNIGRAM, UNUSED, USER_DEFINED, model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

pytestmark = pytest.mark.gpu


def _read(name):
    return open(os.path.join(GOLD, name), "rb").read()


def _nbest(dm, sents, nbest, **kw):
    buf, off = S.to_csr(sents)
    return dm.nbest_encode_csr_host(buf, off, nbest, with_lens=True, **kw)


def _rows(ids, tok_off, path_off, scores, lens):
    """Per sentence: [(ids, lens, score bits)] in path order."""
    bits = scores.view(np.uint32)
    out = []
    for i in range(len(path_off) - 1):
        paths = []
        for p in range(int(path_off[i]), int(path_off[i + 1])):
            a, b = int(tok_off[p]), int(tok_off[p + 1])
            paths.append((ids[a:b].tolist(), lens[a:b].tolist(), int(bits[p])))
        out.append(paths)
    return out


def _want(rm, sents, nbest):
    return [[(p[0], p[1], NB.score_bits(p[2])) for p in NB.nbest(rm, s, nbest)[0]] for s in sents]


def _check(dm, rm, sents, nbest):
    got = _nbest(dm, sents, nbest)
    ids, tok_off, path_off, scores, lens = got
    assert int(path_off[0]) == 0 and int(tok_off[0]) == 0
    assert int(path_off[-1]) == len(tok_off) - 1 == len(scores) and int(tok_off[-1]) == len(ids) == len(lens)
    rows, want = _rows(*got), _want(rm, sents, nbest)
    for i, (a, b) in enumerate(zip(rows, want)):
        assert a == b, (i, sents[i])
    return rows


@pytest.fixture(scope="module")
def botchan():
    """300 normalized botchan lines on test_model.model, the device model and
    the restatement's 5 best of each, computed once."""
    mb = _read("test_model.model")
    lines = O.read_lines_binary(os.path.join(GOLD, "botchan.txt"))[:300]
    dm = S.DeviceModel(mb)
    norm = dm.normalize(lines)
    rm = R.Model(mb)
    return dm, rm, norm, _want(rm, norm, 5)


def test_known_answers():
    """UnigramModelTest.ModelNBestTest / LatticeTest.NBestTest."""
    dm = S.DeviceModel(NB.abc_model())
    names = {3: "a", 4: "b", 5: "c", 6: "ab", 7: "bc", 8: "abc"}
    rows = _rows(*_nbest(dm, [b"abc", b""], 10))
    assert [" ".join(names[i] for i in p[0]) for p in rows[0]] == NB.ABC_ORDER
    assert [p[2] for p in rows[0]] == [NB.score_bits(x) for x in (10.0, 5.0, 2.0, 0.0)]
    assert rows[1] == [([], [], 0)]
    # nbest_size beyond the clamp: still the lattice's 4 paths.
    assert _rows(*_nbest(dm, [b"abc"], 5000))[0] == rows[0]


@pytest.mark.parametrize("nbest", [2, 5])
def test_restatement_parity_botchan(botchan, nbest):
    dm, rm, norm, want5 = botchan
    rows = _check(dm, rm, norm, nbest)
    if nbest == 5:
        assert rows == want5


def test_restatement_parity_botchan_64(botchan):
    dm, rm, norm, _ = botchan
    _check(dm, rm, norm[:100], 64)


def test_restatement_parity_wagahaiwa():
    mb = _read("test_ja_model.model")
    lines = O.read_lines_binary(os.path.join(GOLD, "wagahaiwa_nekodearu.txt"))[:40]
    dm = S.DeviceModel(mb)
    _check(dm, R.Model(mb), dm.normalize(lines), 4)


def test_restatement_parity_all_ties():
    mb = NB.ties_model()
    _check(S.DeviceModel(mb), R.Model(mb), [b"a" * 24], 64)


@pytest.mark.parametrize("nbest", [1, 0])
def test_one_best_is_the_plain_encode(botchan, nbest):
    dm, rm, norm, _ = botchan
    buf, off = S.to_csr(norm)
    ids, lens, to = dm.encode_csr_host(buf, off, with_lens=True)
    gids, gtok, gpath, gscores, glens = _nbest(dm, norm, nbest)
    assert np.array_equal(gpath, np.arange(len(norm) + 1, dtype=np.uint64))
    assert np.array_equal(gtok, to) and np.array_equal(gids, ids) and np.array_equal(glens, lens)


@pytest.mark.parametrize("nbest", [3, 8])
def test_brute_force_top_n(botchan, nbest):
    """60 distinct 12-char prefixes of botchan lines (up to 180 paths each):
    the path count is min(N, paths), and wherever the float64 totals of the
    N-th and (N+1)-th best path differ by more than 1e-3 the returned set is
    the exact top N.  On the CPU all 60 of the 60 sentences have such a gap
    (or at most N paths) at both N = 3 and N = 8."""
    dm, rm, norm, _ = botchan
    sents = NB.short_sentences(norm)
    rows = _rows(*_nbest(dm, sents, nbest))
    clear = 0
    for s, paths in zip(sents, rows):
        got = {(tuple(p[0]), tuple(p[1])) for p in paths}
        total, want = NB.exact_top(rm, s, nbest)
        assert len(paths) == len(got) == min(nbest, total)
        if want is not None:
            clear += 1
            assert got == want, s
    assert 2 * clear >= len(sents)


def test_edge_lattices():
    """UNUSED and USER_DEFINED pieces, chars with no piece, a NUL byte, a trie
    leaf inside a UTF-8 char, an empty sentence between non-empty ones."""
    pcs = model_reader.read_pieces(_read("test_model.model"))
    pcs = [(p, s, UNUSED if p == "▁the".encode() else t) for p, s, t in pcs]
    pcs += [("<tag>", 0.0, USER_DEFINED), (b"\xe2\x96", -8.0, NORMAL)]
    mb = model(pcs, UNIGRAM)
    sents = ["▁the▁a".encode(), b"", "▁a<tag>b".encode(), "▁a☃☃b".encode(), b"", b"ab\x00cd", b"\x00",
             "▁ab".encode() + b"\xe2\x96", "a▁b▁".encode(), b"\x80", b"a\xffb", b"\xf0\x9f", "▁".encode()]
    dm, rm = S.DeviceModel(mb), R.Model(mb)
    for nbest in (1, 2, 7):
        rows = _check(dm, rm, sents, nbest)
        assert rows[1] == rows[4] == [([], [], 0)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_shape(botchan, n):
    dm, rm, norm, want5 = botchan
    assert _rows(*_nbest(dm, norm[:n], 5)) == want5[:n]


def test_tiers(botchan):
    """Arenas of 64 and 200 hypotheses (the measured maximum at N = 5 is 257):
    sentences move to the second tier and to the host, results do not move."""
    dm, rm, norm, want5 = botchan
    try:
        dm.set_nbest_max_hyps(64, 200)
        assert _rows(*_nbest(dm, norm, 5)) == want5
        second, host = dm.nbest_stats()
        assert second > 0 and host > 0 and host <= second
    finally:
        dm.set_nbest_max_hyps(0, 0)
    assert _rows(*_nbest(dm, norm, 5)) == want5
    assert dm.nbest_stats()[1] == 0


def test_shrink_goes_to_the_host():
    mb = NB.ties_model()
    dm = S.DeviceModel(mb)
    _check(dm, R.Model(mb), [b"aa", b"a" * 3000, b"aaa"], 512)
    assert dm.nbest_stats()[1] == 1


def test_status_and_capacity(botchan):
    dm, rm, norm, want5 = botchan
    buf, off = S.to_csr(["▁hello".encode()])
    with pytest.raises(S.SpmError) as e:
        S.DeviceModel(_read("botchan_bpe1k.model")).nbest_encode_csr_host(buf, off, 5)
    assert e.value.code == 12  # SPM_UNIMPLEMENTED
    with pytest.raises(S.SpmError) as e:
        S.DeviceModel(_read("test_model.model"), host_only=True).nbest_encode_csr_host(buf, off, 5)
    assert e.value.code == 9  # SPM_FAILED_PRECONDITION
    # Too-small capacities: RESOURCE_EXHAUSTED with totals that then suffice
    # (nbest_encode_csr_host repeats the call with them).
    assert _rows(*_nbest(dm, norm[:50], 5, capacities=(7, 3))) == want5[:50]
    import ctypes
    b50, o50 = S.to_csr(norm[:50])
    tp, tt = ctypes.c_uint64(), ctypes.c_uint64()
    z = np.zeros(8, dtype=np.uint64)
    po = np.full(51, 77, dtype=np.uint64)
    rc = S.lib().spm_hip_nbest_encode_batch_host(dm.h, S._p(b50), S._p(o50), 50, 5, S._p(z.view(np.int32)), None, 7,
                                                 S._p(z), S._p(z.view(np.float32)), 3, S._p(po), ctypes.byref(tp),
                                                 ctypes.byref(tt))
    assert rc == 8  # SPM_RESOURCE_EXHAUSTED
    assert tp.value == sum(len(r) for r in want5[:50]) and tt.value == sum(len(p[0]) for r in want5[:50] for p in r)
    assert (po == 77).all() and not z.any()  # nothing final was written
    ids, tok_off, path_off, scores = dm.nbest_encode_csr_host(*S.to_csr([]), 5)
    assert ids.size == 0 and tok_off.tolist() == [0] and path_off.tolist() == [0]


def test_device_pointer_call(botchan):
    import torch
    dm, rm, norm, want5 = botchan
    sents = norm[:120]
    buf, off = S.to_csr(sents)
    dev = torch.device("cuda", 0)
    n, N = len(sents), 5
    d_b = torch.from_numpy(buf).to(dev)
    d_o = torch.from_numpy(off.view(np.int64)).to(dev)
    tcap, pcap = N * int(off[-1]), N * n  # the capacities that always suffice
    d_ids = torch.empty(tcap, dtype=torch.int32, device=dev)
    d_len = torch.empty(tcap, dtype=torch.int32, device=dev)
    d_tok = torch.empty(pcap + 1, dtype=torch.int64, device=dev)
    d_sc = torch.empty(pcap, dtype=torch.float32, device=dev)
    d_po = torch.empty(n + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    P, T = dm.nbest_encode_device(d_b.data_ptr(), d_o.data_ptr(), n, N, d_ids.data_ptr(), tcap, d_tok.data_ptr(),
                                  d_sc.data_ptr(), pcap, d_po.data_ptr(), d_len=d_len.data_ptr())
    rows = _rows(d_ids.cpu().numpy()[:T], d_tok.cpu().numpy().view(np.uint64)[:P + 1],
                 d_po.cpu().numpy().view(np.uint64), d_sc.cpu().numpy()[:P], d_len.cpu().numpy()[:T].view(np.uint32))
    assert rows == want5[:120]
    with pytest.raises(S.SpmError) as e:
        dm.nbest_encode_device(d_b.data_ptr(), d_o.data_ptr(), n, N, d_ids.data_ptr(), 10, d_tok.data_ptr(),
                               d_sc.data_ptr(), pcap, d_po.data_ptr())
    assert e.value.code == 8 and e.value.totals == (P, T)
