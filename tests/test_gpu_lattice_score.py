"""GPU: spm_hip_entropy_batch and spm_hip_sample_encode_and_score_batch against
the `sentencepiece` package's recorded entropies (tests/golden/*.entropy.gz),
the restatement tests/lattice_score_ref.py and exact path probabilities; the
processor's CalculateEntropy / SampleEncodeAndScore through
lattice_score_selftest."""
import math
import os
import subprocess
import time

import numpy as np
import pytest

import lattice_score_ref as L
import make_lattice_score_golden as G
import model_reader
import oracle_lib as O
import sample_ref as R
import spm_amd as S
import vocab_ref
from model_builder import NORMAL, UNIGRAM, UNUSED, USER_DEFINED, model
from test_gpu_sample import _edge_model as sample_edge_model, _rows as sample_rows
from test_lattice_score_cpu import MAX_DIFFERING, REL_BOUND, rel_dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
LIB = os.path.join(ROOT, "sentencepiece-comments_amd", "lib")

pytestmark = pytest.mark.gpu

THETA = 0.5
SEED = 20240611
F32 = np.float32
LINES = {"botchan_test_model": 1000, "botchan_bf_unigram1k": 1000, "wagahaiwa_test_ja_model": 300}


def _read(name):
    return open(os.path.join(GOLD, name), "rb").read()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


_FIX = {}


def fixture_data(name):
    """(model bytes, device model, normalized first lines) of a golden fixture."""
    if name not in _FIX:
        _, corpus, model_name = [f for f in G.FIXTURES if f[0] == name][0]
        mb = _read(model_name)
        dm = S.DeviceModel(mb)
        norm = dm.normalize(O.read_lines_binary(os.path.join(GOLD, corpus))[:LINES[name]])
        _FIX[name] = (mb, dm, norm)
    return _FIX[name]


def _entropy(dm, sents, theta=THETA, with_log_z=False):
    buf, off = S.to_csr(sents)
    return dm.entropy_csr_host(buf, off, theta, with_log_z=with_log_z)


def _entropy_device(dm, sents, theta, skip):
    """The device entry over sents[skip:] of a resident batch: the offsets
    passed start at a non-zero value."""
    import torch
    buf, off = S.to_csr(sents)
    dev = torch.device("cuda", 0)
    d_b = torch.from_numpy(buf).to(dev)
    d_o = torch.from_numpy(off.view(np.int64)).to(dev)
    n = len(sents) - skip
    d_h = torch.empty(n, dtype=torch.float32, device=dev)
    d_z = torch.empty(n, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    dm.entropy_device(d_b.data_ptr(), d_o.data_ptr() + 8 * skip, n, theta, d_h.data_ptr(), d_log_z=d_z.data_ptr())
    return d_h.cpu().numpy(), d_z.cpu().numpy()


@pytest.mark.parametrize("name", [f[0] for f in G.FIXTURES])
def test_entropy_against_the_package(name):
    """The first lines of every fixture at alpha 0, 0.5 and 1: bits equal on
    at least 99 %, the rest within the bound of test_lattice_score_cpu.py;
    through the host entry and through the device entry with a non-zero
    first offset."""
    mb, dm, norm = fixture_data(name)
    gold = G.read_golden(name)[:, :len(norm)]
    assert int(S.to_csr(norm)[1][7]) > 0
    for k, alpha in enumerate(G.ALPHAS):
        host = _entropy(dm, norm, alpha)
        devh, _ = _entropy_device(dm, norm, alpha, skip=7)
        assert np.array_equal(_bits(host[7:]), _bits(devh))
        differ = int((_bits(host) != _bits(gold[k])).sum())
        worst = float(rel_dev(host, gold[k]).max())
        print("%s alpha %.1f: %d of %d lines differ from the package, worst relative deviation %.3g"
              % (name, alpha, differ, len(norm), worst))
        assert differ <= MAX_DIFFERING * len(norm)
        assert worst <= REL_BOUND


@pytest.mark.parametrize("name,count", [("botchan_test_model", 300), ("wagahaiwa_test_ja_model", 40)])
def test_entropy_and_log_z_equal_the_restatement(name, count):
    mb, dm, norm = fixture_data(name)
    rm = R.Model(mb)
    sents = norm[:count]
    h, z = _entropy(dm, sents, THETA, with_log_z=True)
    want = [L.entropy(rm, s, THETA, with_log_z=True) for s in sents]
    assert np.array_equal(_bits(z), _bits([w[1] for w in want]))
    assert np.array_equal(_bits(h), _bits([w[0] for w in want]))


def _score(dm, sents, ns, theta=THETA, seed=SEED, index_base=0):
    buf, off = S.to_csr(sents)
    return dm.sample_encode_and_score_csr_host(buf, off, ns, theta, seed, index_base=index_base, with_lens=True)


def _rows(ids, to, sc, lens):
    return [(ids[int(to[r]):int(to[r + 1])].tolist(), lens[int(to[r]):int(to[r + 1])].tolist(), F32(sc[r]).tobytes())
            for r in range(len(to) - 1)]


def test_tier_identity():
    """set_force_general: bit-identical entropies, log partitions, samples and
    scores; the default run leaves (nearly) everything to the fast tier."""
    for name in ("botchan_test_model", "wagahaiwa_test_ja_model"):
        mb, dm, norm = fixture_data(name)
        sents = norm[:300]
        h, z = _entropy(dm, sents, with_log_z=True)
        assert dm.stats().general_path == 0
        got = _score(dm, sents, 3)
        fast_general = dm.stats().general_path
        dm.set_force_general(True)
        try:
            fh, fz = _entropy(dm, sents, with_log_z=True)
            assert dm.stats().general_path == len(sents)
            forced = _score(dm, sents, 3)
            assert dm.stats().general_path == len(sents)
        finally:
            dm.set_force_general(False)
        assert np.array_equal(_bits(h), _bits(fh)) and np.array_equal(_bits(z), _bits(fz))
        for a, b in zip(got, forced):
            assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                  b.view(np.uint32) if b.dtype == np.float32 else b)
        assert fast_general < len(sents) // 10


# Malformed UTF-8, one of every class (the classes of the decode cases of
# test_byte_fallback_cpu.py): a truncated lead, a lone continuation byte, an
# overlong form, a surrogate, a value past U+10FFFF, bytes that are never
# valid, a truncated lead at the end.
MALFORMED = [b"a\xe6\x97b", b"\x97ab", b"a\xc0\x80b", b"\xed\xa0\x80", b"a\xf4\x90\x80\x80", b"\xff\xf8a", b"ab\xf0\x9f"]


def _edge_model(half=False):
    pcs = model_reader.read_pieces(_read("test_model.model"))
    p70 = "▁".encode() + b"z" * 67   # 70 bytes: beyond the sampler's 64-byte mask
    extra = [(p70, -9.5, NORMAL), ("<tag>", 0.0, USER_DEFINED)]
    if half:
        extra.append((b"\xe2\x96", -8.0, NORMAL))  # a piece that ends inside the char "▁"
    return model(pcs + extra, UNIGRAM), p70


def _check_edges(mb, sents, thetas, rm=None, dm=None):
    """Entropy, log partition and three scored samples of every sentence equal
    the restatement in bits, at every theta, in both tiers."""
    dm = dm or S.DeviceModel(mb)
    rm = rm or R.Model(mb)
    general = {}
    for theta in thetas:
        want = [L.entropy(rm, s, theta, with_log_z=True) for s in sents]
        for forced in (False, True):
            dm.set_force_general(forced)
            try:
                h, z = _entropy(dm, sents, theta, with_log_z=True)
                general[("entropy", forced)] = dm.stats().general_path
                ids, to, sc, lens = _score(dm, sents, 3, theta=theta)
                general[("score", forced)] = dm.stats().general_path
            finally:
                dm.set_force_general(False)
            assert np.array_equal(_bits(h), _bits([w[0] for w in want])), (theta, forced)
            assert np.array_equal(_bits(z), _bits([w[1] for w in want])), (theta, forced)
            rows = _rows(ids, to, sc, lens)
            assert len(rows) == 3 * len(sents)
            for r, (r_ids, r_lens, r_sc) in enumerate(rows):
                s = sents[r // 3]
                score = L.path_score(rm, s, theta, r_ids, r_lens)
                assert score is not None and score.tobytes() == r_sc, (theta, forced, r, r_ids)
    return general


def test_edge_sentences():
    """Empty, one known char, one unknown char, all unknown, malformed UTF-8,
    a NUL byte, a piece of 70 bytes, a USER_DEFINED piece; alpha 0 (ln paths),
    0.5, 60 (the 50 cutoff; the entropy tends to 0) and a negative alpha."""
    mb, p70 = _edge_model()
    sents = [b"", b"a", "☃".encode(), "☃☂☁".encode(), b"ab\x00cd", b"\x00", p70, p70 + b"zz", b"the" + p70 + b"s",
             "▁a<tag>b".encode(), "▁hello▁world".encode(), b""] + MALFORMED
    general = _check_edges(mb, sents, (0.0, THETA, 60.0, -0.75))
    # The entropy's fast tier has no 64-byte limit; the sampler's has.
    assert general[("entropy", False)] == 0 and general[("score", False)] == 3
    assert general[("entropy", True)] == general[("score", True)] == len(sents)
    dm, rm = S.DeviceModel(mb), R.Model(mb)
    h0 = _entropy(dm, sents, 0.0)
    for s, h in zip(sents, h0):
        if s:  # ln(paths), within the bound derived in test_lattice_score_cpu.py
            lat = rm.lattice(s)
            want = math.log(L.count_paths(rm, s, lat=lat))
            nodes, M = sum(len(x) for x in lat.end_nodes), max(1.0, want)
            assert abs(float(h) - want) <= 2.0 ** -24 * M * (M * (nodes + 3 * lat.nc) + 5 * nodes), s
    assert h0[0].tobytes() == F32(-0.0).tobytes()
    # Entropy falls as alpha grows; a sentence with one segmentation has none.
    h05, h60 = _entropy(dm, sents, THETA), _entropy(dm, sents, 60.0)
    assert (h60 <= h05 + 1e-6).all() and float(h60[3]) == 0.0 and float(np.median(h60)) < 1e-3


def test_edge_leaf_inside_char():
    """A piece that ends inside a UTF-8 char gives two nodes of one span:
    those sentences take the exact tier."""
    mb, p70 = _edge_model(half=True)
    sents = ["▁".encode(), "▁ab".encode() + b"\xe2\x96", "a▁b▁".encode(), b"ab", b"\xe2\x96", b""]
    general = _check_edges(mb, sents, (THETA,))
    assert general[("entropy", False)] == 3 and general[("score", False)] == 3
    assert general[("entropy", False)] > 0


RERUN_BYTES = 264000  # above the largest slab of any device pool (262 144 + floor(127 * 140 / A) <= 262 514)


def _rerun_batch(norm, p70):
    """Three short sentences that every fast tier keeps (no "▁": the entropy
    case's model flags that char), then one of RERUN_BYTES bytes that holds
    the 70-byte piece once, between two whole words of running text."""
    sp = "▁".encode()
    text = b"".join(norm) * (RERUN_BYTES // sum(len(s) for s in norm) + 1)
    cut1 = text.rfind(sp, 0, RERUN_BYTES // 2)
    cut2 = text.rfind(sp, 0, RERUN_BYTES - len(p70))
    long = text[:cut1] + p70 + text[cut1:cut2]
    long += b"a" * (RERUN_BYTES - len(long))
    assert len(long) == RERUN_BYTES and long.count(p70) == 1
    return [b"hello", b"a", b"thequickbrownfox", long]


def _rerun_call(call, dm, sents):
    """The call's outputs by sentence, and every float among them."""
    buf, off = S.to_csr(sents)
    if call == "sample_encode_csr_host":
        rows = sample_rows(*dm.sample_encode_csr_host(buf, off, THETA, SEED, with_lens=True))
        return rows, np.zeros(0, F32)
    if call == "entropy_csr_host":
        h, z = dm.entropy_csr_host(buf, off, THETA, with_log_z=True)
        return list(zip(_bits(h).tolist(), _bits(z).tolist())), np.concatenate([h, z])
    ids, to, sc, lens = dm.sample_encode_and_score_csr_host(buf, off, 2, THETA, SEED, with_lens=True)
    rows = _rows(ids, to, sc, lens)
    return [rows[2 * i:2 * i + 2] for i in range(len(sents))], sc


@pytest.mark.parametrize("call", ["sample_encode_csr_host", "entropy_csr_host", "sample_encode_and_score_csr_host"])
def test_exact_tier_rerun_host_sized(call):
    """A flagged sentence longer than the device pool's largest slab: the
    call runs again with host-sized scratch over the whole batch.  The short
    sentences get what a call of them alone gives, the long one what the call
    gives under set_force_general, bit for bit.

    The model is test_gpu_sample.py's edge model.  The sampler's fast tier
    (SampleEncode and SampleEncodeAndScore) flags the walk over the 70-byte
    piece.  The entropy's fast tier has no 64-byte limit (test_edge_sentences)
    and flags only a trie leaf inside a UTF-8 char, so its case takes the edge
    model with the piece that ends inside "▁": with the plain one the long
    sentence stays in the fast tier and nothing runs again."""
    mb, _, p70 = sample_edge_model(half=call == "entropy_csr_host")
    dm = S.DeviceModel(mb)
    sents = _rerun_batch(fixture_data("botchan_test_model")[2], p70)
    t0 = time.perf_counter()
    got, floats = _rerun_call(call, dm, sents)
    t1 = time.perf_counter()
    assert dm.stats().general_path == 4
    short, _ = _rerun_call(call, dm, sents[:3])
    assert dm.stats().general_path == 0
    dm.set_force_general(True)
    try:
        t2 = time.perf_counter()
        forced, _ = _rerun_call(call, dm, sents)
        t3 = time.perf_counter()
    finally:
        dm.set_force_general(False)
    print("%s: call with the re-run %.2f s, forced call %.2f s" % (call, t1 - t0, t3 - t2))
    assert len(got) == 4
    assert got[:3] == short
    assert got[3] == forced[3]
    assert np.isfinite(floats).all()


def test_restricted_vocabulary():
    """set_vocabulary on the handle: the lattice is that of the proto with the
    same types and the load-time scores."""
    mb = _read("test_model.model")
    dm = S.DeviceModel(mb)
    pcs = model_reader.read_pieces(mb)
    keep = [p for i, (p, s, t) in enumerate(pcs) if t == NORMAL and i % 3 == 0]
    dm.set_vocabulary(keep)
    types = dm.piece_types()
    assert int((types == UNUSED).sum()) > 100
    full = R.Model(mb)
    rm = R.Model(vocab_ref.retype(mb, types))
    rm.unk_score, rm.max_score = full.unk_score, full.max_score
    norm = fixture_data("botchan_test_model")[2][:40]
    _check_edges(mb, norm, (THETA,), rm=rm, dm=dm)
    dm.reset_vocabulary()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_shapes(n):
    """A call of the first n sentences gives what they got in the call of
    all (600 sentences: more than two blocks of workspace)."""
    mb, dm, norm = fixture_data("botchan_test_model")
    sents = norm[:600]
    if "shapes" not in _FIX:
        _FIX["shapes"] = (_entropy(dm, sents, with_log_z=True), _score(dm, sents, 2))
    (h, z), (ids, to, sc, lens) = _FIX["shapes"]
    ph, pz = _entropy(dm, sents[:n], with_log_z=True)
    assert np.array_equal(_bits(ph), _bits(h[:n])) and np.array_equal(_bits(pz), _bits(z[:n]))
    assert _rows(*_score(dm, sents[:n], 2)) == _rows(ids, to, sc, lens)[:2 * n]


def test_sample_stream():
    """Sample 0 is SampleEncode's draw; sample j is SampleEncode's draw under
    sample_seed(seed, j); results depend neither on the batch split nor on an
    index_base shift; every score is the restatement's score of its ids."""
    mb, dm, norm = fixture_data("botchan_test_model")
    rm = R.Model(mb)
    sents = norm[:300]
    ns = 4
    rows = _rows(*_score(dm, sents, ns, index_base=11))
    buf, off = S.to_csr(sents)
    for j in range(ns):
        ids, lens, to = dm.sample_encode_csr_host(buf, off, THETA, S.sample_seed(SEED, j), index_base=11,
                                                  with_lens=True)
        for i in range(len(sents)):
            a, b = int(to[i]), int(to[i + 1])
            assert rows[i * ns + j][:2] == (ids[a:b].tolist(), lens[a:b].tolist()), (i, j)
    a = _rows(*_score(dm, sents[:100], ns, index_base=11))
    b = _rows(*_score(dm, sents[100:], ns, index_base=111))
    assert a + b == rows
    assert _rows(*_score(dm, sents, ns, seed=SEED + 1, index_base=11)) != rows
    other = [sents[200]] * 3 + [b"filler"]
    assert _rows(*_score(dm, other, ns, index_base=209))[2 * ns:3 * ns] == rows[200 * ns:201 * ns]
    distinct = 0
    for r, (r_ids, r_lens, r_sc) in enumerate(rows):
        assert L.path_score(rm, sents[r // ns], THETA, r_ids, r_lens).tobytes() == r_sc, r
        distinct += r % ns > 0 and r_ids != rows[r - 1][0]
    assert distinct > len(sents)  # the samples of a sentence are not copies


def _distribution_cases():
    mb = _read("test_model.model")
    pcs = model_reader.read_pieces(mb)
    ud = model(pcs + [("<tag>", 0.0, USER_DEFINED)], UNIGRAM)
    un = model([(p, s, UNUSED if p == "▁the".encode() else t) for p, s, t in pcs], UNIGRAM)
    return [("plain", mb, "▁hello"), ("plain", mb, "▁a▁b"), ("plain", mb, "▁in▁a"), ("unk", mb, "▁a☃b"),
            ("user_defined", ud, "▁a<tag>b"), ("unused", un, "▁the▁a")]


@pytest.mark.parametrize("case", range(6))
def test_frequencies_match_the_scores(case):
    """The six short sentences of test_gpu_sample.py's probability test, 50 000
    draws each (num_samples 500 x 100 calls): every path's frequency lies
    within 5 sqrt(p (1 - p) / N) of p = exp(score), no other path is drawn,
    the drawn paths' scores are the restatement's, and the exp(score) of all
    paths sum to 1 within float error."""
    name, mb, text = _distribution_cases()[case]
    s = text.encode()
    dm, rm = S.DeviceModel(mb), R.Model(mb)
    buf, off = S.to_csr([s])
    calls, ns = 100, 500
    n = calls * ns
    freq, seen_score = {}, {}
    for c in range(calls):
        ids, to, sc, lens = dm.sample_encode_and_score_csr_host(buf, off, ns, THETA, 1000 * case + 5, index_base=c,
                                                                with_lens=True)
        for r_ids, r_lens, r_sc in _rows(ids, to, sc, lens):
            key = (tuple(r_ids), tuple(r_lens))
            freq[key] = freq.get(key, 0) + 1
            seen_score[key] = r_sc
    want = rm.enumerate_paths(s, THETA)
    assert set(freq) <= set(want), name
    total = 0.0
    for path, exact in want.items():
        score = L.path_score(rm, s, THETA, path[0], path[1])
        if path in seen_score:
            assert seen_score[path] == score.tobytes(), (name, path)
        p = math.exp(float(score))
        # (a float score of magnitude below 64 after some ten roundings of half an ulp, 3.8e-6, each)
        assert abs(p - exact) <= 1e-4 * exact, (name, path, p, exact)
        total += p
        f = freq.get(path, 0) / n
        assert abs(f - p) <= 5 * math.sqrt(p * (1 - p) / n), (name, path, f, p)
    # Each score carries a few float roundings on a magnitude of at most ~100.
    assert total <= 1.0 + 1e-4 and total >= 1.0 - 1e-4, (name, total)


def test_capacity_overflow():
    """A token capacity below the need: SPM_RESOURCE_EXHAUSTED with the
    offsets and scores written (their last entry is the need) and no token;
    a second call with that capacity succeeds."""
    mb, dm, norm = fixture_data("botchan_test_model")
    sents = norm[:50]
    buf, off = S.to_csr(sents)
    good = dm.sample_encode_and_score_csr_host(buf, off, 3, THETA, SEED, with_lens=True)
    need = int(good[1][-1])
    with pytest.raises(S.SpmError) as e:
        dm.sample_encode_and_score_csr_host(buf, off, 3, THETA, SEED, with_lens=True, token_capacity=need - 1)
    assert e.value.code == 8
    assert np.array_equal(e.value.tok_offsets, good[1]) and np.array_equal(_bits(e.value.scores), _bits(good[2]))
    again = dm.sample_encode_and_score_csr_host(buf, off, 3, THETA, SEED, with_lens=True, token_capacity=need)
    for a, b in zip(good, again):
        assert np.array_equal(a, b)
    # No sentence at all: one offset, nothing else.
    ids, to, sc = dm.sample_encode_and_score_csr_host(*S.to_csr([]), 3, THETA, SEED)
    assert ids.size == 0 and sc.size == 0 and to.tolist() == [0]
    assert _entropy(dm, []).size == 0


def test_status_codes():
    buf, off = S.to_csr(["▁hello".encode()])
    dm = S.DeviceModel(_read("test_model.model"))
    for theta in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(S.SpmError) as e:
            dm.entropy_csr_host(buf, off, theta)
        assert e.value.code == 3  # SPM_INVALID_ARGUMENT
        with pytest.raises(S.SpmError) as e:
            dm.sample_encode_and_score_csr_host(buf, off, 2, theta, SEED)
        assert e.value.code == 3
    with pytest.raises(S.SpmError) as e:
        dm.sample_encode_and_score_csr_host(buf, off, 0, THETA, SEED)
    assert e.value.code == 3
    for name in ("botchan_bpe1k.model", "botchan_word2000.model", "botchan_char60.model"):
        other = S.DeviceModel(_read(name))
        with pytest.raises(S.SpmError) as e:
            other.entropy_csr_host(buf, off, THETA)
        assert e.value.code == 12, name  # SPM_UNIMPLEMENTED
        with pytest.raises(S.SpmError) as e:
            other.sample_encode_and_score_csr_host(buf, off, 2, THETA, SEED)
        assert e.value.code == 12, name
    host = S.DeviceModel(_read("test_model.model"), host_only=True)
    with pytest.raises(S.SpmError) as e:
        host.entropy_csr_host(buf, off, THETA)
    assert e.value.code == 9  # SPM_FAILED_PRECONDITION
    with pytest.raises(S.SpmError) as e:
        host.sample_encode_and_score_csr_host(buf, off, 2, THETA, SEED)
    assert e.value.code == 9


def test_sample_and_score_device_pointers():
    import torch
    mb, dm, norm = fixture_data("botchan_test_model")
    sents = norm[:120]
    ns = 3
    want = _score(dm, sents, ns, index_base=5)
    buf, off = S.to_csr(sents)
    dev = torch.device("cuda", 0)
    d_b = torch.from_numpy(buf).to(dev)
    d_o = torch.from_numpy(off.view(np.int64)).to(dev)
    cap = ns * int(off[-1])
    rows = ns * len(sents)
    d_ids = torch.empty(cap, dtype=torch.int32, device=dev)
    d_len = torch.empty(cap, dtype=torch.int32, device=dev)
    d_tok = torch.empty(rows + 1, dtype=torch.int64, device=dev)
    d_sc = torch.empty(rows, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    dm.sample_encode_and_score_device(d_b.data_ptr(), d_o.data_ptr(), len(sents), ns, THETA, SEED, d_ids.data_ptr(),
                                      cap, d_tok.data_ptr(), d_sc.data_ptr(), index_base=5, d_len=d_len.data_ptr())
    to = d_tok.cpu().numpy().view(np.uint64)
    k = int(to[-1])
    got = _rows(d_ids.cpu().numpy()[:k], to, d_sc.cpu().numpy(), d_len.cpu().numpy()[:k].view(np.uint32))
    assert got == _rows(*want)


def _selftest(model_name, args):
    p = subprocess.run([os.path.join(LIB, "lattice_score_selftest"), os.path.join(GOLD, model_name)] + args,
                       capture_output=True, timeout=60)
    assert p.returncode == 0, p.stderr
    return [r.split(" ") for r in p.stdout.decode().split("\n") if r]


def test_processor():
    """CalculateEntropy gives the package's recorded floats for three botchan
    lines; SampleEncodeAndScore replays under a seed and advances between
    calls; wor is refused; a BPE model gives the package's INTERNAL texts."""
    lines = O.read_lines_binary(os.path.join(GOLD, "botchan.txt"))
    picks = [3, 10, 42]
    gold = G.read_golden("botchan_test_model")[1]
    rows = _selftest("test_model.model", ["12345", "0.5"] + [lines[i].decode() for i in picks])
    ent = [r for r in rows if r[0] == "entropy"]
    assert len(ent) == 3
    for r, i in zip(ent, picks):
        got = np.array([int(r[1], 16)], dtype=np.uint32).view(np.float32)[0]
        assert rel_dev(got, gold[i]) <= REL_BOUND, (i, got, gold[i])
    assert [r for r in rows if r[0] == "entropy1"][0][1] == ent[0][1]
    ids = [r[1:] for r in rows if r[0] == "ids"]
    assert len(ids) == 9
    first, second, replay = ids[:3], ids[3:6], ids[6:]
    assert first == replay and first != second
    assert len({tuple(r) for r in first}) > 1  # three samples, not three copies
    pieces = [r for r in rows if r[0] == "pieces"]
    assert [r[1] for r in pieces] == [r[0] for r in first]  # the same scores
    assert all(len(p) == len(i) + 1 for p, i in zip(pieces, first))
    assert "".join(pieces[0][2:]).replace("▁", " ").strip() == lines[picks[0]].decode().strip()
    # The processor's samples are the C ABI's at index_base 0.
    dm = S.DeviceModel(_read("test_model.model"))
    norm = dm.normalize([lines[picks[0]]])
    got = _rows(*_score(dm, norm, 3, seed=12345))
    assert [r[0] for r in got] == [[int(x) for x in r[1:]] for r in first]
    assert [np.frombuffer(r[2], np.uint32)[0] for r in got] == [int(r[0], 16) for r in first]
    wor = [r for r in rows if r[0] == "wor"][0]
    assert wor[1] == "12" and "not implemented" in " ".join(wor[2:])
    bpe = _selftest("botchan_bpe1k.model", ["1", "0.5", "hello world"])
    assert " ".join(bpe[0]) == "error CalculateEntropy 13 CalculateEntropy is not available for the current model."
    assert " ".join(bpe[1]) == ("error SampleEncodeAndScore 13 SampleEncodeAndScore is not available for the "
                                "current model.")
