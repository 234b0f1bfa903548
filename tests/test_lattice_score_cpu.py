"""CPU: the lattice scores' restatement (lattice_score_ref.py) against the
`sentencepiece` package and its recorded answers (tests/golden/*.entropy.gz,
tools/make_lattice_score_golden.py)."""
import math
import os

import numpy as np
import pytest
import sentencepiece

import lattice_score_ref as L
import make_lattice_score_golden as G
import sample_ref as R

GOLD = G.GOLD
F32 = np.float32

# The restatement takes exp in double and rounds it, the package takes exp in
# float.  Worst relative deviation of the restatement from the package over
# every line of the three fixtures at alpha 0, 0.5 and 1, measured with this
# test (it prints the figure of each fixture and alpha): 5.15e-7, on
# wagahaiwa at alpha 0.5, written here as 5.2e-7.  Every bound below, and the device tests', is 16
# times that: the device's fp64 exp / log are another libm, and one ulp
# there moves the float result the same way.
WORST_MEASURED = 5.2e-7
REL_BOUND = 16 * WORST_MEASURED
MAX_DIFFERING = 0.01  # share of lines whose bits may differ, per (model, alpha)


def rel_dev(a, b):
    """|a - b| / |b| elementwise (0 where both are equal, zeros included)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.abs(a - b)
    return np.where(d == 0, 0.0, d / np.maximum(np.abs(b), np.finfo(np.float32).tiny))


_CACHE = {}


def fixture_data(name):
    """(package processor, restatement model, normalized lines, lattices) of a
    golden fixture, computed once."""
    if name not in _CACHE:
        _, corpus, model_name = [f for f in G.FIXTURES if f[0] == name][0]
        mbytes = open(os.path.join(GOLD, model_name), "rb").read()
        sp = sentencepiece.SentencePieceProcessor(model_proto=mbytes)
        rm = R.Model(mbytes)
        norm = [sp.normalize(l.decode()).encode() for l in G.corpus_lines(corpus)]
        lats = [rm.lattice(s) if s else None for s in norm]
        _CACHE[name] = (sp, rm, norm, lats)
    return _CACHE[name]


@pytest.mark.parametrize("name", [f[0] for f in G.FIXTURES])
def test_goldens_equal_a_fresh_package_run(name):
    _, corpus, model_name = [f for f in G.FIXTURES if f[0] == name][0]
    lines = G.corpus_lines(corpus)
    gold = G.read_golden(name)
    assert gold.shape == (len(G.ALPHAS), len(lines))
    step = 1 if name != "wagahaiwa_test_ja_model" else 3
    fresh = G.package_entropies(model_name, corpus, lines=lines[::step])
    assert np.array_equal(fresh.view(np.uint32), gold[:, ::step].view(np.uint32))
    assert float(gold.max()) > 10.0  # not vacuous


@pytest.mark.parametrize("alpha_index", range(len(G.ALPHAS)))
@pytest.mark.parametrize("name", [f[0] for f in G.FIXTURES])
def test_restatement_equals_the_package(name, alpha_index):
    sp, rm, norm, lats = fixture_data(name)
    alpha = G.ALPHAS[alpha_index]
    gold = G.read_golden(name)[alpha_index]
    got = np.array([L.entropy(rm, s, alpha, lat=lat) for s, lat in zip(norm, lats)], dtype=np.float32)
    differ = int((got.view(np.uint32) != gold.view(np.uint32)).sum())
    worst = float(rel_dev(got, gold).max())
    print("%s alpha %.1f: %d of %d lines differ, worst relative deviation %.3g" % (name, alpha, differ, len(norm), worst))
    assert differ <= MAX_DIFFERING * len(norm)
    assert worst <= REL_BOUND


@pytest.mark.parametrize("name", ["botchan_test_model", "wagahaiwa_test_ja_model"])
def test_alpha_zero_is_the_log_of_the_path_count(name):
    """At alpha 0 every segmentation is equally likely, so the entropy is
    ln(number of segmentations), an integer count that owes nothing to the
    package, and H[p] = A[p] = ln(paths to p) at every position.

    Bound, worst case to first order, with u = 2^-24, M = max(1, ln paths),
    N nodes and nc positions, k_p nodes ending at p.  A[p] folds k_p terms,
    each fold rounding twice on a magnitude of at most M, and LogSumExp does
    not amplify its inputs' errors, so A[len] is within 2 N u M of the truth.
    If H[b] = A[b] + e_b at the begins, then H[p] = A[p] sum(w) + sum(w e_b)
    with w = exp(lp): sum(w) misses 1 by at most (k_p + 3) u M (the folds'
    roundings, the two roundings of every lp, the weights' own), which A[p]
    <= M multiplies, and the k_p accumulation steps round three times each on
    at most M.  Summed over the positions:
      |H[len] - ln paths| <= u M (M (N + 3 nc) + 5 N).
    exp turns an absolute error of lp into a relative error of a weight that
    multiplies H[b], hence the M squared: the bound says little for the long
    Japanese lines (ln paths of several hundred) and is sharp for the others,
    so the test also asks that it is below 1 % of ln paths on most lines."""
    sp, rm, norm, lats = fixture_data(name)
    step = 7
    checked = sharp = 0
    worst = 0.0
    for s, lat in list(zip(norm, lats))[::step]:
        if not s:
            continue
        paths = L.count_paths(rm, s, lat=lat)
        want = math.log(paths)
        nodes = sum(len(x) for x in lat.end_nodes)
        got = float(L.entropy(rm, s, 0.0, lat=lat))
        M = max(1.0, want)
        bound = 2.0 ** -24 * M * (M * (nodes + 3 * lat.nc) + 5 * nodes)
        assert abs(got - want) <= bound, (s, got, want, bound)
        assert abs(L.entropy_exact(rm, s, 0.0)[0] - want) <= 1e-9 * M
        checked += 1
        sharp += bound <= 0.01 * M
        worst = max(worst, abs(got - want) / M)
    print("%s: %d lines, bound below 1 %% on %d, worst deviation %.3g of ln paths" % (name, checked, sharp, worst))
    assert checked > 100 and sharp >= (0.9 * checked if name == "botchan_test_model" else 10)


@pytest.mark.parametrize("name,count", [("botchan_test_model", 200), ("wagahaiwa_test_ja_model", 100)])
def test_score_of_the_packages_samples(name, count):
    """The package's score of a drawn path is fl(T - A[len]) with T the float
    sum, first node to last, of fl(alpha * score): equal in bits on at least
    99 % of the samples, the rest within the bound."""
    sp, rm, norm, lats = fixture_data(name)
    _, corpus, _ = [f for f in G.FIXTURES if f[0] == name][0]
    lines = G.corpus_lines(corpus)
    alpha = 0.5
    total = differ = 0
    for i in range(len(lines)):
        if total >= 4 * count:
            break
        if not norm[i]:
            continue
        rows = sp.sample_encode_and_score(lines[i].decode(), num_samples=4, alpha=alpha, wor=False,
                                          include_best=False, out_type=int)
        assert len(rows) == 4
        for ids, score in rows:
            want = L.path_score(rm, norm[i], alpha, ids)
            assert want is not None, (i, ids)
            total += 1
            if F32(score).tobytes() != want.tobytes():
                differ += 1
                assert rel_dev(want, F32(score)) <= REL_BOUND, (i, score, want)
    print("%s: %d of %d sample scores differ in bits" % (name, differ, total))
    assert total == 4 * count and differ <= MAX_DIFFERING * total


def test_the_packages_edges():
    """-0.0 for an empty text; the package draws nothing from an empty text
    (the C ABI answers zero-token samples of score 0 there, the processor
    repeats the package's error); the errors of a BPE model."""
    sp, rm, norm, lats = fixture_data("botchan_test_model")
    for text in ("", " "):
        h = F32(sp.calculate_entropy(text, 0.5))
        assert h.tobytes() == F32(-0.0).tobytes() == L.entropy(rm, b"", 0.5).tobytes()
    with pytest.raises(RuntimeError) as e:
        sp.sample_encode_and_score("", num_samples=2, alpha=0.5, wor=False, include_best=False)
    assert "SampleEncodeAndScore returns empty result." in str(e.value)
    assert L.path_score(rm, b"", 0.5, []) == 0.0
    bpe = sentencepiece.SentencePieceProcessor(model_file=os.path.join(GOLD, "botchan_bpe1k.model"))
    with pytest.raises(RuntimeError) as e:
        bpe.calculate_entropy("hello", 0.5)
    assert "INTERNAL" in str(e.value) and "CalculateEntropy is not available for the current model." in str(e.value)
    with pytest.raises(RuntimeError) as e:
        bpe.sample_encode_and_score("hello", num_samples=2, alpha=0.5, wor=False, include_best=False)
    assert "INTERNAL" in str(e.value)
    assert "SampleEncodeAndScore is not available for the current model." in str(e.value)


def test_sample_keys():
    """Sample 0 keeps SampleEncode's key; the others differ from it and from
    each other; the library's host entry agrees."""
    import spm_amd as S
    seed, g = 20240611, 12345
    keys = [L.sample_key(seed, g, j) for j in range(16)]
    assert keys[0] == R.sentence_key(seed, g) and len(set(keys)) == 16
    for j in (0, 1, 2, 15, 1 << 40):
        assert S.sample_seed(seed, j) == L.sample_seed(seed, j)
        assert S.sample_uniform(S.sample_seed(seed, j), g, 3) == R.draw_u(L.sample_key(seed, g, j), 3)
