"""CPU: the BPE-dropout restatement (bpe_dropout_ref.py) against the
`sentencepiece` package's recorded draw counts and against its own fixed
points, and the host's integer threshold against the draw comparison.

The recorded counts (tests/golden/bpe_dropout_counts.json.gz, made once by
tools/make_bpe_dropout_golden.py) are 200 000 package draws per input and
alpha.  The restatement's exact path probabilities must explain them: every
observed segmentation is one the keep / drop tree reaches, and each bin with
N * p >= 25, and the pooled rest, lies within 5 sigma of N * p (binomial
sigma).  5 sigma: an unreduced check of the same kind reached 3.96 sigma over
about 1 500 bins, and the fixture is fixed once recorded."""
import gzip
import json
import math
import os
import random

import numpy as np
import pytest

import bpe_cases as C
import bpe_dropout_ref as R
import oracle_lib as O
import sample_ref
import spm_amd as S

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HAND_KW = {"hand:unused": dict(unused=True), "hand:user_defined": dict(user_defined=True)}


def _blob(key):
    if key.startswith("hand:"):
        return C.build_model(**HAND_KW[key]).blob
    with open(os.path.join(GOLD, key), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def recorded():
    with gzip.open(os.path.join(GOLD, "bpe_dropout_counts.json.gz"), "rb") as f:
        return json.loads(f.read().decode())["cases"]


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(key):
        if key not in cache:
            cache[key] = R.Model(_blob(key))
        return cache[key]

    return get


def length_view(model, probs):
    """Path probabilities keyed as the fixture keys them: the pieces' byte
    lengths with runs of unknown tokens merged."""
    out = {}
    for (ids, lens), p in probs.items():
        key = tuple(R.merge_unknown_runs(ids, lens, model.unk_id)[1])
        out[key] = out.get(key, 0.0) + p
    return out


def test_fixture_covers_what_it_should(recorded):
    keys = {c["model"] for c in recorded}
    assert {"botchan_bpe1k.model", "botchan_bf_bpe1k.model"} <= keys
    for k in ("botchan_bpe1k.model", "botchan_bf_bpe1k.model"):
        texts = {c["text"] for c in recorded if c["model"] == k}
        assert len(texts) >= 12 and {"the teacher", "zzz qqq", "I am 日本"} <= texts
        assert {c["alpha"] for c in recorded if c["model"] == k} == {0.1, 0.5}
    assert all(c["draws"] == 200000 and sum(v for _, v in c["counts"]) == c["draws"] for c in recorded)


def test_restatement_explains_the_package_counts(recorded, models):
    worst = (0.0, None)
    bins = 0
    for case in recorded:
        m = models(case["model"])
        probs = length_view(m, R.path_probabilities(m, case["norm"].encode(), case["alpha"]))
        assert abs(sum(probs.values()) - 1.0) < 1e-9
        counts = {tuple(k): v for k, v in case["counts"]}
        unseen = [k for k in counts if k not in probs]
        assert not unseen, "%s %r alpha %s: the package drew %r, which the tree never reaches" % (
            case["model"], case["text"], case["alpha"], unseen[0])
        dev = R.binned_deviation(probs, counts, case["draws"])
        bins += sum(case["draws"] * p >= 25 for p in probs.values())
        if dev > worst[0]:
            worst = (dev, (case["model"], case["text"], case["alpha"]))
    print("worst deviation %.2f sigma at %r over %d bins" % (worst[0], worst[1], bins))
    assert worst[0] <= 5.0, worst


def _oracle_rows(blob, sents):
    buf, off = O.to_csr(sents)
    ids, lens, to = O.OracleModel(blob).encode_normalized_csr(buf, off, with_lens=True)
    return [(list(map(int, ids[int(to[k]):int(to[k + 1])])), list(map(int, lens[int(to[k]):int(to[k + 1])])))
            for k in range(len(sents))]


def test_alpha_zero_is_encode_and_alpha_one_the_initial_split():
    blob = _blob("botchan_bpe1k.model")
    om = O.OracleModel(blob)
    norm = om.normalize(O.read_lines_binary(os.path.join(GOLD, "botchan.txt"))[:600])
    cases = [(blob, norm)]
    for kw in (dict(), dict(ties=True), dict(unused=True), dict(irregular=True), dict(user_defined=True)):
        cases.append((C.build_model(**kw).blob, C.pool()))
    for blob, sents in cases:
        m = R.Model(blob)
        for k, (s, want) in enumerate(zip(sents, _oracle_rows(blob, sents))):
            assert R.encode(m, s, 0.0, 7, k) == want, s
            if not m.user:
                ids, lens = R.encode(m, s, 1.0, 7, k)
                starts = C.walk_starts(s)
                assert lens == [b - a for a, b in zip(starts, starts[1:] + [len(s)])], s
                assert ids == [m.piece_to_id(s[a:a + n]) for a, n in zip(starts, lens)]


def test_host_threshold_is_the_draw_comparison():
    rng = random.Random(5)
    alphas = [0.0, 1.0, 1e-9, 1.0 - 2.0 ** -24, 0.1, 0.5, 2.0 ** -53, 2.0 ** -60, -0.5, 1.5, float("inf"),
              float("-inf")] + [rng.random() for _ in range(20)]
    for alpha in alphas:
        a = float(np.float32(alpha))
        t = S.bpe_dropout_threshold(alpha)
        assert 0 <= t <= 1 << 53
        assert t == (0 if a <= 0 else 1 << 53 if a >= 1 else math.ceil(a * 2.0 ** 53))
        for _ in range(2000):
            key, k = rng.getrandbits(64), (rng.getrandbits(11) << 32) | rng.getrandbits(11)
            bits = sample_ref.mix(key + sample_ref.GOLDEN * (k + 1)) >> 11
            assert (bits < t) == (sample_ref.draw_u(key, k) < a)
        # Around the threshold itself.
        for bits in (t - 1, t, t + 1):
            if 0 <= bits < 1 << 53:
                assert (bits < t) == (bits * 2.0 ** -53 < a)
    with pytest.raises(Exception):
        S.bpe_dropout_threshold(float("nan"))
    # The C entry's draw is the restatement's.
    for _ in range(50):
        seed, g, k = rng.getrandbits(64), rng.getrandbits(40), (rng.getrandbits(10) << 32) | rng.getrandbits(10)
        assert S.sample_uniform(seed, g, k) == sample_ref.uniform(seed, g, k)
