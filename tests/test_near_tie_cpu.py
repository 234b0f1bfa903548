"""The byte kernel's near-tie predicate (device_common.h NearTieAt with
TieBound) flags a superset of NearTie's and NearTieHi's pairs.

float32 numpy restatements of the three device predicates.  A setter of the
forward pass is hi = fl(t0 + s), t0 the begin position's best score and s a
node score with |s| <= mag (spm_hip_api.cc: tie_mag bounds every node score,
the UNK and the USER_DEFINED ones included); lo is the end position's score so
far.  NearTieAt's bound depends on t0 only, so pairs are drawn as (t0, s, lo).
"""
import os

import numpy as np

import model_reader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
E21, E20 = f32(2.0 ** -21), f32(2.0 ** -20)


def near_tie(lo, hi, mag):
    m = (np.maximum(np.abs(lo), np.abs(hi)) + mag).astype(f32)
    return (hi - lo).astype(f32) <= (m * E21).astype(f32)


def near_tie_hi(lo, hi, mag):
    return (hi - lo).astype(f32) <= ((np.abs(hi) + mag).astype(f32) * E20).astype(f32)


def tie_bound(t0, mag):
    return (((np.abs(t0) + mag).astype(f32) + mag).astype(f32) * E20).astype(f32)


def near_tie_at(lo, hi, bound):
    return (hi - lo).astype(f32) <= bound


def _model_mags():
    """tie_mag as the model loader computes it, for the models that ship."""
    mags = []
    for d, names in (("data", ["synth32k_unigram.model"]),
                     ("tests/golden", ["test_model.model", "test_ja_model.model"])):
        for n in names:
            pcs = model_reader.read_pieces(open(os.path.join(ROOT, d, n), "rb").read())
            sc = np.array([s for _, s, t in pcs if t == 1], dtype=f32)
            chars = max(len(p.decode("utf-8", "replace")) for p, _, t in pcs if t != 5)
            mag = max(float(np.abs(sc).max()), abs(float(sc.min()) - 10.0), abs(chars * float(sc.max())) + 1.0)
            mags.append(f32(mag) + f32(1.0))
    return mags


def _step(x, k):
    """x moved by k float32 ulps (k an int array, either sign)."""
    b = x.view(np.int32).astype(np.int64)
    b = np.where(b < 0, np.int64(-2 ** 31) - b, b) + k  # sign-magnitude -> ordered
    b = np.where(b < 0, np.int64(-2 ** 31) - b, b)
    return b.astype(np.int32).view(f32)


def _pairs(mag, rng, n):
    """(t0, s, lo) float32 arrays: random and adversarial."""
    t0 = -(rng.random(n) * rng.choice([1.0, 10.0, 100.0, 5000.0], n)).astype(f32)
    s = ((rng.random(n) * 2 - 1) * float(mag)).astype(f32)
    q = n // 8
    # zeros, powers of two (hi lands on or next to a binade edge), |s| = mag
    t0[:q] = 0.0
    s[q:2 * q] = np.where(rng.random(q) < 0.5, mag, -mag).astype(f32)
    t0[2 * q:3 * q] = -(2.0 ** rng.integers(-3, 13, q)).astype(f32)
    s[2 * q:3 * q] = _step(np.zeros(q, dtype=f32), rng.integers(-4, 5, q))
    s[3 * q:4 * q] = 0.0
    with np.errstate(all="ignore"):
        hi = (t0 + s).astype(f32)
        # lo: 0..8 ulps below hi (equal exponents, or across a power of two
        # where hi sits on an edge), further random distances, and above hi
        lo = _step(hi, -rng.integers(0, 9, n))
        far = rng.random(n) < 0.3
        lo = np.where(far, (hi - np.abs(hi + mag) * (2.0 ** -rng.uniform(14, 26, n))).astype(f32), lo)
        lo[-q:] = _step(hi[-q:], rng.integers(1, 4, q))
    return t0, s, hi, lo


def test_near_tie_at_is_a_superset():
    rng = np.random.default_rng(11)
    mags = _model_mags() + [f32(1.0), f32(2.0), f32(27.0), f32(100.0), f32(10000.0)]
    total = flagged_old = 0
    for mag in mags:
        t0, s, hi, lo = _pairs(mag, rng, 400000)
        assert np.all(np.abs(s) <= mag)
        with np.errstate(all="ignore"):
            old = near_tie(lo, hi, mag)
            old_hi = near_tie_hi(lo, hi, mag)
            new = near_tie_at(lo, hi, tie_bound(t0, mag))
        assert not np.any(old & ~old_hi), "NearTieHi misses a NearTie pair"
        assert not np.any(old_hi & ~new), "NearTieAt misses a NearTieHi pair"
        total += len(lo)
        flagged_old += int(old.sum())
    assert total >= 3_000_000 and flagged_old > total // 10  # the adversarial pairs are near


def test_near_tie_at_false_for_an_empty_slot():
    rng = np.random.default_rng(12)
    for mag in _model_mags() + [f32(1.0), f32(10000.0)]:
        t0, s, hi, _ = _pairs(mag, rng, 100000)
        lo = np.full_like(hi, -np.inf)
        with np.errstate(all="ignore"):
            assert not np.any(near_tie_at(lo, hi, tie_bound(t0, mag)))
            # and for a NaN setter (a position without a node)
            assert not np.any(near_tie_at(hi, np.full_like(hi, np.nan), tie_bound(t0, mag)))
