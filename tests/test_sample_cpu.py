"""CPU: the sampler's random stream over the C ABI, the Python restatement
(tests/sample_ref.py) against the reference's LatticeTest.SampleTest, and
the argument checks of spm_hip_sample_encode_batch_host — no GPU calls."""
import math
import os
import subprocess

import numpy as np
import pytest

import sample_ref as R
from sample_ref import ABC_THETAS, abc_expected, abc_model, abc_name

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def S():
    import spm_amd
    if not os.path.exists(spm_amd.LIB_PATH):
        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "sentencepiece-comments_amd")])
    spm_amd.lib()
    return spm_amd


def test_uniform_matches_python_stream(S):
    top = (1 << 64) - 1
    grid = [0, 1, 2, 63, 0x9E3779B97F4A7C15, 1 << 32, (1 << 63) + 5, top - 1, top]
    for seed in grid:
        for index in grid:
            for draw in (0, 1, 7, 1 << 40, top):
                u = S.sample_uniform(seed, index, draw)
                assert u == R.uniform(seed, index, draw), (seed, index, draw)
                assert 0.0 <= u < 1.0


def test_uniform_is_uniform():
    # Mean and a 16-bin histogram of 64 000 draws (binomial sd of a bin: 0.00096).
    us = np.array([R.uniform(12345, g, k) for g in range(8000) for k in range(8)])
    assert abs(us.mean() - 0.5) < 5 * math.sqrt(1 / 12 / us.size)
    hist = np.histogram(us, bins=16, range=(0, 1))[0] / us.size
    assert np.abs(hist - 1 / 16).max() < 5 * math.sqrt((1 / 16) * (15 / 16) / us.size)


def test_enumeration_reproduces_reference_probabilities():
    m = R.Model(abc_model())
    for theta in ABC_THETAS:
        got = {abc_name(ids): p for (ids, _), p in m.enumerate_paths(b"ABC", theta).items()}
        want = abc_expected(theta)
        assert set(got) == set(want)
        # The model file holds float scores: each is off its decimal by at
        # most 2^-24 relative (< 1.1e-7 absolute here), a path's sum of three
        # by < 3.3e-7, and with theta <= 1 a probability by less than twice
        # that, relative.
        for k in want:
            assert abs(got[k] - want[k]) < 1e-6, (theta, k)


def test_restatement_samples_the_reference_distribution():
    m = R.Model(abc_model())
    trials = 100000
    for t, theta in enumerate(ABC_THETAS):
        prep = m.prepare(b"ABC", theta)
        freq = {}
        for g in range(trials):
            ids, lens, _ = m.draw(prep, R.sentence_key(1000 + t, g))
            assert sum(lens) == 3
            k = abc_name(ids)
            freq[k] = freq.get(k, 0) + 1
        want = abc_expected(theta)
        assert set(freq) == set(want)
        for k in want:
            assert abs(freq[k] / trials - want[k]) < 0.02, (theta, k, freq[k] / trials, want[k])


def test_is_path_and_margin():
    m = R.Model(abc_model())
    ids, lens, margin = m.sample(b"ABC", 0.5, 3, 0)
    assert m.is_path(b"ABC", ids, lens)
    assert not m.is_path(b"ABC", ids, [ln + 1 for ln in lens])
    assert not m.is_path(b"ABC", [0] + ids[1:], lens) or ids[0] == 0
    assert margin > 0
    assert m.sample(b"", 0.5, 3, 0) == ([], [], math.inf)


def test_host_only_handle_and_theta_checks(S):
    mb = open(os.path.join(GOLD, "test_model.model"), "rb").read()
    d = S.DeviceModel(mb, host_only=True)
    buf, off = S.to_csr([b"\xe2\x96\x81hello"])
    with pytest.raises(S.SpmError) as e:
        d.sample_encode_csr_host(buf, off, 0.5, 1)
    assert e.value.code == 9  # SPM_FAILED_PRECONDITION
    # The argument check comes before the handle's: a non-finite theta is
    # SPM_INVALID_ARGUMENT on any handle.
    for theta in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(S.SpmError) as e:
            d.sample_encode_csr_host(buf, off, theta, 1)
        assert e.value.code == 3
