"""CPU: spm_hip_fit_ids_host.  The Python restatement (fit_ref.py) against
answers written out by hand, the host loop bit-equal to the restatement with
the sizing bound on the same inputs, and the argument checks (made before any
HIP call, so they need no GPU)."""
import os
import subprocess

import numpy as np
import pytest

import fit_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = -1
NO = R.NO_PLACE


@pytest.fixture(scope="module")
def S():
    import spm_amd
    if not os.path.exists(spm_amd.LIB_PATH):
        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "sentencepiece-comments_amd")])
    spm_amd.lib()
    return spm_amd


def case(lens):
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens, dtype=np.uint64)
    return np.arange(1, int(off[-1]) + 1, dtype=np.int32), off


# L = 4; sentences [], [1 2], [3], [4 5], [], [6 7 8 9], [10..15], [16].
LENS = [0, 2, 1, 2, 0, 4, 6, 1]
HAND = {
    0: [[1, 2, 3, P], [4, 5, P, P], [6, 7, 8, 9], [10, 11, 12, 13], [16, P, P, P]],
    6: [[1, 2, 3, P], [4, 5, P, P], [6, 7, 8, 9], [10, 13, 14, 15], [16, P, P, P]],  # TRUNCATE_LEFT | KEEP_END
}
HAND_SEQ = [[1, 1, 2, -1], [3, 3, -1, -1], [5, 5, 5, 5], [6, 6, 6, 6], [7, -1, -1, -1]]
HAND_POS = [[0, 1, 0, 0], [0, 1, 0, 0], [0, 1, 2, 3], [0, 1, 2, 3], [0, 0, 0, 0]]
HAND_PLACE = [NO, 0, 2, 4, NO, 8, 12, 16]


@pytest.mark.parametrize("flags", [0, 6])
def test_ref_equals_hand_written_answer(flags):
    out, seq, pos, lengths, place, stats = R.fit_ref(*case(LENS), 4, P, flags)
    assert out.tolist() == HAND[flags] and seq.tolist() == HAND_SEQ and pos.tolist() == HAND_POS
    assert lengths.tolist() == [3, 2, 4, 4, 1] and place.tolist() == HAND_PLACE and stats == (5, 14, 1, 2)


def test_ref_of_nothing():
    assert R.fit_ref(*case([0, 0]), 3, P)[5] == (0, 0, 0, 0)
    assert R.fit_ref(*case([]), 3, P)[0].shape == (0, 3)


def check_host(S, ids, off, L, flags, spare=None):
    want = R.fit_ref(ids, off, L, 7, flags)
    need, n = want[5][0], len(off) - 1
    assert need <= S.fit_rows_bound(int(off[-1]) - int(off[0]), n, L)  # the documented sizing
    cap = None if spare is None else max(need + spare, 0)
    got = S.fit_ids_host(ids, off, L, 7, flags, rows_capacity=cap, fill=-77)
    rows = need if cap is None else min(need, cap)
    for g, w in zip(got[:4], want[:4]):
        assert np.array_equal(g[:rows], w[:rows]) and (g[rows:] == -77).all()
    assert np.array_equal(got[4], want[4]) and tuple(got[5].tolist()) == want[5]


@pytest.mark.parametrize("L", [1, 2, 5, 64, 257])
def test_host_equals_ref(S, L):
    rng = np.random.default_rng(3000 + L)
    for n in (0, 1, 2, 1000):
        ids, off = R.random_csr(rng, R.mixed_lens(rng, n, L), base=n)
        for flags in (0, 2, 4, 6):
            check_host(S, ids, off, L, flags)
    check_host(S, *R.random_csr(rng, np.zeros(50, dtype=np.int64)), L, 0)
    for spare in (-1, 0, 3):
        check_host(S, ids, off, L, 4, spare=spare)


def test_argument_errors(S):
    ids, off = case(LENS)
    for kw in ({"row_len": 0}, {"row_len": 1 << 31}, {"flags": 1}, {"flags": 8}):
        with pytest.raises(S.SpmError) as e:
            S.fit_ids_host(ids, off, **{"row_len": 4, "pad_id": P, **kw})
        assert e.value.code == S.SPM_INVALID_ARGUMENT
    L = S.lib()
    out, stats = np.zeros(8, np.int32), np.zeros(4, np.uint64)
    p = lambda a: a.ctypes.data  # noqa: E731
    bad = S.SPM_INVALID_ARGUMENT
    assert L.spm_hip_fit_ids_host(p(ids), p(off), 8, 4, P, 0, 2, None, None, None, None, None, p(stats)) == bad
    assert L.spm_hip_fit_ids_host(p(ids), None, 8, 4, P, 0, 2, p(out), None, None, None, None, None) == bad
    assert L.spm_hip_fit_ids_host(p(ids), p(off), 1 << 31, 4, P, 0, 2, p(out), None, None, None, None, None) == bad
    # The device entry checks before it enqueues: no scratch, too little scratch.
    need = S.fit_ids_scratch_bytes(8, 4, 2)
    assert need > 0 and need % 16 == 0 and S.fit_ids_scratch_bytes(0, 4, 2) == 0
    assert L.spm_hip_fit_ids(16, 16, 8, 4, P, 0, 2, 16, None, None, None, None, None, None, need, None) == bad
    assert L.spm_hip_fit_ids(16, 16, 8, 4, P, 0, 2, 16, None, None, None, None, None, 16, need - 1, None) == bad
    assert L.spm_hip_fit_ids(16, 16, 8, 4, P, 1, 2, 16, None, None, None, None, None, 16, need, None) == bad
