"""CPU: spm_hip_window_ids_host.  The Python restatement (window_ref.py)
against answers written out by hand, the host loop bit-equal to the
restatement with the sizing bound on the same inputs, the fresh-slot invariant
and the argument checks (made before any HIP call, so they need no GPU)."""
import numpy as np
import pytest

import window_ref as R
from test_fit_cpu import S  # noqa: F401  (the fixture: spm_amd with the library built and loaded)

P = -1
SHAPES = [(1, 0, 0), (3, 0, 3), (4, 1, 0), (4, 3, 0), (5, 1, 3), (8, 0, 1), (17, 5, 2), (257, 64, 3)]

# One sentence of ids 1..len: (L, S, flags) -> {len: (out, fresh)}.
HAND = {
    (4, 1, 0): {
        0: ([[P, P, P, P]], [[0, 0, 0, 0]]),
        1: ([[1, P, P, P]], [[1, 0, 0, 0]]),
        4: ([[1, 2, 3, 4]], [[1, 1, 1, 1]]),
        5: ([[1, 2, 3, 4], [4, 5, P, P]], [[1, 1, 1, 1], [0, 1, 0, 0]]),
        7: ([[1, 2, 3, 4], [4, 5, 6, 7]], [[1, 1, 1, 1], [0, 1, 1, 1]]),
        8: ([[1, 2, 3, 4], [4, 5, 6, 7], [7, 8, P, P]], [[1, 1, 1, 1], [0, 1, 1, 1], [0, 1, 0, 0]]),
    },
    (5, 1, 3): {
        1: ([[1, P, P, P, P]], [[1, 0, 0, 0, 0]]),
        2: ([[1, 2, P, P, P]], [[1, 1, 0, 0, 0]]),
        3: ([[1, 2, 3, P, P]], [[1, 1, 1, 0, 0]]),
        5: ([[1, 2, 3, 4, 5]], [[1, 1, 1, 1, 1]]),
        6: ([[1, 2, 3, 4, 6], [1, 4, 5, 6, P]], [[1, 1, 1, 1, 1], [0, 0, 1, 0, 0]]),
        9: ([[1, 2, 3, 4, 9], [1, 4, 5, 6, 9], [1, 6, 7, 8, 9]],
            [[1, 1, 1, 1, 1], [0, 0, 1, 1, 0], [0, 0, 1, 1, 0]]),
    },
}


@pytest.mark.parametrize("shape", sorted(HAND))
def test_ref_equals_hand_written_answer(shape):
    L, stride, flags = shape
    for n, (w_out, w_fresh) in HAND[shape].items():
        out, pos, fresh, lengths, row_sentence, first_row, stats = R.window_ref(
            np.arange(1, n + 1), [0, n], L, stride, P, flags)
        assert out.tolist() == w_out and fresh.tolist() == w_fresh, n
        assert pos.tolist() == [[max(v - 1, 0) for v in row] for row in w_out], n
        assert lengths.tolist() == [sum(v != P for v in row) for row in w_out], n
        assert first_row.tolist() == [0, len(w_out)] and stats == (len(w_out), int(len(w_out) > 1)), n


def check_host(S, ids, off, L, stride, flags, spare=None):
    want = R.window_ref(ids, off, L, stride, 7, flags)
    need, n = want[6][0], len(off) - 1
    assert need <= S.window_rows_bound(int(off[-1]) - int(off[0]), n, L, stride, flags & 1, flags & 2)
    cap = None if spare is None else max(need + spare, 0)
    got = S.window_ids_host(ids, off, L, stride, 7, flags, rows_capacity=cap, fill=-77)
    rows = need if cap is None else min(need, cap)
    for g, w in zip(got[:5], want[:5]):
        assert np.array_equal(g[:rows], w[:rows]) and (g[rows:] == np.array(-77).astype(g.dtype)).all()
    assert np.array_equal(got[5], want[5]) and tuple(got[6].tolist()) == want[6]
    return want


@pytest.mark.parametrize("L,stride,flags", SHAPES)
def test_host_equals_ref_and_fresh_covers_every_token_once(S, L, stride, flags):
    rng = np.random.default_rng(5000 + L)
    lens = R.edge_lens(L, stride, flags)
    ids, off = R.random_csr(rng, lens + [int(x) for x in rng.integers(0, 4 * L + 2, size=40)], base=3)
    out, pos, fresh, _, row_sentence, first_row, _ = check_host(S, ids, off, L, stride, flags)
    for i in range(len(off) - 1):
        rows = slice(int(first_row[i]), int(first_row[i + 1]))
        assert (row_sentence[rows] == i).all()
        assert sorted(pos[rows][fresh[rows] == 1].tolist()) == list(range(int(off[i + 1] - off[i])))
    for spare in (-1, 0, 3):
        check_host(S, ids, off, L, stride, flags, spare=spare)
    check_host(S, *R.random_csr(rng, []), L, stride, flags)


def test_argument_errors(S):
    ids, off = np.arange(1, 10, dtype=np.int32), np.array([0, 9], dtype=np.uint64)
    L = S.lib()
    out = np.zeros(64, np.int32)
    p = lambda a: a.ctypes.data  # noqa: E731
    bad, nil = S.SPM_INVALID_ARGUMENT, (None,) * 6

    def host(row_len=4, stride=1, flags=0, n=1, o=p(out), offsets=p(off)):
        return L.spm_hip_window_ids_host(p(ids), offsets, n, row_len, stride, P, flags, 4, o, *nil)
    assert host() == S.SPM_OK
    for kw in ({"row_len": 0}, {"row_len": 1 << 31}, {"flags": 4}, {"o": None}, {"offsets": None},
               {"stride": 4}, {"row_len": 2, "stride": 0, "flags": 3}, {"row_len": 3, "stride": 1, "flags": 3}):
        assert host(**kw) == bad, kw
    assert host(n=1 << 31) == S.SPM_OUT_OF_RANGE
    # The device entry checks before it enqueues: no scratch, too little scratch.
    need = S.window_ids_scratch_bytes(1)
    assert need > 0 and need % 16 == 0 and S.window_ids_scratch_bytes(0) == 0
    dev = lambda scratch, nbytes, stride=1: L.spm_hip_window_ids(  # noqa: E731
        16, 16, 1, 4, stride, P, 0, 4, 16, *nil, scratch, nbytes, None)
    assert dev(None, need) == bad and dev(16, need - 1) == bad and dev(24, need) == bad and dev(16, need, 4) == bad
