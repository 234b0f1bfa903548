"""CPU: dense id batches.  The numpy restatement (dense_ref.py) against answers
written out by hand, spm_hip_pad_ids_host / spm_hip_pack_ids_host bit-equal to
the restatement, and the argument checks of all four entry points (made before
any HIP call, so they need no GPU)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import dense_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = -1  # pad id of the literals


@pytest.fixture(scope="module")
def S():
    import spm_amd
    if not os.path.exists(spm_amd.LIB_PATH):
        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "sentencepiece-comments_amd")])
    spm_amd.lib()
    return spm_amd


def case(lens, base=0):
    """Sentences of the given lengths over the ids 1, 2, 3, ...; `base` unused ids in front."""
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens, dtype=np.uint64)
    total = int(off[-1])
    ids = np.concatenate([np.full(base, 99999, dtype=np.int32), np.arange(1, total + 1, dtype=np.int32)])
    return ids, off + np.uint64(base)


LENS = [0, 1, 3, 4, 5, 9]  # sentences [], [1], [2 3 4], [5..8], [9..13], [14..22]
# L = 4.  The four sentences that fit, padded on the right and on the left.
FIT_RIGHT = [[P, P, P, P], [1, P, P, P], [2, 3, 4, P], [5, 6, 7, 8]]
FIT_LEFT = [[P, P, P, P], [P, P, P, 1], [P, 2, 3, 4], [5, 6, 7, 8]]
# The two that are cut, by TRUNCATE_LEFT (2) and KEEP_END (4).
CUT = {
    0: [[9, 10, 11, 12], [14, 15, 16, 17]],
    2: [[10, 11, 12, 13], [19, 20, 21, 22]],
    4: [[9, 10, 11, 13], [14, 15, 16, 22]],
    6: [[9, 11, 12, 13], [14, 20, 21, 22]],
}
MASK_RIGHT = [[0, 0, 0, 0], [1, 0, 0, 0], [1, 1, 1, 0], [1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1]]
MASK_LEFT = [[0, 0, 0, 0], [0, 0, 0, 1], [0, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1]]
# L = 1: one token per sentence.
ONE = {
    0: [P, 1, 2, 5, 9, 14],
    2: [P, 1, 4, 8, 13, 22],
    4: [P, 1, 4, 8, 13, 22],   # cut on the right, the slot keeps the last token
    6: [P, 1, 2, 5, 9, 14],    # cut on the left, the slot keeps the first token
}
PACK_LENS = [3, 0, 6, 1]  # [1 2 3], [], [4..9], [10] at L = 4
PACK_OUT = [[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, P, P]]
PACK_SEQ = [[0, 0, 0, 2], [2, 2, 2, 2], [2, 3, -1, -1]]
PACK_POS = [[0, 1, 2, 0], [1, 2, 3, 4], [5, 0, 0, 0]]


def literal_pad(flags):
    return (FIT_LEFT if flags & 1 else FIT_RIGHT) + CUT[flags & 6], MASK_LEFT if flags & 1 else MASK_RIGHT


@pytest.mark.parametrize("flags", range(8))
def test_pad_ref_literals(flags):
    ids, off = case(LENS)
    out, lengths, mask, stats = R.pad_ref(ids, off, 4, P, flags)
    want, want_mask = literal_pad(flags)
    assert out.tolist() == want
    assert mask.tolist() == want_mask
    assert lengths.tolist() == [0, 1, 3, 4, 4, 4]
    assert stats == (2, 6)


@pytest.mark.parametrize("flags", [0, 2, 4, 6, 1, 5])
def test_pad_ref_row_len_one(flags):
    ids, off = case(LENS)
    out, lengths, mask, stats = R.pad_ref(ids, off, 1, P, flags)
    assert out[:, 0].tolist() == ONE[flags & 6]  # one column: PAD_LEFT changes nothing
    assert lengths.tolist() == [0, 1, 1, 1, 1, 1] and mask[:, 0].tolist() == [0, 1, 1, 1, 1, 1]
    assert stats == (4, 2 + 3 + 4 + 8)


def test_pack_ref_literal():
    ids, off = case(PACK_LENS)
    out, seq, pos, stats = R.pack_ref(ids, off, 4, P)
    assert (out.tolist(), seq.tolist(), pos.tolist(), stats) == (PACK_OUT, PACK_SEQ, PACK_POS, (3, 10))


def check_pad(S, ids, off, L, pad_id, flags):
    out, lengths, mask, stats = S.pad_ids_host(ids, off, L, pad_id, flags)
    w_out, w_len, w_mask, w_stats = R.pad_ref(ids, off, L, pad_id, flags)
    assert np.array_equal(out, w_out) and np.array_equal(lengths, w_len) and np.array_equal(mask, w_mask)
    assert tuple(int(x) for x in stats) == w_stats


def check_pack(S, ids, off, L, pad_id):
    w_out, w_seq, w_pos, w_stats = R.pack_ref(ids, off, L, pad_id)
    rows = w_stats[0]
    # Two spare rows: the call must leave them alone.
    out, seq, pos, stats = S.pack_ids_host(ids, off, L, pad_id, rows_capacity=rows + 2, fill=12345)
    for got, want in ((out, w_out), (seq, w_seq), (pos, w_pos)):
        assert np.array_equal(got[:rows], want) and (got[rows:] == 12345).all()
    assert tuple(int(x) for x in stats) == w_stats
    if rows > 1:  # too few rows: the need is still reported, the rows given are right
        out, seq, pos, stats = S.pack_ids_host(ids, off, L, pad_id, rows_capacity=rows - 1)
        assert np.array_equal(out, w_out[:-1]) and np.array_equal(seq, w_seq[:-1]) and np.array_equal(pos, w_pos[:-1])
        assert tuple(int(x) for x in stats) == w_stats


@pytest.mark.parametrize("base", [0, 7])
def test_host_literal_cases(S, base):
    ids, off = case(LENS, base)
    for flags in range(8):
        for L in (4, 1):
            check_pad(S, ids, off, L, P, flags)
    out, _, mask, _ = S.pad_ids_host(ids, off, 4, P, 6)
    assert out.tolist() == literal_pad(6)[0] and mask.tolist() == MASK_RIGHT
    ids, off = case(PACK_LENS, base)
    check_pack(S, ids, off, 4, P)
    out, seq, pos, _ = S.pack_ids_host(ids, off, 4, P)
    assert (out.tolist(), seq.tolist(), pos.tolist()) == (PACK_OUT, PACK_SEQ, PACK_POS)


def test_host_random(S):
    rng = np.random.default_rng(20240601)
    row_lens = [1, 2, 3, 4, 5, 8, 63, 64, 65]
    for k in range(200):
        L = row_lens[k % len(row_lens)]
        n = int(rng.integers(0, 51))
        lens = rng.integers(0, 3 * L + 1, size=n)
        base = int(rng.integers(0, 20)) if k % 3 == 0 else 0
        off = np.zeros(n + 1, dtype=np.uint64)
        off[1:] = np.cumsum(lens, dtype=np.uint64)
        off += np.uint64(base)
        ids = rng.integers(-5, 32000, size=int(off[-1]), dtype=np.int32)
        pad_id = (-1, -100, 0, 2**31 - 1, -2**31)[k % 5]
        check_pad(S, ids, off, L, pad_id, k % 8)
        check_pack(S, ids, off, L, pad_id)


def test_host_nullable_outputs(S):
    ids, off = case(LENS, 3)
    want = R.pad_ref(ids, off, 4, P, 5)
    for absent in range(8):
        wl, wm, ws = not absent & 1, not absent & 2, not absent & 4
        out, lengths, mask, stats = S.pad_ids_host(ids, off, 4, P, 5, with_lengths=wl, with_mask=wm, with_stats=ws)
        assert np.array_equal(out, want[0])
        assert lengths is None if not wl else np.array_equal(lengths, want[1])
        assert mask is None if not wm else np.array_equal(mask, want[2])
        assert stats is None if not ws else tuple(int(x) for x in stats) == want[3]
    ids, off = case(PACK_LENS, 3)
    want = R.pack_ref(ids, off, 4, P)
    for absent in range(8):
        wq, wp, ws = not absent & 1, not absent & 2, not absent & 4
        out, seq, pos, stats = S.pack_ids_host(ids, off, 4, P, with_seq=wq, with_pos=wp, with_stats=ws)
        assert np.array_equal(out, want[0])
        assert seq is None if not wq else np.array_equal(seq, want[1])
        assert pos is None if not wp else np.array_equal(pos, want[2])
        assert stats is None if not ws else tuple(int(x) for x in stats) == want[3]


def test_host_empty_batch(S):
    ids, off = np.zeros(0, np.int32), np.array([5], dtype=np.uint64)
    out, lengths, mask, stats = S.pad_ids_host(ids, off, 4, P)
    assert out.shape == (0, 4) and lengths.shape == (0,) and stats.tolist() == [0, 0]
    out, seq, pos, stats = S.pack_ids_host(ids, off, 4, P, rows_capacity=2, fill=7)
    assert (out == 7).all() and (seq == 7).all() and (pos == 7).all() and stats.tolist() == [0, 0]


@pytest.mark.parametrize("device", [False, True])
def test_status_codes(S, device):
    """The same argument checks in front of the host and the device entries;
    the device entries return before they enqueue anything."""
    L = S.lib()
    ids, off = case(LENS)
    out = np.zeros(64, dtype=np.int32)
    V = ctypes.c_void_p
    a_ids, a_off, a_out = V(ids.ctypes.data), V(off.ctypes.data), V(out.ctypes.data)
    n = len(LENS)

    def pad(off_p=a_off, out_p=a_out, n=n, row_len=4, flags=0):
        if device:
            return L.spm_hip_pad_ids(a_ids, off_p, n, row_len, P, flags, out_p, None, None, None, None)
        return L.spm_hip_pad_ids_host(a_ids, off_p, n, row_len, P, flags, out_p, None, None, None)

    def pack(off_p=a_off, out_p=a_out, n=n, row_len=4):
        if device:
            return L.spm_hip_pack_ids(a_ids, off_p, n, row_len, P, 16, out_p, None, None, None, None)
        return L.spm_hip_pack_ids_host(a_ids, off_p, n, row_len, P, 16, out_p, None, None, None)

    for call in (pad, pack):
        assert call(row_len=0) == S.SPM_INVALID_ARGUMENT
        assert call(row_len=1 << 31) == S.SPM_INVALID_ARGUMENT
        assert call(out_p=None) == S.SPM_INVALID_ARGUMENT
        assert call(off_p=None) == S.SPM_INVALID_ARGUMENT
        assert call(n=0, out_p=None) == S.SPM_INVALID_ARGUMENT  # checked before n == 0 returns
        assert L.spm_hip_last_error()
    for bit in (8, 16, 1 << 31):
        assert pad(flags=bit) == S.SPM_INVALID_ARGUMENT
        assert pad(flags=bit | 7) == S.SPM_INVALID_ARGUMENT
    assert pack(n=(1 << 31)) == S.SPM_OUT_OF_RANGE
    assert pad(n=(1 << 63), row_len=4) == S.SPM_OUT_OF_RANGE
    if not device:
        assert pad() == S.SPM_OK and pack() == S.SPM_OK
        assert pad(row_len=(1 << 31) - 1, n=0) == S.SPM_OK  # the largest row, no sentence
        assert pack(n=0) == S.SPM_OK
