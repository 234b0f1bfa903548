"""Restatement of spm_hip_fit_ids (whole sentences share a row, in-order
next-fit) as a plain Python loop over the sentences, written from the rule in
include/spm_hip.h; the cut of a long sentence is dense_ref.pad_ref's."""
import numpy as np

import dense_ref

NO_PLACE = (1 << 64) - 1


def fit_ref(ids, off, row_len, pad_id, flags=0):
    """-> (out, seq, pos int32[R, L], row_lengths int32[R], place uint64[n],
    (R, placed, cut, dropped))."""
    ids = np.asarray(ids, dtype=np.int32)
    off = [int(x) for x in off]
    n, L = len(off) - 1, int(row_len)
    rows, place = [], np.full(n, NO_PLACE, dtype=np.uint64)
    placed = cut = dropped = 0
    for i in range(n):
        sent = ids[off[i]:off[i + 1]]
        if len(sent) == 0:
            continue
        kept, _, _, (c, d) = dense_ref.pad_ref(sent, [0, len(sent)], min(len(sent), L), pad_id, flags)
        kept = kept[0].tolist()
        cut, dropped = cut + c, dropped + d
        if not rows or len(rows[-1]) + len(kept) > L:
            rows.append([])
        place[i] = (len(rows) - 1) * L + len(rows[-1])
        rows[-1] += [(tok, i, j) for j, tok in enumerate(kept)]
        placed += len(kept)
    grid = np.array([r + [(pad_id, -1, 0)] * (L - len(r)) for r in rows], dtype=np.int32).reshape(len(rows), L, 3)
    lengths = np.array([len(r) for r in rows], dtype=np.int32)
    return grid[:, :, 0], grid[:, :, 1], grid[:, :, 2], lengths, place, (len(rows), placed, cut, dropped)


def mixed_lens(rng, n, L):
    """Lengths from {0, 1, L-1, L, L+1, 2L+3}, every second one random in [0, 3L]."""
    special = np.array([0, 1, L - 1, L, L + 1, 2 * L + 3])
    lens = special[rng.integers(0, len(special), size=n)]
    return np.where(np.arange(n) % 2 == 1, rng.integers(0, 3 * L + 1, size=n), lens)


def random_csr(rng, lens, base=0):
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens, dtype=np.uint64)
    ids = rng.integers(0, 32000, size=base + int(off[-1]), dtype=np.int32)
    return ids, off + np.uint64(base)
