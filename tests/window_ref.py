"""Restatement of spm_hip_window_ids (a long sentence as rows that overlap by
a stride) as a plain Python loop over the sentences, written from the rule in
include/spm_hip.h."""
import numpy as np

from fit_ref import random_csr  # noqa: F401

def sentence_rows(len_, L, S, h, t):
    """The rows of one sentence: lists of token indices."""
    if len_ <= h + t:
        return [list(range(len_))]
    C = L - h - t
    step, m = C - S, len_ - h - t
    rows, w = [], 0
    while True:
        body = range(w * step, min(w * step + C, m))
        rows.append([0] * h + [h + j for j in body] + [len_ - 1] * t)
        if w * step + C >= m:
            return rows
        w += 1


def window_ref(ids, off, row_len, stride, pad_id, flags=0):
    """-> (out, pos int32[R, L], fresh uint8[R, L], lengths, row_sentence
    int32[R], first_row uint64[n+1], (R, sentences with more than one row))."""
    ids = np.asarray(ids, dtype=np.int32)
    off = [int(x) for x in off]
    n, L = len(off) - 1, int(row_len)
    out, pos, fresh, lengths, row_sentence, first_row, multi = [], [], [], [], [], [0], 0
    for i in range(n):
        rows = sentence_rows(off[i + 1] - off[i], L, stride, flags & 1, flags >> 1 & 1)
        seen = set()
        for r in rows:
            pads = L - len(r)
            out.append([int(ids[off[i] + p]) for p in r] + [pad_id] * pads)
            pos.append(r + [0] * pads)
            fresh.append([int(p not in seen) for p in r] + [0] * pads)
            seen.update(r)
            lengths.append(len(r))
            row_sentence.append(i)
        first_row.append(first_row[-1] + len(rows))
        multi += len(rows) > 1
    grid = lambda a, dt: np.array(a, dtype=dt).reshape(len(a), L)  # noqa: E731
    return (grid(out, np.int32), grid(pos, np.int32), grid(fresh, np.uint8), np.array(lengths, dtype=np.int32),
            np.array(row_sentence, dtype=np.int32), np.array(first_row, dtype=np.uint64), (len(out), multi))


def edge_lens(L, S, flags):
    """Sentence lengths around every edge of the rule."""
    ht = (flags & 1) + (flags >> 1 & 1)
    C = L - ht
    step = C - S
    body = [C - 1, C, C + 1, C + step - 1, C + step, C + step + 1, 3 * C + 2]
    return sorted({0, 1, ht} | {ht + m for m in body if m >= 1})
