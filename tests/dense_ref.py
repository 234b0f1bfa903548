"""Restatement of the dense id batches (spm_hip_pad_ids / spm_hip_pack_ids) in
plain numpy, written from the rules in include/spm_hip.h: per sentence, with
slices, not per output slot as the engine computes them."""
import numpy as np

PAD_LEFT, TRUNCATE_LEFT, KEEP_END = 1, 2, 4


def pad_ref(ids, off, row_len, pad_id, flags=0):
    """-> (out int32[n, L], lengths int32[n], mask uint8[n, L], (cut, dropped))."""
    ids = np.asarray(ids, dtype=np.int32)
    off = [int(x) for x in off]
    n, L = len(off) - 1, int(row_len)
    out = np.full((n, L), pad_id, dtype=np.int32)
    lengths = np.zeros(n, dtype=np.int32)
    mask = np.zeros((n, L), dtype=np.uint8)
    cut = dropped = 0
    for i in range(n):
        sent = ids[off[i]:off[i + 1]]
        k = min(len(sent), L)
        kept = sent[len(sent) - k:] if flags & TRUNCATE_LEFT else sent[:k]
        kept = kept.copy()
        if len(sent) > L:
            cut += 1
            dropped += len(sent) - L
            if flags & KEEP_END:
                if flags & TRUNCATE_LEFT:
                    kept[0] = sent[0]
                else:
                    kept[-1] = sent[-1]
        lo = L - k if flags & PAD_LEFT else 0
        out[i, lo:lo + k] = kept
        mask[i, lo:lo + k] = 1
        lengths[i] = k
    return out, lengths, mask, (cut, dropped)


def pack_ref(ids, off, row_len, pad_id):
    """-> (out, seq, pos, each int32[ceil(T / L), L], (rows, T))."""
    ids = np.asarray(ids, dtype=np.int32)
    off = [int(x) for x in off]
    n, L = len(off) - 1, int(row_len)
    stream = ids[off[0]:off[-1]]
    T = len(stream)
    rows = -(-T // L)
    lens = [off[i + 1] - off[i] for i in range(n)]
    seq = np.concatenate([np.full(m, i, dtype=np.int32) for i, m in enumerate(lens)] + [np.zeros(0, np.int32)])
    pos = np.concatenate([np.arange(m, dtype=np.int32) for m in lens] + [np.zeros(0, np.int32)])
    tail = rows * L - T

    def grid(a, fill):
        return np.concatenate([a, np.full(tail, fill, dtype=np.int32)]).reshape(rows, L)

    return grid(stream, pad_id), grid(seq, -1), grid(pos, 0), (rows, T)


def csr(rows):
    """Lists of ids -> (ids int32, off uint64[n + 1])."""
    off = np.zeros(len(rows) + 1, dtype=np.uint64)
    if rows:
        off[1:] = np.cumsum([len(r) for r in rows], dtype=np.uint64)
    flat = np.array([x for r in rows for x in r], dtype=np.int32)
    return flat, off
