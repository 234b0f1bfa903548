"""Python restatement of the unigram lattice scores (test infrastructure).

The checker of spm_hip_entropy_batch and spm_hip_sample_encode_and_score_batch,
written from the arithmetic that include/spm_hip.h spells out, on the lattice
and forward pass of sample_ref.Model:

  * entropy():  H[0] = 0 and, over the nodes (b, p) in end_nodes_ order,
      lp   = fl(fl(fl(theta * s) + A[b]) - A[p])
      H[p] = fl(H[p] + fl((float) exp((double) lp) * fl(H[b] + lp)));
    the answer is -H[len] (-0.0 for an empty sentence);
  * entropy_exact(): the same quantity in fp64 with exact LogSumExp;
  * count_paths(): the number of segmentations, an integer;
  * path_score(): fl(T - A[len]) with T = 0 and T = fl(T + fl(theta * s))
    over the path's nodes from the first to the last;
  * sample_key(): the key of sample j of the sentence with global index g.
"""
import math

import numpy as np

import sample_ref as R

F32 = np.float32


SAMPLE_STRIDE = 0xD1B54A32D192ED03


def sample_seed(seed, j):
    """Seed of sample j: sample 0 keeps the caller's seed."""
    return seed & R.M64 if j == 0 else R.mix(seed + SAMPLE_STRIDE * j)


def sample_key(seed, g, j):
    """Sample 0 is SampleEncode's stream of (seed, g); sample j > 0 is that
    stream for the seed mix(seed + SAMPLE_STRIDE * j) at the same index."""
    return R.sentence_key(sample_seed(seed, j), g)


def entropy(rm, s, theta, with_log_z=False, lat=None):
    """(float32) entropy of sentence bytes s at inverse temperature theta
    (lat: the sentence's lattice when the caller has it)."""
    if len(s) == 0:
        return (F32(-0.0), F32(0.0)) if with_log_z else F32(-0.0)
    lat = lat or rm.lattice(s)
    A = rm.forward(lat, theta)
    theta = F32(theta)
    H = [F32(0.0)] * (lat.nc + 1)
    for p in range(1, lat.nc + 1):
        for b, sc, _ in lat.end_nodes[p]:
            lp = F32(F32(F32(theta * sc) + A[b]) - A[p])
            H[p] = F32(H[p] + F32(F32(math.exp(float(lp))) * F32(H[b] + lp)))
    h = F32(-H[lat.nc])
    return (h, A[lat.nc]) if with_log_z else h


def entropy_exact(rm, s, theta):
    """The entropy in fp64: (H, log Z)."""
    if len(s) == 0:
        return 0.0, 0.0
    lat = rm.lattice(s)
    theta = float(F32(theta))
    A = [0.0] * (lat.nc + 1)
    H = [0.0] * (lat.nc + 1)
    for p in range(1, lat.nc + 1):
        terms = [theta * float(sc) + A[b] for b, sc, _ in lat.end_nodes[p]]
        top = max(terms)
        A[p] = top + math.log(sum(math.exp(t - top) for t in terms))
        for (b, _, _), t in zip(lat.end_nodes[p], terms):
            lp = t - A[p]
            H[p] += math.exp(lp) * (H[b] + lp)
    return -H[lat.nc], A[lat.nc]


def count_paths(rm, s, lat=None):
    """The number of segmentations of s."""
    lat = lat or rm.lattice(s)
    N = [0] * (lat.nc + 1)
    N[0] = 1
    for p in range(1, lat.nc + 1):
        N[p] = sum(N[b] for b, _, _ in lat.end_nodes[p])
    return N[lat.nc]


def path_score(rm, s, theta, ids, lens=None):
    """Score of the path `ids` of s: fl(sum of fl(theta * s_k), first to last,
    - A[len]).  Without byte lengths the path is found by matching the ids on
    the lattice, where one unknown id stands for a run of one or more unknown
    nodes (the processor merges such runs); None when no path matches."""
    if len(s) == 0:
        return F32(0.0) if len(ids) == 0 else None
    lat = rm.lattice(s)
    A = rm.forward(lat, theta)
    theta = F32(theta)
    begin = [[] for _ in range(lat.nc + 1)]
    for e in range(lat.nc + 1):
        for b, sc, pid in lat.end_nodes[e]:
            begin[b].append((e, sc, pid))
    if lens is not None:
        char_of = {b: c for c, b in enumerate(lat.cs)}
        pos, total = 0, F32(0.0)
        for pid, ln in zip(ids, lens):
            b, e = char_of[pos], char_of[pos + int(ln)]
            sc = [x for x in begin[b] if x[0] == e and x[2] == int(pid)]
            if not sc:
                return None
            total = F32(total + F32(theta * sc[0][1]))
            pos += int(ln)
        return F32(total - A[lat.nc]) if pos == len(s) else None
    ids = [int(x) for x in ids]
    # (position, index into ids, inside an unknown run) -> list of node scores
    stack = [(0, 0, False, ())]
    while stack:
        p, k, in_unk, scores = stack.pop()
        if p == lat.nc:
            if k == len(ids):
                total = F32(0.0)
                for sc in scores:
                    total = F32(total + F32(theta * sc))
                return F32(total - A[lat.nc])
            continue
        for e, sc, pid in begin[p]:
            if in_unk and pid == rm.unk_id:
                stack.append((e, k, True, scores + (sc,)))
            if k < len(ids) and pid == ids[k]:
                stack.append((e, k + 1, pid == rm.unk_id, scores + (sc,)))
    return None
