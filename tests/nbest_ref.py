"""Python restatement of the unigram n-best search (test infrastructure).

The checker of spm_hip_nbest_encode_batch and of csrc/host_nbest.h, written
from the arithmetic include/spm_hip.h spells out, on top of sample_ref.Model's
lattice:

  * Viterbi (unigram_model.cc:222-261): strict >, the first left node wins,
  * the A* search of Lattice::NBest (:339-478) with float32 scalars,
  * libstdc++'s __push_heap / __adjust_heap written out, so hypotheses of
    equal fx pop in std::priority_queue's order,
  * the agenda shrink (:464-474), its threshold a parameter (shrink_at),
  * the path score of Model::NBestEncode (:729-753): the left-to-right
    float32 sum of the node scores, not fx.

nbest() returns (paths, stats): paths = [(ids, byte lengths, float32 score)],
stats = (hypotheses allocated, largest agenda).
"""
import numpy as np

import sample_ref

F32 = np.float32
MAX_AGENDA = 100000   # kMaxAgendaSize
MIN_AGENDA = 512      # kMinAgendaSize


def _push_heap(heap, hole, value):
    """std::__push_heap with top index 0; heap[hole] is the free slot."""
    while hole > 0:
        parent = (hole - 1) // 2
        if not heap[parent][0] < value[0]:
            break
        heap[hole] = heap[parent]
        hole = parent
    heap[hole] = value


def heap_push(heap, value):
    heap.append(value)
    _push_heap(heap, len(heap) - 1, value)


def heap_pop(heap):
    """top(), then std::pop_heap (__adjust_heap over len - 1 entries) + pop_back."""
    top = heap[0]
    value = heap.pop()
    n = len(heap)
    if n > 0:
        hole = child = 0
        while child < (n - 1) // 2:
            child = 2 * (child + 1)
            if heap[child][0] < heap[child - 1][0]:
                child -= 1
            heap[hole] = heap[child]
            hole = child
        if n % 2 == 0 and child == (n - 2) // 2:
            child = 2 * (child + 1)
            heap[hole] = heap[child - 1]
            hole = child - 1
        _push_heap(heap, hole, value)
    return top


def clamp(nbest_size):
    return max(1, min(int(nbest_size), 1024))


def nbest(model, s, nbest_size, shrink_at=MAX_AGENDA):
    """The n best paths of normalized bytes s under sample_ref.Model `model`."""
    if len(s) == 0:
        return [([], [], F32(0.0))], (0, 0)
    N = clamp(nbest_size)
    lat = model.lattice(s)
    nc = lat.nc
    # Nodes: 0 = BOS (ends at 0), 1 = EOS (begins at nc), then the lattice's.
    begin, score, pid, end_of = [0, nc], [F32(0.0), F32(0.0)], [-1, -1], [0, nc]
    end_lists = [[] for _ in range(nc + 1)]   # in end_nodes_ insertion order
    end_lists[0].append(0)
    by_begin = [[] for _ in range(nc + 1)]
    for e in range(1, nc + 1):
        for b, sc, i in lat.end_nodes[e]:
            nd = len(begin)
            begin.append(b)
            score.append(F32(sc))
            pid.append(i)
            end_of.append(e)
            end_lists[e].append(nd)
            by_begin[b].append(nd)
    by_begin[nc].append(1)
    bt = [F32(0.0)] * len(begin)
    prev = [-1] * len(begin)
    for p in range(nc + 1):
        for r in by_begin[p]:
            best, best_score = -1, F32(0.0)
            for l in end_lists[p]:
                sc = F32(bt[l] + score[r])
                if best < 0 or sc > best_score:
                    best, best_score = l, sc
            prev[r], bt[r] = best, best_score

    def emit(nodes):
        total = F32(0.0)
        for nd in nodes:
            total = F32(total + score[nd])
        return ([pid[nd] for nd in nodes],
                [lat.cs[end_of[nd]] - lat.cs[begin[nd]] for nd in nodes], total)

    if N == 1:
        nodes, nd = [], prev[1]
        while nd > 0:
            nodes.append(nd)
            nd = prev[nd]
        return [emit(nodes[::-1])], (0, 0)
    hnode, hnext, hgx = [1], [-1], [score[1]]
    heap = []
    heap_push(heap, (score[1], 0))
    results, max_agenda = [], 1
    while heap:
        top = heap_pop(heap)[1]
        tn = hnode[top]
        if tn == 0:
            nodes, h = [], hnext[top]
            while hnext[h] != -1:
                nodes.append(hnode[h])
                h = hnext[h]
            results.append(emit(nodes))
            if len(results) == N:
                break
            continue
        gx = hgx[top]
        for l in end_lists[begin[tn]]:
            hnode.append(l)
            hnext.append(top)
            hgx.append(F32(score[l] + gx))
            heap_push(heap, (F32(bt[l] + gx), len(hnode) - 1))
        max_agenda = max(max_agenda, len(heap))
        if len(heap) >= shrink_at:
            kept = []
            for _ in range(min(MIN_AGENDA, N * 10)):
                heap_push(kept, heap_pop(heap))
            heap = kept
    return results, (len(hnode), max_agenda)


def merge_unknown(ids, unk_id):
    """PopulateSentencePieceText's unknown-run merge on a path's ids."""
    out = []
    for i in ids:
        if i == unk_id and out and out[-1] == unk_id:
            continue
        out.append(i)
    return out


# ---- shared by the n-best tests --------------------------------------------
def abc_model():
    """UnigramModelTest.ModelNBestTest / LatticeTest.NBestTest."""
    from model_builder import base_pieces, model
    return model(base_pieces() + [("a", 0.0, 1), ("b", 0.0, 1), ("c", 0.0, 1), ("ab", 2.0, 1), ("bc", 5.0, 1),
                                  ("abc", 10.0, 1)], add_dummy_prefix=False)


ABC_ORDER = ["abc", "a bc", "ab c", "a b c"]


def ties_model():
    """a -1, aa -2, aaa -3, aaaa -4: every path of 'a' * k scores -k."""
    from model_builder import base_pieces, model
    return model(base_pieces() + [("a" * k, -float(k), 1) for k in (1, 2, 3, 4)], add_dummy_prefix=False)


def read_fixture(path):
    """[rows] per input line of a gzip-compressed tests/golden n-best fixture
    (per line the path count, then one row of ids per path), and its rows'
    text: what `spm_encode --output_format=nbest_id` prints."""
    import gzip
    lines = gzip.open(path, "rt").read().split("\n")
    out, text, k = [], [], 0
    while k < len(lines) and lines[k] != "":
        cnt = int(lines[k])
        text += lines[k + 1:k + 1 + cnt]
        out.append([[int(x) for x in r.split()] for r in lines[k + 1:k + 1 + cnt]])
        k += 1 + cnt
    return out, "".join(r + "\n" for r in text).encode()


def short_sentences(norm):
    """Up to 60 distinct 12-char prefixes of normalized lines: lattices small
    enough for sample_ref.Model.enumerate_paths."""
    out = []
    for nz in norm:
        t = nz.decode()[:12].encode()
        if t and t not in out:
            out.append(t)
    return out[:60]


def exact_top(model, s, nbest):
    """(paths of s, the exact top-nbest set of (ids, lens) or None) by
    exhaustive enumeration in float64: None when the nbest-th and the next
    total are within 1e-3, where float32 rounding may order them either way."""
    import math
    # enumerate_paths at theta 1: log p = the path's float64 total, up to a constant.
    allp = sorted(((math.log(p), k) for k, p in model.enumerate_paths(s, 1.0).items()), reverse=True)
    if len(allp) > nbest and allp[nbest - 1][0] - allp[nbest][0] <= 1e-3:
        return len(allp), None
    return len(allp), {k for _, k in allp[:nbest]}


def score_bits(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def parse_selftest(text):
    """nbest_selftest host output -> [(paths [(ids, lens, score bits)], hyps, max agenda, shrinks)]."""
    rows = text.split("\n")
    out, k = [], 0
    while k < len(rows) and rows[k] != "":
        cnt, hyps, agenda, shrinks = (int(x) for x in rows[k].split())
        paths = []
        for r in rows[k + 1:k + 1 + cnt]:
            f = r.split()
            toks = [t.split(":") for t in f[1:]]
            paths.append(([int(t[0]) for t in toks], [int(t[1]) for t in toks], int(f[0], 16)))
        out.append((paths, hyps, agenda, shrinks))
        k += 1 + cnt
    return out
