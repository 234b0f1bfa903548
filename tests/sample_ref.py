"""Python restatement of the unigram sampler (test infrastructure).

The checker of spm_hip_sample_encode_batch, written from the arithmetic that
include/spm_hip.h spells out, with numpy float32 / float64 scalars:

  * the lattice of Model::PopulateNodes (unigram_model.cc:535-604) from the
    pieces model_reader.py reads,
  * LogSumExp (unigram_model.cc:51-63),
  * the forward pass A[p] and the backward draw of Lattice::Sample
    (unigram_model.cc:488-526),
  * the counter-based random stream (mix / key / draw).

sample() returns the tokens and the margin: the smallest distance of any
draw's u to a boundary of its CDF.  enumerate_paths() lists every path of a
short sentence with its exact probability, proportional to
exp(theta * sum of scores).
"""
import math

import numpy as np

from model_builder import base_pieces, model
from model_reader import read_pieces

F32 = np.float32
NORMAL, UNKNOWN, CONTROL, USER_DEFINED, UNUSED = 1, 2, 3, 4, 5
M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
_CHAR_LEN = (1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 3, 4)  # util.h:389


def mix(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sentence_key(seed, g):
    return mix(seed + GOLDEN * (g + 1))


def draw_u(key, k):
    return float(mix(key + GOLDEN * (k + 1)) >> 11) * 2.0 ** -53


def uniform(seed, g, k):
    return draw_u(sentence_key(seed, g), k)


def log_sum_exp(x, y):
    """unigram_model.cc:51-63 outside init mode: float in and out, double exp / log."""
    vmin, vmax = (y, x) if y < x else (x, y)
    if vmax > F32(vmin + F32(50.0)):
        return vmax
    return F32(np.float64(vmax) + math.log(math.exp(float(F32(vmin - vmax))) + 1.0))


class Lattice:
    def __init__(self, cs, end_nodes):
        self.cs = cs                  # byte offset of every char position, + the length
        self.end_nodes = end_nodes    # per char position: [(begin char, score, id)] in end_nodes_ order
        self.nc = len(cs) - 1


class Model:
    def __init__(self, model_bytes):
        pieces = read_pieces(model_bytes)
        self.table = {}
        self.prefixes = set()
        self.unk_id = -1
        mn, mx = F32(np.finfo(np.float32).max), F32(np.finfo(np.float32).tiny)  # FLT_MAX, FLT_MIN (:681-683)
        for i, (p, s, t) in enumerate(pieces):
            if t == UNKNOWN:
                self.unk_id = i
            if t == NORMAL:
                mn, mx = min(mn, F32(s)), max(mx, F32(s))
            if t in (NORMAL, USER_DEFINED, UNUSED):
                self.table[p] = (i, F32(s), t)
                for k in range(1, len(p) + 1):
                    self.prefixes.add(p[:k])
        self.max_score = mx
        self.unk_score = F32(mn - F32(10.0))  # kUnkPenalty (:563)

    def lattice(self, s):
        nb = len(s)
        cs, q = [], 0
        while q < nb:  # SetSentence (:147-187)
            cs.append(q)
            q += min(_CHAR_LEN[s[q] >> 4], nb - q)
        cs.append(nb)
        nc = len(cs) - 1
        end_nodes = [[] for _ in range(nc + 1)]
        for p in range(nc):
            single, cpos = False, p
            for q in range(cs[p], nb):
                if s[q] == 0:
                    break
                key = s[cs[p]:q + 1]
                if key not in self.prefixes:
                    break
                ent = self.table.get(key)
                if ent is None:
                    continue
                while cs[cpos] < q + 1:
                    cpos += 1
                length = cpos - p
                pid, score, t = ent
                if t == UNUSED:
                    continue
                if t == USER_DEFINED:  # length * max_score_ + 1.0 assigned to float (:589-591)
                    score = F32(np.float64(F32(length) * self.max_score) + 1.0)
                end_nodes[p + length].append((p, score, pid))
                if length == 1:
                    single = True
            if not single:
                end_nodes[p + 1].append((p, self.unk_score, self.unk_id))
        return Lattice(cs, end_nodes)

    def forward(self, lat, theta):
        theta = F32(theta)
        A = [F32(0.0)] * (lat.nc + 1)
        for p in range(1, lat.nc + 1):
            first = True
            for b, sc, _ in lat.end_nodes[p]:
                t = F32(F32(theta * sc) + A[b])
                A[p] = t if first else log_sum_exp(A[p], t)
                first = False
        return A

    def prepare(self, s, theta):
        """Lattice, alpha and every position's CDF boundaries (they do not
        depend on the draw): edges[e][i] = (w_0 + .. + w_i) / S for all
        candidates of e but the last."""
        lat = self.lattice(s)
        A = self.forward(lat, theta)
        theta = F32(theta)
        edges = [[] for _ in range(lat.nc + 1)]
        for e in range(1, lat.nc + 1):
            cands = lat.end_nodes[e]
            w = [F32(math.exp(float(F32(F32(A[b] + F32(theta * sc)) - A[e])))) for b, sc, _ in cands]
            S = 0.0
            for x in w:
                S += float(x)
            cum = 0.0
            for i in range(len(cands) - 1):
                cum += float(w[i])
                edges[e].append(cum / S if S != 0.0 else math.nan)
        return lat, edges

    def draw(self, prep, key):
        """One backward walk with the draws of `key`: (ids, byte lengths, margin)."""
        lat, edges = prep
        e, k, margin = lat.nc, 0, math.inf
        ids, lens = [], []
        while e > 0:
            cands = lat.end_nodes[e]
            u = draw_u(key, k)
            k += 1
            pick = len(cands) - 1
            for i, edge in enumerate(edges[e]):
                if u < edge:
                    pick = i
                    break
            for edge in edges[e]:
                if edge == edge:
                    margin = min(margin, abs(u - edge))
            b, _, pid = cands[pick]
            ids.append(pid)
            lens.append(lat.cs[e] - lat.cs[b])
            e = b
        return ids[::-1], lens[::-1], margin

    def sample(self, s, theta, seed, g):
        """One draw for sentence bytes s at global index g.
        Returns (ids, byte lengths, margin)."""
        if len(s) == 0:
            return [], [], math.inf
        return self.draw(self.prepare(s, theta), sentence_key(seed, g))

    def enumerate_paths(self, s, theta):
        """{(ids tuple, byte lengths tuple): probability} over every path of s."""
        lat = self.lattice(s)
        begin = [[] for _ in range(lat.nc + 1)]
        for e in range(lat.nc + 1):
            for b, sc, pid in lat.end_nodes[e]:
                begin[b].append((e, sc, pid))
        out = {}

        def rec(p, ids, lens, total):
            if p == lat.nc:
                out[(tuple(ids), tuple(lens))] = total
                return
            for e, sc, pid in begin[p]:
                rec(e, ids + [pid], lens + [lat.cs[e] - lat.cs[p]], total + float(sc))

        rec(0, [], [], 0.0)
        if not out:
            return {}
        top = max(out.values())
        wsum = sum(math.exp(float(theta) * (v - top)) for v in out.values())
        return {k: math.exp(float(theta) * (v - top)) / wsum for k, v in out.items()}

    def is_path(self, s, ids, lens):
        """The tokens (ids, byte lengths) are a path of s's lattice."""
        lat = self.lattice(s)
        char_of = {b: c for c, b in enumerate(lat.cs)}
        pos = 0
        for pid, ln in zip(ids, lens):
            b, e = char_of.get(pos), char_of.get(pos + int(ln))
            if b is None or e is None or e <= b:
                return False
            if not any(nb == b and nid == int(pid) for nb, _, nid in lat.end_nodes[e]):
                return False
            pos += int(ln)
        return pos == len(s)


# LatticeTest.SampleTest (unigram_model_test.cc:317-357).
ABC_PIECES = [("A", 1.0, 1), ("B", 1.2, 1), ("C", 1.5, 1), ("AB", 1.6, 1),
              ("BC", 1.7, 1), ("ABC", 1.8, 1)]
ABC_THETAS = [0.0, 0.01, 0.5, 0.7, 1.0]
ABC_PATHS = {"A B C": 1.0 + 1.2 + 1.5, "AB C": 1.6 + 1.5, "A BC": 1.0 + 1.7, "ABC": 1.8}


def abc_model():
    return model(base_pieces() + ABC_PIECES, add_dummy_prefix=False)


def abc_expected(theta):
    w = {k: math.exp(theta * v) for k, v in ABC_PATHS.items()}
    z = sum(w.values())
    return {k: v / z for k, v in w.items()}


def abc_name(ids):
    names = [p[0] for p in base_pieces() + ABC_PIECES]
    return " ".join(names[i] for i in ids)
