"""Python restatement of BPE-dropout (test infrastructure).

The checker of spm_hip_bpe_dropout_encode_batch: bpe::Model::SampleEncode of
the `sentencepiece` package (0.2.2, bpe_model.cc) written out literally, with
the one change include/spm_hip.h spells out: the package draws from a
process-wide mt19937 at every pop, here the decision is the draw named by the
popped pair's bytes in the sentence's counter-based stream.

  * the symbol list (PrefixMatch: the longest USER_DEFINED piece, frozen, else
    OneCharLen clamped to the sentence),
  * the agenda ordered by (score descending, left index ascending),
  * the stale check (an emptied symbol, or a size that no longer matches),
  * the drop at the pop, after the stale check,
  * rev_merge (every pushed pair whose piece is UNUSED, the last push wins)
    and the recursive resegment.

encode() is one draw; path_probabilities() enumerates the keep / drop tree of
a short sentence and returns every segmentation with its exact probability.
"""
import heapq
import math

import numpy as np

import byte_fallback_ref
from sample_ref import draw_u, sentence_key

NORMAL, UNKNOWN, CONTROL, USER_DEFINED, UNUSED, BYTE = 1, 2, 3, 4, 5, 6
_CHAR_LEN = (1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 3, 4)  # util.h: OneCharLen


class Model:
    """pieces_ (NORMAL, USER_DEFINED, UNUSED) and reserved_id_map_ (the rest) of
    ModelInterface::InitializePieces; types: an optional override per id."""

    def __init__(self, model_bytes, types=None):
        rows = byte_fallback_ref.read_pieces(model_bytes)
        self.pieces, self.reserved, self.user = {}, {}, []
        self.score, self.type = [], []
        self.unk_id = 0
        for i, (p, s, t) in enumerate(rows):
            if types is not None:
                t = types[i]
            self.score.append(s)
            self.type.append(t)
            if t == UNKNOWN:
                self.unk_id = i
            if t in (NORMAL, USER_DEFINED, UNUSED):
                self.pieces.setdefault(p, i)
                if t == USER_DEFINED:
                    self.user.append(p)
            else:
                self.reserved.setdefault(p, i)

    def piece_to_id(self, w):
        if w in self.reserved:
            return self.reserved[w]
        return self.pieces.get(w, self.unk_id)

    def prefix_match(self, s, q):
        """(length, frozen) of the symbol that starts at s[q]."""
        best = 0
        for u in self.user:
            if len(u) > best and s.startswith(u, q):
                best = len(u)
        if best:
            return best, True
        return min(_CHAR_LEN[s[q] >> 4], len(s) - q), False


class _State:
    """The loop's state between two pops."""

    def __init__(self, m, s):
        self.m, self.s = m, s
        self.off, self.len, self.frz, self.prev, self.next = [], [], [], [], []
        self.heap, self.seq, self.rev = [], 0, {}
        q = 0
        while q < len(s):
            n, frozen = m.prefix_match(s, q)
            k = len(self.off)
            self.off.append(q)
            self.len.append(n)
            self.frz.append(frozen)
            self.prev.append(k - 1)
            q += n
            self.next.append(-1 if q >= len(s) else k + 1)
        for k in range(1, len(self.off)):
            self.maybe_add(k - 1, k)

    def copy(self):
        c = _State.__new__(_State)
        c.m, c.s, c.off, c.frz = self.m, self.s, self.off, self.frz
        c.len, c.prev, c.next = list(self.len), list(self.prev), list(self.next)
        c.heap, c.seq, c.rev = list(self.heap), self.seq, dict(self.rev)
        return c

    def maybe_add(self, left, right):
        if left < 0 or right < 0 or self.frz[left] or self.frz[right]:
            return
        size = self.len[left] + self.len[right]
        w = self.s[self.off[left]:self.off[left] + size]
        pid = self.m.pieces.get(w)
        if pid is None:
            return
        # (score descending, left ascending); seq only keeps tuples comparable.
        heapq.heappush(self.heap, (-self.m.score[pid], left, self.seq, right, size))
        self.seq += 1
        if self.m.type[pid] == UNUSED:
            self.rev[w] = self.len[left]

    def pop_valid(self):
        """The next popped pair that passes the stale check, or None."""
        while self.heap:
            _, left, _, right, size = heapq.heappop(self.heap)
            if self.len[left] == 0 or self.len[right] == 0 or self.len[left] + self.len[right] != size:
                continue
            return left, right
        return None

    def name(self, top):
        left, right = top
        return self.off[left], self.off[right] + self.len[right]

    def merge(self, top):
        left, right = top
        self.len[left] += self.len[right]
        self.next[left] = self.next[right]
        if self.next[right] >= 0:
            self.prev[self.next[right]] = left
        self.len[right] = 0
        self.maybe_add(self.prev[left], left)
        self.maybe_add(left, self.next[left])

    def finish(self):
        ids, lens = [], []

        def resegment(o, n):
            w = self.s[o:o + n]
            i = self.m.piece_to_id(w)
            if self.m.type[i] != UNUSED or w not in self.m.pieces or w not in self.rev:
                ids.append(i)
                lens.append(n)
                return
            k = self.rev[w]
            resegment(o, k)
            resegment(o + k, n - k)

        k = 0 if self.off else -1
        while k != -1:
            resegment(self.off[k], self.len[k])
            k = self.next[k]
        return ids, lens


def alpha_double(alpha):
    """The C-ABI takes alpha as a float; the test is u < (double) alpha."""
    return float(np.float32(alpha))


def dropped(key, start, end, alpha):
    a = alpha_double(alpha)
    return draw_u(key, (start << 32) | end) < a


def encode(model, norm_sentence, alpha, seed, g):
    """One draw: (ids, lens) of the sentence with global index g under seed."""
    st = _State(model, bytes(norm_sentence))
    key = sentence_key(seed, g)
    while True:
        top = st.pop_valid()
        if top is None:
            return st.finish()
        start, end = st.name(top)
        if dropped(key, start, end, alpha):
            continue
        st.merge(top)


def path_probabilities(model, norm_sentence, alpha):
    """{(ids tuple, lens tuple): probability} over the keep / drop tree: every
    pop that passes the stale check drops with probability alpha.  Short
    sentences only (the tree is exponential)."""
    a = min(max(alpha_double(alpha), 0.0), 1.0)
    out = {}
    stack = [(_State(model, bytes(norm_sentence)), 1.0)]
    while stack:
        st, p = stack.pop()
        top = st.pop_valid()
        if top is None:
            ids, lens = st.finish()
            key = (tuple(ids), tuple(lens))
            out[key] = out.get(key, 0.0) + p
            continue
        if a > 0.0:
            stack.append((st.copy() if a < 1.0 else st, p * a))
        if a < 1.0:
            st.merge(top)
            stack.append((st, p * (1.0 - a)))
    return out


def merge_unknown_runs(ids, lens, unk_id):
    """Consecutive unknown tokens as one (PopulateSentencePieceText)."""
    oi, ol = [], []
    for i, n in zip(ids, lens):
        if oi and i == unk_id and oi[-1] == unk_id:
            ol[-1] += n
        else:
            oi.append(int(i))
            ol.append(int(n))
    return oi, ol


def binned_deviation(probs, counts, draws):
    """Worst |count - N p| / sigma (binomial sigma) over the bins with
    N p >= 25 and over the pooled rest."""
    def sigmas(c, p):
        if p >= 1.0:
            assert c == draws
            return 0.0
        return abs(c - draws * p) / math.sqrt(draws * p * (1.0 - p))

    worst, rest_p, rest_c = 0.0, 0.0, 0
    for key, p in probs.items():
        c = counts.get(key, 0)
        if draws * p >= 25:
            worst = max(worst, sigmas(c, p))
        else:
            rest_p += p
            rest_c += c
    if rest_p > 0.0:
        worst = max(worst, sigmas(rest_c, rest_p))
    return worst
