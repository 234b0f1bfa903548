"""Python restatement of the unigram trainer's pruning searches (test
infrastructure).

The checker of spm_hip_prune_nbest, of csrc/host_prune_nbest.h and of
spm_hip_model_from_pieces:

  * TrainerModel: the lattice of TrainerModel::SetSentencePieces + PopulateNodes
    (unigram_model_trainer.cc:97-119, unigram_model.cc:535-604) over a bare
    piece list, in the shape nbest_ref.nbest takes.  Every piece is NORMAL with
    id = list index; the trie keys are C strings (a NUL ends a key; of keys
    equal up to their NUL the piece that sorts first as whole bytes wins, as
    BuildTrie's sort and darts-clone's insert decide it); unk_id keeps its
    default 0, so a UNK node carries id 0
    at float32(min(scores)) - float32(10); the walk stops at a NUL byte.
  * prune(): the keep / alternatives decision of PruneSentencePieces
    (unigram_model_trainer.cc:348-371) from NBest(2) of a piece over its own
    string.

Also the piece lists the pruning tests share (CPU host path and GPU kernel).
"""
import numpy as np

import nbest_ref
import sample_ref

F32 = np.float32
MAX_HYPS = 4096   # hypotheses of the device slab (spm_hip_prune_nbest)


def _bytes(p):
    return p if isinstance(p, bytes) else p.encode()


class TrainerModel:
    def __init__(self, pieces, scores):
        self.pieces = [_bytes(p) for p in pieces]
        self.scores = [F32(s) for s in np.asarray(scores, dtype=np.float32)]
        assert len(self.pieces) == len(self.scores) and self.pieces
        self.table = {}
        self.prefixes = set()
        for i, p in sorted(enumerate(self.pieces), key=lambda ip: (ip[1], ip[0])):
            key = p.split(b"\0", 1)[0]
            if not key or key in self.table:
                continue
            self.table[key] = (i, self.scores[i])
            for k in range(1, len(key) + 1):
                self.prefixes.add(key[:k])
        self.unk_id = 0
        self.unk_score = F32(min(self.scores) - F32(10.0))

    def lattice(self, s):
        s = _bytes(s)
        nb = len(s)
        cs, q = [], 0
        while q < nb:  # SetSentence (unigram_model.cc:147-187)
            cs.append(q)
            q += min(sample_ref._CHAR_LEN[s[q] >> 4], nb - q)
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
                end_nodes[p + length].append((p, ent[1], ent[0]))
                if length == 1:
                    single = True
            if not single:
                end_nodes[p + 1].append((p, self.unk_score, self.unk_id))
        return sample_ref.Lattice(cs, end_nodes)


def chars(piece):
    """Char positions of a piece as SetSentence cuts them (alt_off's unit)."""
    s, q, n = _bytes(piece), 0, 0
    while q < len(s):
        q += min(sample_ref._CHAR_LEN[s[q] >> 4], len(s) - q)
        n += 1
    return n


def prune_string(model, s, shrink_at=nbest_ref.MAX_AGENDA):
    """(keep, alternatives, hyps) of one piece string under `model`."""
    paths, stats = nbest_ref.nbest(model, _bytes(s), 2, shrink_at)
    if len(paths) == 1:
        return 1, [], stats[0]
    if len(paths[0][0]) >= 2:
        return 0, [], stats[0]
    return 1, list(paths[1][0]), stats[0]


def prune(pieces, scores, i, model=None):
    return prune_string(model or TrainerModel(pieces, scores), pieces[i])


def prune_all(pieces, scores):
    """[(keep, alternatives, hyps)] per piece."""
    model = TrainerModel(pieces, scores)
    return [prune_string(model, p) for p in pieces]


def expect_device(ref, max_hyps=MAX_HYPS):
    """What spm_hip_prune_nbest returns for a restatement result: a search of
    more than max_hyps hypotheses is flagged keep = 2 with no alternatives."""
    keep, alt, hyps = ref
    return (2, []) if hyps > max_hyps else (keep, alt)


def branches(refs, max_hyps=MAX_HYPS):
    """(keep 0, keep 1 without alternatives, keep 1 with alternatives, keep 2)."""
    out = [0, 0, 0, 0]
    for keep, alt, hyps in refs:
        if hyps > max_hyps:
            out[3] += 1
        elif keep == 0:
            out[0] += 1
        else:
            out[2 if alt else 1] += 1
    return tuple(out)


# ---- the piece lists -------------------------------------------------------
def _f32(xs):
    return np.asarray(xs, dtype=np.float32)


NESTED_SHAPES = {
    "ties": lambda k: -float(k),
    "affine": lambda k: -(3.0 + 0.37 * k),
    "convex": lambda k: -(0.5 * k + 0.01 * k * k),
}


def nested(ch, n, shape):
    """ch * k for k = 1..n, scores NESTED_SHAPES[shape](k) rounded to float32."""
    f = NESTED_SHAPES[shape]
    return [(ch * k).encode() for k in range(1, n + 1)], _f32([f(k) for k in range(1, n + 1)])


RANDOM_ALPHABET = ["a", "b", "あ", "𝄞", "é"]


def random_list(seed=3, count=300, alphabet=RANDOM_ALPHABET, max_chars=8):
    """`count` distinct pieces of 1..max_chars chars, scores -0.5 * randint(1, 12)."""
    rng = np.random.RandomState(seed)
    seen, pieces = set(), []
    while len(pieces) < count:
        n = int(rng.randint(1, max_chars + 1))
        p = "".join(alphabet[int(rng.randint(0, len(alphabet)))] for _ in range(n))
        if p not in seen:
            seen.add(p)
            pieces.append(p.encode())
    scores = _f32([-0.5 * int(rng.randint(1, 13)) for _ in pieces])
    return pieces, scores


def unk_list():
    """Pieces with chars that are no piece of their own: UNK nodes (id 0) in
    the lattices and in the alternatives."""
    pieces = ["ab", "a", "abc", "xbc", "bc", "axc", "あx", "xあ", "axb", "ax", "xb", "xyz", "b𝄞c", "𝄞c", "ab𝄞"]
    scores = [-2.0, -1.0, -3.5, -3.0, -1.5, -4.0, -2.5, -2.5, -3.0, -2.0, -2.0, -6.0, -3.0, -2.0, -2.5]
    return [p.encode() for p in pieces], _f32(scores)


def collision_list():
    """Piece 0 is a one-char piece that also occurs inside others: a real id 0
    next to the UNK nodes' id 0 ('z' and 'q' are no pieces)."""
    pieces = ["a", "aa", "ab", "b", "aab", "aza", "za", "az", "aaa", "qa", "aq", "baa"]
    scores = [-1.0, -2.0, -2.5, -1.5, -3.0, -5.0, -3.0, -3.0, -3.0, -2.0, -2.0, -3.5]
    return [p.encode() for p in pieces], _f32(scores)


def edge_list():
    """A piece of one char, a piece with an embedded NUL (its trie key is the
    part before the NUL), a piece ending in a truncated UTF-8 lead byte."""
    pieces = [b"a", b"ab", b"b", b"ab\0cd", b"cd", b"c", b"a\xe3", b"\xe3\x81\x82\xe3\x81", b"\xe3\x81\x82",
              b"b\xf0\x9d", b"d\0"]
    scores = [-1.0, -1.5, -1.0, -4.0, -1.5, -1.0, -3.0, -3.0, -2.0, -3.5, -2.0]
    return pieces, _f32(scores)


def nul_first_list():
    """A NUL-holding piece listed before the piece its trie key equals: the
    key keeps the later, shorter piece (the one that sorts first)."""
    pieces = [b"ab\0cd", b"a", b"b", b"ab", b"c\0x", b"c\0", b"abc"]
    scores = [-4.0, -1.0, -1.0, -1.5, -2.0, -1.0, -2.5]
    return pieces, _f32(scores)


def sized_list(V, seed=11):
    """V distinct pieces over a b c (V = 1: a one-piece list)."""
    if V == 1:
        return [b"abc"], _f32([-2.0])
    return random_list(seed=seed + V, count=V, alphabet=["a", "b", "c"], max_chars=7)


def boundary_list(n):
    """Pieces of n - 1, n, n + 1 bytes (the fast kernels' 16-byte and the
    ring's 64-byte limits) over a small alphabet with every char a piece."""
    base = "abcdefghij"
    long_ = [(base * 8)[:m] for m in (n - 1, n, n + 1)]
    pieces = list("abcdefghij") + ["ab", "abc", "cde", "ij", "ja", "fgh", "hij", "defg"] + long_
    scores = [-3.0 - 0.1 * k for k in range(10)] + [-4.0, -5.5, -5.0, -4.5, -4.5, -6.0, -5.5, -7.0] + \
             [-0.4 * m for m in (n - 1, n, n + 1)]
    return [p.encode() for p in pieces], _f32(scores)


def prefixed_batch(pieces, scores, copies):
    """The list, then `copies` more copies of it, copy c = 1.. under the prefix
    chr(0x4E00 + c): one 3-byte char that is no piece of its own.  A copy's
    piece has the base piece's lattice behind a first position that holds a
    UNK node and the copy's own pieces; only those carry the copy's ids."""
    out, sc = list(pieces), [scores]
    for c in range(1, copies + 1):
        pre = chr(0x4E00 + c).encode()
        out += [pre + p for p in pieces]
        sc.append(scores)
    return out, np.concatenate(sc).astype(np.float32)


def prefixed_batch_refs(pieces, scores, copies):
    """prune_all of prefixed_batch(...), one search per distinct lattice:
    copy 1's results with its ids [V, 2V) moved to the copy's range."""
    V = len(pieces)
    bp, bs = prefixed_batch(pieces, scores, copies)
    model = TrainerModel(bp, bs)
    refs = [prune_string(model, p) for p in bp[:2 * V]]
    for c in range(2, copies + 1):
        for keep, alt, hyps in refs[V:2 * V]:
            refs.append((keep, [i + (c - 1) * V if V <= i < 2 * V else i for i in alt], hyps))
    return bp, bs, model, refs


def cases():
    """name -> (pieces, scores): every list the host path and the kernel are
    checked on (the grid-stride batch is built from 'random' by the GPU test)."""
    out = {}
    for shape in NESTED_SHAPES:
        out["nested_a96_" + shape] = nested("a", 96, shape)
    for shape in NESTED_SHAPES:
        out["nested_hiragana16_" + shape] = nested("あ", 16, shape)
        out["nested_clef16_" + shape] = nested("𝄞", 16, shape)
    out["random"] = random_list()
    out["unk"] = unk_list()
    out["collision"] = collision_list()
    out["edges"] = edge_list()
    out["nul_first"] = nul_first_list()
    for V in (1, 63, 64, 65, 129):
        out["sized_%d" % V] = sized_list(V)
    for n in (16, 64):
        out["boundary_%d" % n] = boundary_list(n)
    return out


CASE_NAMES = sorted(cases())
BATCH_COPIES = 54   # 300 * 55 = 16500 pieces: more than the kernel's 16384 lanes
_refs = {}


def case_refs(name):
    """(pieces, scores, model, [(keep, alternatives, hyps)]) of a case, or of
    'batch' (the random list under BATCH_COPIES prefixes); computed once per
    process and shared by the tests, which leave it unchanged."""
    if name not in _refs:
        if name == "batch":
            _refs[name] = prefixed_batch_refs(*random_list(), BATCH_COPIES)
        else:
            pieces, scores = cases()[name]
            model = TrainerModel(pieces, scores)
            _refs[name] = (pieces, scores, model, [prune_string(model, p) for p in pieces])
    return _refs[name]
