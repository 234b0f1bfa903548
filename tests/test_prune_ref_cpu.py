"""CPU: the pruning restatement (tests/prune_ref.py) pinned — no GPU calls.

TrainerModel's lattices against sample_ref.Model's (itself pinned to the pip
sentencepiece's fixtures) wherever the two models coincide: a list whose entry
0 is the literal "<unk>", typed UNKNOWN in the .model, absent from the inputs
and not the minimum score.  Then prune()'s three outcomes on lattices small
enough to read, and the hypothesis counts the device and host tests rely on.
"""
import numpy as np
import pytest

import model_builder as MB
import prune_ref as P
import sample_ref as R


def _bits(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def _same_lattice(a, b):
    assert a.cs == b.cs
    assert a.nc == b.nc
    assert len(a.end_nodes) == len(b.end_nodes)
    for x, y in zip(a.end_nodes, b.end_nodes):
        assert [(p, _bits(s), i) for p, s, i in x] == [(p, _bits(s), i) for p, s, i in y]


# Sentences with chars outside every list (U+2585 is the trainer's rare-char
# stand-in), a truncated lead byte and a NUL in the input.
EXTRA = ["a▅b".encode(), "zzz".encode(), "aあ𝄞éb?".encode(), b"ab\xe3\x81", b"ab\0ab", "𝄞𝄞a▅".encode()]


@pytest.mark.parametrize("name", [n for n in P.CASE_NAMES if n not in ("edges", "nul_first")])
def test_lattices_equal_sample_ref(name):
    """(The 'edges' and 'nul_first' lists are left out: their NUL-holding pieces
    are C-string trie keys under the TrainerModel, which sample_ref.Model does
    not restate.)"""
    pieces, scores = P.cases()[name]
    pieces = [b"<unk>"] + list(pieces)
    scores = np.concatenate([np.float32([0.0]), scores]).astype(np.float32)
    assert float(scores[0]) > float(scores.min())
    tm = P.TrainerModel(pieces, scores)
    rm = R.Model(MB.model([(pieces[0], float(scores[0]), MB.UNKNOWN)] +
                          [(p, float(s), MB.NORMAL) for p, s in zip(pieces[1:], scores[1:])]))
    assert rm.unk_id == tm.unk_id == 0
    assert _bits(rm.unk_score) == _bits(tm.unk_score)
    inputs = pieces[1:][:40] + pieces[1:][-40:] + EXTRA
    assert not any(b"<unk>" in s for s in inputs)
    for s in inputs:
        _same_lattice(tm.lattice(s), rm.lattice(s))


def test_trie_keys_are_c_strings():
    """A NUL ends a key; of keys equal up to the NUL the piece sorting first
    wins (BuildTrie sorts the pieces, darts.h insert() keeps the first)."""
    pieces, scores = P.edge_list()
    tm = P.TrainerModel(pieces, scores)
    assert tm.table[b"ab"][0] == 1          # not 3, "ab\0cd"
    assert tm.table[b"d"][0] == 10          # "d\0"
    nf = P.TrainerModel(*P.nul_first_list())
    assert nf.table[b"ab"][0] == 3          # "ab" sorts before "ab\0cd", listed first
    assert nf.table[b"c"][0] == 5           # "c\0" before "c\0x"
    lat = tm.lattice(b"ab\0cd")
    assert lat.cs == [0, 1, 2, 3, 4, 5]
    assert lat.end_nodes[3] == [(2, tm.unk_score, 0)]   # the NUL position: UNK only


def test_prune_outcomes():
    pieces, scores = [b"a", b"b", b"ab", b"ba", b"c"], np.float32([-1.0, -1.0, -1.5, -3.0, -2.0])
    assert P.prune(pieces, scores, 0)[:2] == (1, [])          # one path
    assert P.prune(pieces, scores, 2)[:2] == (1, [0, 1])      # "ab" beats "a b": kept, alternatives a b
    assert P.prune(pieces, scores, 3)[:2] == (0, [])          # "b a" (-2) beats "ba" (-3)
    # hyps counts the EOS hypothesis: EOS, then c.
    assert P.prune(pieces, scores, 4) == (1, [], 3)
    # An unknown char inside a piece: the alternatives hold the UNK id 0.
    pieces, scores = [b"ab", b"axb", b"b"], np.float32([-1.0, -2.0, -1.5])
    keep, alt, _ = P.prune(pieces, scores, 1)
    assert (keep, alt) == (1, [0, 0, 2])


def test_chars():
    assert [P.chars(p) for p in (b"a", "あ𝄞é".encode(), b"a\xe3", b"ab\0cd")] == [1, 3, 2, 5]


def test_nested_convex_hypothesis_counts():
    """The figures the device tests rest on: the convex scores overflow the
    4096-hypothesis slab on 27 pieces, first on 'a' * 31 with 4160."""
    refs = P.case_refs("nested_a96_convex")[3]
    over = [(k + 1, r[2]) for k, r in enumerate(refs) if r[2] > P.MAX_HYPS]
    assert len(over) == 27 and over[0] == (31, 4160) and max(h for _, h in over) == 16126
    assert P.branches(refs) == (68, 1, 0, 27)


@pytest.mark.parametrize("name,most", [("nested_a96_ties", 1064), ("nested_a96_affine", 1608)])
def test_nested_runs_without_overflow(name, most):
    """(For the affine shape this restatement counts 1608 hypotheses at most,
    with the scores -(3 + 0.37 k) rounded to float32; the figure of 681 first
    reported for it was not reproduced.  Either is far below the slab's 4096.)"""
    refs = P.case_refs(name)[3]
    assert max(r[2] for r in refs) == most <= P.MAX_HYPS
    assert P.branches(refs)[3] == 0


def test_batch_memo_equals_direct_search():
    """prefixed_batch_refs' renamed copies equal a search of their own."""
    bp, bs, model, refs = P.case_refs("batch")
    assert len(bp) == len(refs) == 300 * (P.BATCH_COPIES + 1) > 16384
    for i in list(range(600, len(bp), 977)) + [len(bp) - 1]:
        assert P.prune_string(model, bp[i]) == refs[i]
    b = P.branches(refs)
    assert b[0] > 0 and b[1] > 0 and b[2] > 0
