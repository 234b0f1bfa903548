"""GPU: the pruning step's two device pieces against the restatement
(tests/prune_ref.py), bit for bit.

* spm_hip_prune_nbest (prune_nbest_kernel): per piece, keep == 2 exactly when
  the restatement's search allocates more than 4096 hypotheses, else keep and
  the alternatives equal the restatement's;
* spm_hip_model_from_pieces: the Viterbi ids and piece lengths of the model
  the pruning step encodes the corpus with equal nbest_ref.nbest(TrainerModel,
  s, 1), through the fast kernels and again through the general kernel.
"""
import contextlib

import numpy as np
import pytest

import nbest_ref as NB
import prune_ref as P
import spm_amd as S

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _closing(*handles):
    """Device handles released when the test ends, a failing one included."""
    try:
        yield handles[0] if len(handles) == 1 else handles
    finally:
        for h in handles:
            h.close()


def _check_prune(got, refs, pieces):
    keep, alts = got
    assert len(keep) == len(alts) == len(refs)
    for i, ref in enumerate(refs):
        want_keep, want_alt = P.expect_device(ref)
        assert (int(keep[i]), alts[i]) == (want_keep, want_alt), (i, pieces[i], ref)


@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_prune_nbest_matches_restatement(name):
    pieces, scores, _, refs = P.case_refs(name)
    with _closing(S.DevicePieces(pieces, scores)) as dp:
        _check_prune(dp.prune_nbest(), refs, pieces)


def test_nested_runs_take_every_branch():
    """The convex scores overflow the slab on 27 of the 96 pieces ('a' * 31
    by 64 hypotheses) and not on the other 69; ties and affine scores overflow
    nowhere, and reach kept pieces with alternatives."""
    b = P.branches(P.case_refs("nested_a96_convex")[3])
    assert b[3] == 27 and b[0] > 0 and b[1] > 0
    assert P.case_refs("nested_a96_convex")[3][30][2] == P.MAX_HYPS + 64
    for name in ("nested_a96_ties", "nested_a96_affine"):
        b = P.branches(P.case_refs(name)[3])
        assert b[3] == 0 and b[2] > 0


def test_random_list_takes_three_branches():
    b = P.branches(P.case_refs("random")[3])
    assert b[0] > 0 and b[1] > 0 and b[2] > 0 and b[3] == 0


def test_unk_id_in_alternatives():
    """UNK nodes carry id 0: in the alternatives of pieces with a char that is
    no piece, and next to a real piece 0 in the collision list."""
    pieces, _, _, refs = P.case_refs("unk")
    assert any(0 in alt for _, alt, _ in refs)
    pieces, _, _, refs = P.case_refs("collision")
    assert pieces[0] == b"a"
    assert refs[pieces.index(b"za")][:2] == (1, [0, 0])   # UNK, then the real piece 0


def test_grid_stride_batch():
    """More pieces than lanes (16500 > 16384): the first lanes take a second
    piece on a reused slab."""
    pieces, scores, _, refs = P.case_refs("batch")
    assert len(pieces) > 16384
    with _closing(S.DevicePieces(pieces, scores)) as dp:
        _check_prune(dp.prune_nbest(), refs, pieces)


def test_set_scores_then_prune_nbest():
    """What the trainer does when the M-step kept every piece: new scores into
    the last E-step's piece set, then the search.  Equal to a fresh set's."""
    pieces, scores, _, refs = P.case_refs("random")
    other = np.roll(scores, 7) - np.float32(0.25)
    other_refs = P.prune_all(pieces, other)
    assert sum(a[:2] != b[:2] for a, b in zip(refs, other_refs)) > 100   # the scores matter
    with _closing(S.DevicePieces(pieces, other), S.DevicePieces(pieces, scores)) as (dp, fresh):
        _check_prune(dp.prune_nbest(), other_refs, pieces)
        dp.set_scores(scores)
        got = dp.prune_nbest()
        _check_prune(got, refs, pieces)
        want = fresh.prune_nbest()
        assert np.array_equal(got[0], want[0]) and got[1] == want[1]
    # Nested runs: the new scores change which pieces overflow.
    pieces, ties, _, _ = P.case_refs("nested_a96_ties")
    _, convex, _, refs = P.case_refs("nested_a96_convex")
    with _closing(S.DevicePieces(pieces, ties)) as dp2:
        dp2.set_scores(convex)
        _check_prune(dp2.prune_nbest(), refs, pieces)


@pytest.mark.parametrize("value,limit", [("1", 2), ("2", 2), ("6", 6), ("7", 7), ("163", 163), ("1063", 1063),
                                         ("1064", 1064), ("5000", 4096)])
def test_max_hyps_knob(value, limit, monkeypatch):
    """SPM_HIP_PRUNE_MAX_HYPS, clamped to [2, 4096]: a piece is flagged exactly
    when its search allocates more hypotheses than the limit.  Over the tied
    runs (3 to 1064 hypotheses; 163 is 'a' * 16's count) and the collision
    list (3, 6, 9 and 11): limits on both sides of a piece's exact count."""
    monkeypatch.setenv("SPM_HIP_PRUNE_MAX_HYPS", value)
    flagged = 0
    for name in ("nested_a96_ties", "collision"):
        pieces, scores, _, refs = P.case_refs(name)
        with _closing(S.DevicePieces(pieces, scores)) as dp:
            keep, alts = dp.prune_nbest()
        for i, ref in enumerate(refs):
            assert (int(keep[i]), alts[i]) == P.expect_device(ref, limit), (i, pieces[i], ref)
        flagged += sum(r[2] > limit for r in refs)
    hyps = sorted(r[2] for n in ("nested_a96_ties", "collision") for r in P.case_refs(n)[3])
    assert hyps[0] == 3 and hyps[-1] == 1064 and 163 in hyps and 6 in hyps
    assert (flagged == 0) == (limit >= 1064)
    if limit == 2:
        assert flagged == len(hyps)


# ---- spm_hip_model_from_pieces ---------------------------------------------
def _sentences(pieces, count=80):
    """Up to `count` of the pieces themselves, joins of neighbours, and
    sentences with chars no list holds: U+2585 (the trainer's rare-char
    stand-in), '?' and U+4E00."""
    ps = [p for p in pieces if p]
    step = max(1, (len(ps) + count - 1) // count)
    some = ps[::step][:count]
    out = list(some)
    out += [a + b for a, b in zip(some, some[1:])]
    out += [a + "▅".encode() + b for a, b in zip(some[::3], some[1::3])]
    out += ["▅".encode(), b"?" + some[0], some[-1] + "一▅?".encode(), "▅▅".encode() + some[0] + "▅".encode()]
    out += [b"".join(some[:12]), b"".join(some[::-1][:25])]
    seen, uniq = set(), []
    for s in out:
        if s not in seen:
            seen.add(s)
            uniq.append(s)
    return uniq


def _want_viterbi(model, sents):
    ids, lens, tok = [], [], [0]
    for s in sents:
        (pi, pl, _), = NB.nbest(model, s, 1)[0]
        ids += pi
        lens += pl
        tok.append(len(ids))
    return ids, lens, tok


@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_from_pieces_viterbi(name):
    pieces, scores, model, _ = P.case_refs(name)
    # (the 96-char runs: fewer sentences, the restatement's Viterbi is Python)
    sents = _sentences(pieces, 6 if name.startswith("nested_a96") else 80)
    want_ids, want_lens, want_tok = _want_viterbi(model, sents)
    if name in ("unk", "collision"):
        assert 0 in want_ids
    buf, off = S.to_csr(sents)
    with _closing(S.DeviceModel.from_pieces(pieces, scores)) as dm:
        for general in (False, True):
            dm.set_force_general(general)
            ids, lens, tok = dm.encode_csr_host(buf, off, with_lens=True)
            assert tok.tolist() == want_tok, general
            for i in range(len(sents)):
                a, b = want_tok[i], want_tok[i + 1]
                assert (ids[a:b].tolist(), lens[a:b].tolist()) == (want_ids[a:b], want_lens[a:b]), \
                    (general, sents[i])


def test_from_pieces_kernel_tiers():
    """The boundary lists sit on both sides of the byte kernel's 16-byte ring
    and of the 64-byte ring: 15/16/17-byte pieces leave the byte kernel, 65
    bytes leave the fast kernels altogether."""
    with _closing(*(S.DeviceModel.from_pieces(*P.case_refs(n)[:2])
                    for n in ("collision", "boundary_16", "boundary_64"))) as (small, b16, b64):
        assert small.info().fast_variant == 1
        assert b16.info().fast_variant != 1
        assert b64.info().fast_variant == 0
