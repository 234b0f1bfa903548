"""BPE encode tiers without a GPU: every model variant of bpe_cases reports the
tier it was built for (spm_hip_model_info.fast_variant on host-only handles),
and the sentence generators meet their own conditions under the oracle."""
import numpy as np
import pytest

import bpe_cases as C
import oracle_lib as O
import spm_amd as S


def _tier(**kw):
    spec = C.build_model(**kw)
    inf = S.DeviceModel(spec.blob, host_only=True).info()
    assert inf.piece_size == len(spec)
    assert inf.ring_width == 0
    return inf.fast_variant


@pytest.mark.parametrize("extra", [{}, {"unused": True}, {"irregular": True}], ids=["plain", "unused", "irregular"])
@pytest.mark.parametrize("kw,tier", [
    ({}, C.TIER_LANE_AFFINE),
    ({"order": "shuffled"}, C.TIER_LANE_TABLE),
    ({"ties": True}, C.TIER_LANE_WORDS),
    ({"pad_to": 32768}, C.TIER_HALF),
], ids=["affine", "table", "words", "half"])
def test_variant_reports_its_tier(kw, tier, extra):
    assert _tier(**kw, **extra) == tier


def test_tier_by_vocabulary_size():
    """32767 pieces is the lane kernel's last size (ids are int16 there);
    32768 and 65600 take the half kernel; a USER_DEFINED piece leaves the
    general kernel only, whatever the size."""
    assert _tier(pad_to=32767) == C.TIER_LANE_AFFINE
    assert _tier(pad_to=32767, reserved_top=True) == C.TIER_LANE_AFFINE
    assert _tier(pad_to=32767, order="shuffled") == C.TIER_LANE_TABLE
    assert _tier(pad_to=32768) == C.TIER_HALF
    assert _tier(pad_to=32768, reserved_top=True) == C.TIER_HALF
    assert _tier(pad_to=65600) == C.TIER_HALF
    assert _tier(user_defined=True) == C.TIER_GENERAL
    assert _tier(user_defined=True, pad_to=32768) == C.TIER_GENERAL


def test_model_shape():
    spec = C.build_model()
    assert len(C.ALPHABET) == 23 and len(C.MERGES) == C.N_MERGES
    assert all(c in spec.id_of for c in C.ALPHABET)  # every char is a piece
    assert all(len(p) == 2 for p in C.MERGES[:C.N_CHAR_MERGES])
    assert {"aa", "bb", "aaaa"} <= set(C.MERGES)
    assert max(len(p) for p in C.MERGES) == C.MAX_PIECE_CHARS
    assert 0.03 * C.N_MERGES <= len(C.UNUSED_PIECES) <= 0.08 * C.N_MERGES
    assert any(len(p) == 2 for p in C.UNUSED_PIECES)
    # Dropped chars stay inside merged pieces (what makes a model irregular).
    irr = C.build_model(irregular=True)
    for c in C.DROPPED:
        assert c not in irr.id_of and any(c in p for p in C.MERGES)
    top = C.build_model(pad_to=32767, reserved_top=True)
    assert top.id_of["z"] == 32766 and top.pieces[-1][2] == C.CONTROL
    big = C.build_model(pad_to=65600)
    assert min(big.id_of[p] for p in C.MERGES + C.ALPHABET) == 65600 - C.N_MERGES - 23
    # The live ids straddle 16 bits: every char and the last merges lie past 65535.
    assert min(big.id_of[c] for c in C.ALPHABET) > 65535 > big.id_of[C.MERGES[0]]
    sents = b"".join(C.pool()).decode(errors="ignore")
    fillers = [p for p, _, _ in big.pieces[3:65600 - C.N_MERGES - 23]]
    assert sorted(c for c in fillers if c in sents) == sorted(C.LISTED_FILLERS)
    assert all(p[1] < -float(C.N_MERGES + 23) for p in big.pieces[3:65600 - C.N_MERGES - 23])


def test_limit_sentences_are_what_their_names_say():
    lim = C.limits()
    for name, (s, nb, nc) in lim.items():
        assert (len(s), C.n_chars(s)) == (nb, nc), name
    sizes = {(nb, nc) for _, nb, nc in lim.values()}
    for want in [(128, 32), (129, 36), (33, 33), (34, 34), (35, 35), (64, 64), (65, 65), (65, 64)]:
        assert want in sizes
    assert {255, 256} <= {nb for nb, _ in sizes}
    assert all((k, k) in sizes for k in range(2, 41))
    p = C.pool()
    assert p[0] == b"" and p[-1] == b"" and any(a == b"" and b == b"" for a, b in zip(p[1:-1], p[2:-1]))
    assert 950 <= len(p) <= 1200


def test_edge_sentences_match_the_parity_suite():
    import test_gpu_parity
    assert C.edge_sentences() == test_gpu_parity._edge_sentences()


@pytest.mark.parametrize("tier", [C.TIER_LANE_AFFINE, C.TIER_LANE_TABLE, C.TIER_LANE_WORDS, C.TIER_HALF])
def test_every_routing_class_is_populated(tier):
    p = C.pool()
    routes = [C.route(s, tier) for s in p]
    for cls in ("first", "fast", "general"):
        assert routes.count(cls) >= 20, cls
    # ... and in the batch shapes: the refused tile holds no first-kernel sentence.
    tile = C.batch("refused_tile", C.TILE)
    assert len(tile) == C.TILE and all(C.route(s, tier) != "first" for s in tile)
    assert {C.route(s, tier) for s in tile} == {"fast", "general"}


def test_routing_predictor_on_the_limits():
    lim = {k: v[0] for k, v in C.limits().items()}
    lane, half = C.TIER_LANE_AFFINE, C.TIER_HALF
    want = {  # name: (lane tier, half tier)
        "four32": ("first", "first"), "four31_ascii5": ("general", "general"),
        "ascii32": ("first", "first"), "ascii33": ("first", "fast"), "ascii34": ("first", "fast"),
        "ascii35": ("fast", "fast"), "ascii64": ("fast", "fast"), "ascii65": ("general", "general"),
        "ascii63_two1": ("general", "general"), "two32": ("first", "first"), "two33": ("first", "general"),
        "three34": ("first", "general"), "three35": ("general", "general"),
        "bytes255": ("general", "general"), "bytes256": ("general", "general"),
    }
    for name, (wl, wh) in want.items():
        assert (C.route(lim[name], lane), C.route(lim[name], half)) == (wl, wh), name
    # The half kernel's consistency rule: a split by non-continuation bytes
    # that differs from the OneCharLen walk is refused.
    for s in (b"abc\xc3", b"\xe3\x81", b"\xf8", b"a"):
        assert C.route(s, half) == "first", s  # both splits agree (a cut char is one char in both)
    for s in (b"\x80abc", b"\xc3abc", b"a\xe3bc", b"ab\x80\x80cd", "é".encode() + b"\x80\x80"):
        assert C.route(s, half) == "fast", s
        assert C.route(s, lane) == "first", s


def test_batch_shapes():
    whole = len(C.pool())
    for arr in C.ARRANGEMENTS:
        for n in C.SIZES:
            assert len(C.batch(arr, n)) == (n or whole)
    assert sorted(C.batch("refused_tile")) == sorted(C.batch("shuffled")) == sorted(C.pool())
    for n in C.SIZES:
        b = C.batch("short_last", n)
        assert len(b[-1]) <= 4 and sum(len(s) for s in b) % 4 != 0


def test_generators_under_the_oracle():
    """Merges really happen on the sweep (tokens per char <= 0.6), and padding
    the vocabulary changes nothing but the ids: the mini model and its
    32768-piece padding give identical piece lengths on the whole pool, and
    ids that differ by the constant shift of the mini pieces."""
    mini, big = C.build_model(), C.build_model(pad_to=32768)
    om, ob = O.OracleModel(mini.blob), O.OracleModel(big.blob)
    sw = C.sweep()
    assert len(sw) == 71 * 12
    assert 0.4 <= sum(len(s) > C.FAST_BYTES for s in sw) / len(sw) <= 0.6
    buf, off = O.to_csr(sw)
    ids, to = om.encode_normalized_csr(buf, off)
    assert len(ids) / sum(C.n_chars(s) for s in sw) <= 0.6
    p = C.pool()
    buf, off = O.to_csr(p)
    mi, ml, mt = om.encode_normalized_csr(buf, off, with_lens=True)
    bi, bl, bt = ob.encode_normalized_csr(buf, off, with_lens=True)
    assert np.array_equal(mt, bt) and np.array_equal(ml, bl)
    shift = 32768 - len(mini)
    assert all(big.id_of[q] - mini.id_of[q] == shift for q, _, t in mini.pieces[3:])
    # Mini pieces shift; <unk> stays, except on the three listed fillers,
    # which the padded model knows.
    listed = {big.id_of[c] for c in C.LISTED_FILLERS}
    moved = mi >= 3
    assert np.array_equal(bi[moved], mi[moved] + shift)
    assert set(bi[~moved].tolist()) <= {0} | listed and listed <= set(bi[~moved].tolist())
    assert np.all(mi[~moved] == 0)
