"""Every BPE encode tier on the GPU against the CPU oracle.

The models of bpe_cases put EncodeBpe on each first kernel (asserted through
spm_hip_model_info.fast_variant, never assumed): bpe_lane_kernel<true> with
merged id = base - rank (1) and from the rank table (2), bpe_lane_kernel<false>
(3) and bpe_half_kernel (4, at 32768 and at 65600 pieces).  The sentences sit
on the kernels' limits; the routing predictor says how many of them must reach
the general kernel.  Ids, piece lengths and token offsets are compared bit for
bit.  Each model and its oracle output are made once per module (the oracle
loads the 32768- and 65600-piece models in well under a second, so both are
compared against the oracle directly)."""
import numpy as np
import pytest

import bpe_cases as C
import oracle_lib as O
import spm_amd as S

pytestmark = pytest.mark.gpu

PLAIN = {
    "affine": (dict(), C.TIER_LANE_AFFINE),
    "table": (dict(order="shuffled"), C.TIER_LANE_TABLE),
    "words": (dict(ties=True), C.TIER_LANE_WORDS),
    "half32768": (dict(pad_to=32768), C.TIER_HALF),
    "half65600": (dict(pad_to=65600), C.TIER_HALF),
}
BASE4 = {k: PLAIN[k] for k in ("affine", "table", "words", "half32768")}


class _Loaded:
    """A model on the device, and the oracle's tokens of every pool sentence."""

    def __init__(self, kw):
        self.spec = C.build_model(**kw)
        self.dm = S.DeviceModel(self.spec.blob)
        self.om = O.OracleModel(self.spec.blob)
        self.want = {}
        self.learn(C.pool())

    def learn(self, sents):
        new = sorted(set(sents) - set(self.want))
        if not new:
            return
        buf, off = O.to_csr(new)
        ids, lens, to = self.om.encode_normalized_csr(buf, off, with_lens=True)
        for k, s in enumerate(new):
            a, b = int(to[k]), int(to[k + 1])
            self.want[s] = (ids[a:b].copy(), lens[a:b].copy())

    def check(self, sents, force_general=False):
        """Encodes the batch on the device, requires the oracle's ids, piece
        lengths and token offsets; returns the call's stats."""
        self.learn(sents)
        self.dm.set_force_general(force_general)
        try:
            buf, off = S.to_csr(sents)
            ids, lens, to = self.dm.encode_csr_host(buf, off, with_lens=True)
            st = self.dm.stats()
        finally:
            self.dm.set_force_general(False)
        want = [self.want[s] for s in sents]
        wto = np.zeros(len(sents) + 1, dtype=np.uint64)
        wto[1:] = np.cumsum([len(w[0]) for w in want], dtype=np.uint64)
        bad = np.nonzero(to != wto)[0]
        assert bad.size == 0, "token offsets differ first after sentence %d: %r" % (bad[0] - 1, sents[bad[0] - 1])
        wids = np.concatenate([w[0] for w in want]) if int(wto[-1]) else np.zeros(0, np.int32)
        wlens = np.concatenate([w[1] for w in want]) if int(wto[-1]) else np.zeros(0, np.uint32)
        for name, got, exp in (("ids", ids, wids), ("piece lengths", lens, wlens)):
            bad = np.nonzero(got != exp)[0]
            if bad.size:
                k = int(np.searchsorted(wto, bad[0], side="right")) - 1
                raise AssertionError("%s differ at token %d (sentence %d: %r): got %d, want %d"
                                     % (name, bad[0], k, sents[k], got[bad[0]], exp[bad[0]]))
        assert st.sentences == len(sents)
        return st


@pytest.fixture(scope="module")
def zoo():
    cache = {}

    def get(**kw):
        key = tuple(sorted(kw.items()))
        if key not in cache:
            cache[key] = _Loaded(kw)
        return cache[key]

    yield get
    cache.clear()


def _tier(m):
    inf = m.dm.info()
    return inf.fast_variant


@pytest.mark.parametrize("name", list(PLAIN))
def test_tier_bit_exact_and_routed(zoo, name):
    """Every batch shape on every tier: bit-exact, and exactly the predicted
    sentences (over 64 bytes and refused by the first kernel) reach the
    general kernel; once more with force_general."""
    kw, tier = PLAIN[name]
    m = zoo(**kw)
    assert _tier(m) == tier
    for arr in C.ARRANGEMENTS:
        for n in C.SIZES:
            sents = C.batch(arr, n)
            st = m.check(sents)
            assert st.general_path == C.flagged_count(sents, tier), (arr, n)
    sents = C.batch("shuffled")
    assert m.check(sents, force_general=True).general_path == len(sents)


def _must_flag(sents, tier, kind):
    """Sentences the first or the fast kernel takes and must flag: a char
    outside an irregular vocabulary, or (a sure case of an UNUSED push) an
    UNUSED two-char piece as the whole sentence."""
    n = 0
    for s in sents:
        if C.route(s, tier) == "general":
            continue
        if kind == "irregular":
            chars = [s[q:q + C.one_char_len(s[q])] for q in C.walk_starts(s)]
            n += any(c == d.encode() for c in chars for d in C.DROPPED)
        else:
            n += any(s == p.encode() for p in C.UNUSED_PIECES if len(p) == 2)
    return n


@pytest.mark.parametrize("kind", ["unused", "irregular"])
@pytest.mark.parametrize("name", list(BASE4))
def test_unused_and_irregular_models(zoo, name, kind):
    """UNUSED pieces (flag, then the general kernel's resegmentation) and
    irregular vocabularies (a char outside the vocabulary flags) on every
    tier: bit-exact, and at least the predicted sentences flagged."""
    kw, tier = BASE4[name]
    m = zoo(**kw, **{kind: True})
    assert _tier(m) == tier
    for arr in C.ARRANGEMENTS:
        for n in C.SIZES:
            sents = C.batch(arr, n)
            st = m.check(sents)
            assert st.general_path >= C.flagged_count(sents, tier) + _must_flag(sents, tier, kind), (arr, n)
    whole = C.batch("shuffled")
    assert _must_flag(whole, tier, kind) > 0
    m.check(whole, force_general=True)


@pytest.mark.parametrize("reserved_top", [False, True])
def test_lane_ids_up_to_32766(zoo, reserved_top):
    """32767 pieces with the live ids on top: the lane kernel's int16 symbols
    hold ids up to 32766; with reserved_top the CONTROL piece "z" (id 32766,
    outside pieces_) travels as ~PieceToId."""
    m = zoo(pad_to=32767, reserved_top=reserved_top)
    assert _tier(m) == C.TIER_LANE_AFFINE
    if reserved_top:
        assert m.spec.id_of["z"] == 32766
        assert m.want[b"azbzzc"][0].tolist().count(32766) == 3
    for arr in C.ARRANGEMENTS:
        for n in (127, 129, None):
            sents = C.batch(arr, n)
            assert m.check(sents).general_path == C.flagged_count(sents, C.TIER_LANE_AFFINE)
    m.check(C.batch("shuffled"), force_general=True)


def _half_eligible():
    return [s for s in C.pool() if C.route(s, C.TIER_HALF) == "first"]


@pytest.mark.parametrize("vocab", [32768, 65600])
@pytest.mark.parametrize("n", [1, 3, 5, 129, 255])
def test_half_kernel_odd_batches(zoo, vocab, n):
    """Odd n and n = 1: the last wave's second half has no sentence.  Every
    sentence here is one the half kernel takes, the longest ones last."""
    m = zoo(pad_to=vocab)
    assert _tier(m) == C.TIER_HALF
    sents = sorted(_half_eligible(), key=len)[-n:]
    assert len(sents) == n and len(sents[-1]) > 64
    assert m.check(sents).general_path == 0


def test_half_kernel_mixed_pairs(zoo):
    """The two halves of a wave hold sentences of different kinds, in both
    orders: eligible + refused (to the fast kernel, and to the general one),
    eligible + flagged by an UNUSED push, empty + long."""
    m, mu = zoo(pad_to=32768), zoo(pad_to=32768, unused=True)
    assert _tier(m) == _tier(mu) == C.TIER_HALF
    lim = {k: v[0] for k, v in C.limits().items()}
    elig, refused_fast, refused_gen, long_ = lim["four32"], lim["ascii33"], lim["ascii65"], lim["bytes256"]
    unused2 = next(p for p in C.UNUSED_PIECES if len(p) == 2).encode()
    H = C.TIER_HALF
    assert [C.route(s, H) for s in (elig, refused_fast, refused_gen, long_, unused2, b"")] == \
        ["first", "fast", "general", "general", "first", "first"]
    for a, b, flagged in ((elig, refused_fast, 0), (elig, refused_gen, 1), (b"", long_, 1), (b"", b"", 0),
                          (elig, b"", 0)):
        for pair in ((a, b), (b, a)):
            assert m.check(list(pair)).general_path == flagged, pair
            assert m.check(list(pair) * 3 + [pair[0]]).general_path == 3 * flagged + (pair[0] in (refused_gen, long_))
    for pair in ((elig, unused2), (unused2, elig), (unused2, unused2), (unused2, b""), (b"", unused2)):
        st = mu.check(list(pair))
        assert st.general_path == pair.count(unused2), pair
        # (without UNUSED pieces the same sentence stays on the half kernel)
        assert m.check(list(pair)).general_path == 0


def test_padding_changes_only_the_ids(zoo):
    """Across tiers without the oracle: the mini model (lane kernel) and its
    paddings to 32767 (lane kernel), 32768 and 65600 pieces (half kernel)
    must cut the whole pool into pieces of identical lengths, and ids that
    differ by the mini pieces' constant shift."""
    sents = C.batch("shuffled")
    buf, off = S.to_csr(sents)
    out = {}
    for v in (None, 32767, 32768, 65600):
        m = zoo(pad_to=v) if v else zoo()
        assert _tier(m) == (C.TIER_HALF if v and v >= 32768 else C.TIER_LANE_AFFINE)
        out[v] = m.dm.encode_csr_host(buf, off, with_lens=True)
    ids0, lens0, to0 = out[None]
    mini_size = len(zoo().spec)
    for v in (32767, 32768, 65600):
        ids, lens, to = out[v]
        assert np.array_equal(to, to0) and np.array_equal(lens, lens0), v
        moved = ids0 >= 3  # <unk> stays (or becomes one of the listed fillers)
        assert np.array_equal(ids[moved], ids0[moved] + (v - mini_size)), v
        assert np.all(ids[~moved] < v - mini_size)
