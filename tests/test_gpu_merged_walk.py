"""Byte kernel deep walk (unigram_fast_kernel<16, true>): past the shallow
depths a lane carries one trie chain of its position pair, and the lanes whose
two chains are both deep run the second one in a pass of its own.  Ids, piece
lengths and offsets bit-for-bit against the oracle.

The inputs are built from what such a walk can get wrong: a lane with two deep
chains (either one winning), waves that mix the roles, walks that die at every
depth with and without a leaf behind them, setters of one ring slot that come
from the two chains of one lane an ulp (or nothing) apart, "▁" words next to
continuation bytes, and two corpora.  Everything is placed at position phases
0..3, so chains sit in both pairs of a group and across the pair boundary.
None of this depends on how the walk is scheduled: the two-chain walk passes
the same file.  Batches go through the device-pointer API, hold at most 400
sentences and end with a sentence longer than 64 bytes.
"""
import os

import numpy as np
import pytest

import oracle_lib as O
import spm_amd as S
import synth
from model_builder import NORMAL, UNIGRAM, base_pieces, model
from test_gpu_piece_table import _encode_device, _near_tie_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

f32 = np.float32
WS = "▁".encode()
L16 = "abcdefghijklmnop"
U16 = L16.upper()
LONG_LAST = b"q" + b"abcdefgh" * 9  # > 64 bytes


def _check(mb, sents, long_last=LONG_LAST):
    """Encodes sents (+ a long last sentence) with the byte kernel and with
    the oracle, asserts ids, piece lengths and offsets equal; returns (stats,
    oracle ids, oracle lens, oracle offsets)."""
    sents = list(sents) + ([long_last] if long_last is not None else [])
    assert len(sents) <= 400 and len(sents[-1]) > 64
    buf, off = S.to_csr(sents)
    oids, olens, oto = O.OracleModel(mb).encode_normalized_csr(buf, off, with_lens=True)
    dm = S.DeviceModel(mb)
    assert dm.info().fast_variant == 1
    ids, lens, to = _encode_device(dm, buf, off)
    st = dm.stats()
    dm.close()
    assert np.array_equal(to, oto), "token counts differ"
    bad = np.nonzero(ids != oids)[0]
    assert bad.size == 0, "first id mismatch at token %d" % bad[0]
    assert np.array_equal(lens, olens)
    assert st.general_path < len(sents)  # the fast kernel wrote tokens itself
    return st, oids, olens, oto


def _tokens(i, olens, oto):
    return olens[int(oto[i]):int(oto[i + 1])].tolist()


def _singles(chars, base=-4.0):
    return [(c, base - 0.0625 * i, NORMAL) for i, c in enumerate(chars)]


# ---- 1. two deep chains in one lane ---------------------------------------

def _two_chain_model():
    """Lower case: the piece from p beats "a" + the piece from p + 1; upper
    case: the piece from p + 1 wins.  12- and 15-byte pieces of both."""
    p = base_pieces() + [("q", -3.0, NORMAL)] + _singles(L16) + _singles(U16, -5.5)
    p += [(L16[0:12], -1.0, NORMAL), (L16[1:13], -3.0, NORMAL)]
    p += [(L16[0:15], -1.25, NORMAL), (L16[1:16], -3.25, NORMAL)]
    p += [(U16[0:12], -3.0, NORMAL), (U16[1:13], -1.0, NORMAL)]
    p += [(U16[0:15], -3.25, NORMAL), (U16[1:16], -1.25, NORMAL)]
    return p


def test_two_deep_chains_in_one_lane():
    words = [L16[:13], L16[:16], U16[:13], U16[:16]]
    sents = []
    for w in words:
        for phase in range(4):
            sents += [("q" * phase + w).encode(), ("q" * phase + w + "q").encode(), ("q" * phase + w + w).encode()]
    st, oids, olens, oto = _check(model(_two_chain_model(), UNIGRAM), sents)
    for i, s in enumerate(sents):
        phase = len(s) - len(s.lstrip(b"q"))
        toks = _tokens(i, olens, oto)[phase:]
        n = 12 if len(s.strip(b"q")) % 13 == 0 else 15
        # the chain-0 piece then one char, or one char then the chain-1 piece
        assert toks[:2] == ([n, 1] if s[phase:phase + 1] == b"a" else [1, n]), (s, toks)
    assert st.general_path == 0


# ---- 2. a wave that mixes the roles ---------------------------------------

def _mixed_model():
    """X_n = "abc.."[:n] and Y_n = "bcd.."[:n], n = 5..15.  A word "abc.."[:n
    + 1] at an even position walks X and Y in one lane (two deep chains), at
    an odd position in two; a word "bcd.."[:n] alone is chain 0 at an even and
    chain 1 at an odd position."""
    p = base_pieces() + [("q", -3.0, NORMAL)] + _singles(L16)
    p += [("ab", -3.5, NORMAL), ("abc", -3.25, NORMAL)]
    for n in range(5, 16):
        # odd n: "a" + Y_n beats X_(n+1) (and X_n + a char); even n: X_(n+1) wins
        p.append((L16[:n], (-1.0 if n % 2 else -6.0) - 0.015625 * n, NORMAL))
        p.append((L16[1:1 + n], (-0.25 if n % 2 else -2.0) - 0.015625 * n, NORMAL))
    return p


def _mixed_sentences():
    words = [L16[:n + 1] for n in range(5, 16)] + [L16[1:1 + n] for n in range(5, 16)] + ["abc", "b", "qq"]
    slots = [(w, ph) for w in words for ph in range(4)]
    sents = []
    for i, (w, ph) in enumerate(slots):
        w2, ph2 = slots[(7 * i + 3) % len(slots)]
        s = ("q" * ph + w).ljust(22, "q") + ("q" * ph2 + w2).ljust(22, "q")
        sents.append(s.encode())
    return sents


def test_mixed_wave():
    sents = _mixed_sentences()
    assert len(sents) >= 64 and {len(s) for s in sents} == {44}  # one length: the sort keeps them together
    pieces = _mixed_model()
    st, oids, olens, oto = _check(model(pieces, UNIGRAM), sents)
    assert set(range(5, 16)) <= set(olens.tolist())
    assert st.general_path == 0
    # The roles are what the construction claims.  A walk from position b is
    # chain b & 1 of the pair (b & ~1, b | 1); it is deep if it matches >= 5
    # bytes, and its lane has two deep chains if the pair's other walk is deep
    # too.  Per role, the piece lengths the walk passes as leaves, and the
    # lengths of the oracle's tokens that begin there.
    leaves = {p[0].encode() for p in pieces[3:]}
    prefixes = {w[:n] for w in leaves for n in range(1, len(w) + 1)}

    def walk(s, b):  # (bytes matched, lengths of the leaves passed)
        n, found = 0, []
        while n < 15 and b + n < len(s) and s[b:b + n + 1] in prefixes:
            n += 1
            if s[b:b + n] in leaves:
                found.append(n)
        return n, found

    roles = ("chain 0 only", "chain 1 only", "two chains, chain 0", "two chains, chain 1")
    walked = {r: set() for r in roles}
    won = {r: set() for r in roles}
    for i, s in enumerate(sents):
        role_at = {}
        for b in range(len(s)):
            n, found = walk(s, b)
            if n < 5:
                continue
            two = walk(s, b ^ 1)[0] >= 5
            role_at[b] = roles[(2 if two else 0) + (b & 1)]
            walked[role_at[b]].update(x for x in found if x >= 5)
        b = 0
        for t in _tokens(i, olens, oto):
            if t >= 5:
                won[role_at[b]].add(t)
            b += t
    print("mixed wave, token lengths per role:", {r: sorted(v) for r, v in won.items()})
    for r in roles:
        assert walked[r] == set(range(5, 16)), (r, sorted(walked[r]))
        assert len(won[r]) >= 5, r  # and each role decides tokens of the result


# ---- 3. walks that die at every depth --------------------------------------

def test_walks_through_inner_nodes():
    """Only the 15-byte pieces (from "a" and from "b") are leaves: a walk is
    alive to depth k through inner nodes, then meets another byte (k = 3..14)
    or the sentence end (k = 3..14, the depths around every merge depth)."""
    p = base_pieces() + [("q", -3.0, NORMAL)] + _singles(L16) + [(L16[:15], -1.0, NORMAL), (L16[1:16], -1.5, NORMAL)]
    sents, leafless = [], []
    for k in range(3, 15):
        for w in (L16[:k], L16[1:1 + k]):
            for phase in range(4):
                sents += [("q" * phase + w).encode(), ("q" * phase + w + "q").encode(),
                          ("q" * phase + w + "q" + L16).encode()]
                leafless += [True, True, False]
    st, oids, olens, oto = _check(model(p, UNIGRAM), sents)
    for i, s in enumerate(sents):
        if leafless[i]:
            assert set(_tokens(i, olens, oto)) == {1}, s
        else:
            assert 15 in _tokens(i, olens, oto), s
    assert st.general_path == 0


# ---- 4. ties and near ties --------------------------------------------------

FAMILIES = ["abcdefghijkl", "ABCDEFGHIJKL", "0123456789:;", "mnoprstuvwxy", "MNOPRSTUVWXY", "!#$%&()*+,-.",
            "abcdefghijkL", "abcdefghiJKL"]


def _tie_pieces():
    """Setters of one end position from a deep walk, an ulp or nothing apart.
    The filler "q" scores 0 and every score is a small dyadic number, so the
    sums are exact at every phase.  Per family f (12 bytes), in insert order:
      0  f (begin 0) == f[0] + f[1:] (begin 1): the two chains of one lane,
         exactly equal, the earlier begin wins
      1  f one ulp below f[0] + f[1:]: the chain-1 node wins by an ulp
      2  f one ulp above: the chain-1 node loses by an ulp
      3  f (deep) one ulp below f[:9] + f[9:] (a shallow node of a later pair)
      4  the same, exactly equal
      5  f one ulp below f[0] + f[1:], which is one ulp below f[:2] + f[2:]:
         three setters from chain 0, chain 1 and the next pair's chain 0
      6  f[:11] + f[11] (shallow, begin 11) against f (deep, begin 0) where
         the walk shares its first 11 bytes with family 0: near, later wins
      7  15 bytes: f + "XYZ" tied with f[0] + (f + "XYZ")[1:] (slot 18 at
         phase 2), and 14 bytes an ulp apart
    """
    up = lambda v: float(np.nextafter(f32(v), f32(np.inf)))
    dn = lambda v: float(np.nextafter(f32(v), f32(-np.inf)))
    p = base_pieces() + [("q", 0.0, NORMAL), ("z", -2.0, NORMAL), ("zz", -16.0, NORMAL)]
    heads = set()
    for f in FAMILIES:
        heads.add(f[0])
    # family heads score -1, every other char -32 (far below any tie)
    seen = {"q", "z"}
    for f in FAMILIES:
        for c in f:
            if c not in seen:
                seen.add(c)
                p.append((c, -1.0 if c in heads else -4.0 if c == "L" else -32.0, NORMAL))
    f0, f1, f2, f3, f4, f5, f6, f7 = FAMILIES
    p += [(f0, -9.0, NORMAL), (f0[1:], -8.0, NORMAL)]
    p += [(f1, dn(-9.0), NORMAL), (f1[1:], -8.0, NORMAL)]
    p += [(f2, up(-9.0), NORMAL), (f2[1:], -8.0, NORMAL)]
    p += [(f3, dn(-9.0), NORMAL), (f3[:9], -6.0, NORMAL), (f3[9:], -3.0, NORMAL)]
    p += [(f4, -9.0, NORMAL), (f4[:9], -6.0, NORMAL), (f4[9:], -3.0, NORMAL)]
    p += [(f5, dn(dn(-9.0)), NORMAL), (f5[1:], dn(-8.0), NORMAL), (f5[:2], -2.0, NORMAL), (f5[2:], -7.0, NORMAL)]
    # f6 = family 0 with another last byte: f6[:11] is an inner node of f0's walk
    p += [(f6, dn(-9.0), NORMAL), (f6[:11], -5.0, NORMAL)]  # "L" scores -4
    # 15 bytes: f7 + "XYZ"
    w15 = f7 + "XYZ"
    p += [(w15, -9.0, NORMAL), (w15[1:], -8.0, NORMAL), ("X", -32.0, NORMAL), ("Y", -32.0, NORMAL), ("Z", -32.0, NORMAL)]
    p += [(w15[:14], dn(-7.0), NORMAL), (w15[1:14], -6.0, NORMAL)]
    # drop duplicate single chars (a later family repeats an earlier one's letters)
    out, names = [], set()
    for q in p:
        if q[0] not in names:
            names.add(q[0])
            out.append(q)
    return out


def test_ties_decided_by_a_deep_insert():
    words = FAMILIES[:7] + [FAMILIES[7] + "XYZ", FAMILIES[7] + "XY"]
    sents = []
    for w in words:
        for tail in ("", "z", "zz", "q" + w):
            for phase in range(4):
                sents.append(("q" * phase + w + tail).encode())
    st, oids, olens, oto = _check(model(_tie_pieces(), UNIGRAM), sents)
    # What the cases claim (phase 0, no tail): first setter on an exact tie, the later one an ulp above.
    first = {w: _tokens(16 * k, olens, oto) for k, w in enumerate(words)}
    assert first[FAMILIES[0]] == [12]
    assert first[FAMILIES[1]] == [1, 11]
    assert first[FAMILIES[2]] == [12]
    assert first[FAMILIES[3]] == [9, 3]
    assert first[FAMILIES[4]] == [12]
    assert first[FAMILIES[5]] == [2, 10]
    assert first[FAMILIES[6]] == [11, 1]
    assert first[FAMILIES[7] + "XYZ"] == [15]
    assert first[FAMILIES[7] + "XY"] == [1, 13]
    print("deep ties: general_path", int(st.general_path), "of", len(sents) + 1)
    # Family 5 is an exact 3-deep chain at every phase and tail (16 sentences),
    # which the fast kernel hands over; nothing else here is.
    assert st.general_path == 16


def _near_tie_long_case():
    """The near-tie stress construction (every multi-char piece one ulp below,
    or equal to, the sum of its first char and the rest) with words of 2..11
    bytes, so that most near pairs are set by deep inserts; sentences are runs
    of vocabulary words."""
    rng = np.random.default_rng(11)
    alpha = "abcdef"
    sc = {"▁": f32(-1.0)}
    for c in alpha:
        sc[c] = f32(-rng.uniform(1.0, 3.0))
    by_len = {1: list(alpha)}
    for L in range(2, 12):
        by_len[L] = []
        for _ in range(40):
            rest = by_len[L - 1][int(rng.integers(0, len(by_len[L - 1])))]
            w = alpha[int(rng.integers(0, len(alpha)))] + rest
            if w in sc:
                continue
            tot = f32(sc[w[0]] + sc[rest])
            sc[w] = np.nextafter(tot, f32(-np.inf)) if rng.random() < 0.7 else tot
            by_len[L].append(w)
    mb = model(base_pieces() + [(w, float(v), NORMAL) for w, v in sc.items()], UNIGRAM)
    vocab = [w for L in range(1, 12) for w in by_len[L]]
    sents = []
    for _ in range(299):
        k = int(rng.integers(0, 5))
        sents.append(("▁" + "".join(vocab[int(x)] for x in rng.integers(0, len(vocab), k))).encode())
    sents.append("▁".encode() + b"abcdef" * 12)
    return mb, sents


def test_near_tie_stress_long_words():
    mb, sents = _near_tie_long_case()
    assert max(len(s) for s in sents[:-1]) > 20
    st, _, _, _ = _check(mb, sents, long_last=None)
    print("near-tie stress, long words: general_path", int(st.general_path), "of", len(sents))
    # 233 on the two-chain walk (measured on the kernel before the merged deep
    # phase, MI355X): another insert order must not flag more.
    assert st.general_path <= 233


def test_near_tie_stress_construction():
    mb, sents = _near_tie_case()
    st, _, _, _ = _check(mb, sents, long_last=None)
    assert st.general_path > 0


# ---- 5. the c2 shape ---------------------------------------------------------

def test_ws_words_next_to_continuation_bytes():
    """A deep piece that starts with "▁" (its next position is a continuation
    byte, no char start) as chain 0 and as chain 1, runs of such words, and a
    stray continuation byte before, inside and after one."""
    p = base_pieces() + [("q", -3.0, NORMAL), (WS, -2.0, NORMAL)] + _singles(L16)
    p += [(WS + L16[:n].encode(), -1.0 - 0.015625 * n, NORMAL) for n in (2, 3, 5, 8, 10, 12)]
    p += [(L16[:n], -2.5 - 0.015625 * n, NORMAL) for n in (4, 6, 9)]
    ws = lambda n: WS + L16[:n].encode()
    bodies = [ws(12), ws(10), ws(8) + b"q", ws(5), ws(12) * 3, ws(12) + ws(2) + ws(8), ws(9), ws(12) + b"a",
              b"\x96" + ws(12), b"\x81" + ws(10) + b"\x81", ws(12) + b"\x96\x81", WS[:2] + ws(8), ws(5) + WS[:1],
              ws(4) + b"\x81" + L16[4:12].encode(), ws(3) + ws(12)[1:]]
    sents = [b"q" * phase + b for b in bodies for phase in range(4)]
    st, oids, olens, oto = _check(model(p, UNIGRAM), sents)
    assert {3 + 12, 3 + 10, 3 + 8, 3 + 5} <= set(olens.tolist())
    assert st.general_path == 0


# ---- 6. differential ---------------------------------------------------------

def test_differential_synth32k():
    """2,000 sentences of the benchmark's corpus with its 32k model."""
    mb = open(os.path.join(ROOT, "data", "synth32k_unigram.model"), "rb").read()
    buf, off = synth.normalized(2000, seed=4321)
    b = buf.tobytes()
    sents = [b[int(off[i]):int(off[i + 1])] for i in range(2000)]
    long_last = max(sents, key=len)
    long_last = long_last if len(long_last) > 64 else long_last * (64 // len(long_last) + 1)
    general = 0
    for k in range(0, 2000, 399):
        st, _, _, _ = _check(mb, sents[k:k + 399], long_last=long_last)
        general += int(st.general_path)
    assert general == 0


def test_differential_botchan():
    """The first 400 lines of botchan.txt, normalized by the model's host
    normalizer: real text, where a lane's two chains are both deep in one
    position pair out of twenty."""
    gold = os.path.join(ROOT, "tests", "golden")
    mb = open(os.path.join(gold, "test_model.model"), "rb").read()
    lines = O.read_lines_binary(os.path.join(gold, "botchan.txt"))[:400]
    dm = S.DeviceModel(mb)
    norm = list(dm.normalize(lines))
    dm.close()
    last = max(range(len(norm)), key=lambda i: len(norm[i]))
    norm.append(norm.pop(last))  # the batch ends with its longest line
    st, oids, olens, oto = _check(mb, norm, long_last=None)
    assert int((olens >= 8).sum()) > 100  # deep walks that end in a token
    print("botchan: general_path", int(st.general_path), "of", len(norm))
    # The two-chain walk flags none of these lines (measured on the kernel
    # before the merged deep phase, MI355X).  A lane with two deep chains must
    # not start to be flagged: not for having them, and not because the two
    # near-tie entries, which all slots share, fill in another order.
    assert st.general_path == 0
