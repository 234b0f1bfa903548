"""Byte kernel forward pass (unigram_fast_kernel<16, true>): every unrolled
insert site, the UNK node, positions that are no char starts, and the near-tie
entries, bit-for-bit against the oracle.

The forward pass is unrolled over walk depth (1..15), position phase within a
group of four (0..3) and walk lane (two positions are walked together), takes
a one-byte char's UNK node from its root table and the others from a select
that is skipped per wave, and keeps its predicates as wave masks: each case
below is built so that one of those paths decides the result.  Batches go
through the device-pointer API (the host API serves batches this small with
another kernel); every batch ends with a sentence longer than 64 bytes.
"""
import os

import numpy as np
import pytest

import oracle_lib as O
import spm_amd as S
import synth
from model_builder import NORMAL, UNIGRAM, UNUSED, base_pieces, model
# _near_tie_case is test_gpu_parity.test_unigram_near_tie_stress's model and
# sentence construction as a function (the test itself builds them inline).
from test_gpu_piece_table import _encode_device, _near_tie_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

f32 = np.float32
LETTERS = "abcdefghijklmno"  # 15
LONG_LAST = b"q" + b"abcdefgh" * 9  # > 64 bytes


def _check(mb, sents):
    """Encodes sents (+ the long last sentence) with the byte kernel and the
    oracle, asserts ids, piece lengths and offsets equal; returns (stats,
    oracle ids, oracle lens, oracle offsets)."""
    sents = list(sents) + [LONG_LAST]
    assert len(sents) <= 400 and len(sents[-1]) > 64
    buf, off = S.to_csr(sents)
    oids, olens, oto = O.OracleModel(mb).encode_normalized_csr(buf, off, with_lens=True)
    dm = S.DeviceModel(mb)
    assert dm.info().fast_variant == 1
    ids, lens, to = _encode_device(dm, buf, off)
    assert np.array_equal(to, oto), "token counts differ"
    bad = np.nonzero(ids != oids)[0]
    assert bad.size == 0, "first id mismatch at token %d" % bad[0]
    assert np.array_equal(lens, olens)
    st = dm.stats()
    assert st.general_path < len(sents)  # the fast kernel wrote tokens itself
    dm.close()
    return st, oids, olens, oto


def _site_model():
    """Pieces of every byte length 1..15 in ASCII (a prefix of LETTERS) and,
    from 3 bytes on, starting with a 3-byte char; each beats every split."""
    pieces = base_pieces() + [("q", -3.0, NORMAL), ("日", -3.5, NORMAL)]
    pieces += [(c, -4.0 - 0.125 * i, NORMAL) for i, c in enumerate(LETTERS)]
    pieces += [(LETTERS[:n], -1.0 - 0.015625 * n, NORMAL) for n in range(2, 16)]
    pieces += [("日" + LETTERS[:n - 3], -1.25 - 0.015625 * n, NORMAL) for n in range(4, 16)]
    return pieces


def _site_sentences():
    sents = []
    for n in range(1, 16):
        words = [LETTERS[:n].encode()]
        if n >= 3:
            words.append(("日" + LETTERS[:n - 3]).encode())
        for w in words:
            for phase in range(4):
                # the piece last in the sentence, and followed by another char
                sents += [b"q" * phase + w, b"q" * phase + w + b"q"]
    return sents


def test_every_insert_site():
    """A piece of every length 1..15 at every position phase 0..3 (ring slots
    phase + length up to 18), ASCII and behind a 3-byte char."""
    sents = _site_sentences()
    st, oids, olens, oto = _check(model(_site_model(), UNIGRAM), sents)
    # The whole piece is the token: each length is reached at each phase.
    for i, s in enumerate(sents):
        phase = len(s) - len(s.lstrip(b"q"))
        toks = olens[int(oto[i]):int(oto[i + 1])].tolist()
        assert toks[:phase] == [1] * phase and toks[phase] == len(s.rstrip(b"q")) - phase, (s, toks)
    assert set(range(1, 16)) <= set(olens.tolist())
    assert st.general_path == 0


# Chars without a usable single-char node: an ASCII byte in no piece, 2-, 3-
# and 4-byte chars in none, single-char pieces typed UNUSED (one and two
# bytes), and chars whose bytes are in the trie only as an inner node.
UNK_CHARS = ["z", "ß", "漢", "🙂", "u", "é", "x", "字"]


def _unk_model():
    pieces = base_pieces() + [(c, -2.0 - 0.25 * i, NORMAL) for i, c in enumerate("abcq")]
    pieces += [("ab", -3.0, NORMAL), ("u", -1.0, UNUSED), ("é", -1.0, UNUSED), ("xy", -2.5, NORMAL),
               ("字典", -2.5, NORMAL)]
    # Multi-char pieces that cover the char from either side.
    for i, x in enumerate(UNK_CHARS):
        pieces += [("a" + x, -6.0 - 0.5 * i, NORMAL), (x + "b", -6.25 - 0.5 * i, NORMAL)]
    return pieces


def _unk_sentences():
    sents = []
    for x in UNK_CHARS:
        for t in (x, x + x, x + "ab", "ab" + x + "ab", "ab" + x, "a" + x, x + "b", "a" + x + "b", "ca" + x + "bc",
                  "c" + x + "c"):
            for phase in (0, 1, 2, 3):
                sents.append(("q" * phase + t).encode())
    return sents


def test_unk_node():
    sents = _unk_sentences()
    mb = model(_unk_model(), UNIGRAM)
    st, oids, olens, oto = _check(mb, sents)
    unk = 0  # base_pieces(): <unk> first
    # The cases are what they claim: UNK tokens of 1, 2, 3 and 4 bytes occur.
    assert {1, 2, 3, 4} <= set(olens[oids == unk].tolist())
    assert st.general_path == 0


def test_positions_that_are_no_char_start():
    """A lead byte whose tail the sentence end cuts off, stray continuation
    bytes (first and later), 0xFF (flags the sentence to the general kernel)."""
    mb = model(_unk_model(), UNIGRAM)
    tails = [b"\xe3\x81", b"\xe3", b"\xf0\x9f\x99", b"\xf0\x9f", b"\xf0", b"\xc3", b"\x80\x80ab", b"\xbfab",
             b"a\x80b", b"\xe6\xbc", "漢".encode() + b"\xa2", b"\xe6\xbca", b"\xc3a\x80\x80b", b"\xff", b"a\xffb",
             b"ab\xff", b"\xffab"]
    sents = [b"q" * phase + pre + t for t in tails for phase in range(4) for pre in (b"", b"ab")]
    st, _, _, _ = _check(mb, sents)
    n_ff = sum(b"\xff" in s for s in sents)
    assert st.general_path == n_ff


def _near_tie_model():
    """Setters of one end position an ulp apart.  Scores are small dyadic
    numbers and the filler 'q' scores 0, so every sum below is exact at every
    phase.  Per family (own letters), in ascending begin = insert order:
      a b    : ab = a + b - ulp            (later setter wins by an ulp)
      c d    : cd = c + d + ulp            (later setter loses by an ulp)
      e f    : ef = e + f                  (exact tie: the first one stays)
      g h i  : ghi < g + hi < gh.. + i     (three setters, an ulp each: 3-deep)
      j k l  : jkl < j + kl, then j k + l far above (the entry is cleared)
      r..y   : rstuvwxy < r + stuvwxy at end 8, set in group 0, used after two
               ring shifts; variants with a far and with a near third setter.
    """
    up = lambda v: np.nextafter(f32(v), f32(np.inf))
    dn = lambda v: np.nextafter(f32(v), f32(-np.inf))
    p = base_pieces() + [("q", 0.0, NORMAL), ("z", -2.0, NORMAL), ("zz", -16.0, NORMAL)]
    p += [("a", -1.0, NORMAL), ("b", -2.0, NORMAL), ("ab", float(dn(-3.0)), NORMAL)]
    p += [("c", -1.0, NORMAL), ("d", -2.0, NORMAL), ("cd", float(up(-3.0)), NORMAL)]
    p += [("e", -1.0, NORMAL), ("f", -2.0, NORMAL), ("ef", -3.0, NORMAL)]
    # ghi: end 3 set by ghi (begin 0), g + hi (begin 1), T2 + i (begin 2), T2 = g + h = -3.
    p += [("g", -1.0, NORMAL), ("h", -2.0, NORMAL), ("i", -4.0, NORMAL), ("hi", float(dn(-6.0)), NORMAL),
          ("ghi", float(dn(dn(-7.0))), NORMAL)]
    # jkl: jkl one ulp below j + kl = -9, then (j + k) + l = -5: far.
    p += [("j", -1.0, NORMAL), ("k", -2.0, NORMAL), ("l", -2.0, NORMAL), ("kl", -8.0, NORMAL),
          ("jkl", float(dn(-9.0)), NORMAL)]
    # r..y: end 8.  rstuvwxy (begin 0) one ulp below r + stuvwxy (begin 1) = -9.
    p += [("r", -1.0, NORMAL), ("stuvwxy", -8.0, NORMAL), ("rstuvwxy", float(dn(-9.0)), NORMAL)]
    # third setters of end 8 from begin 7 (T7 = rstuvwx = -6): y is absent
    # (UNK, far below); Y1 = 'm' far above (-8), Y2 = 'n' an ulp above -9.
    p += [("rstuvwx", -6.0, NORMAL), ("rstuvwxm", float(dn(-9.0)), NORMAL), ("stuvwxm", -8.0, NORMAL),
          ("m", -2.0, NORMAL), ("rstuvwxn", float(dn(dn(-9.0))), NORMAL), ("stuvwxn", float(dn(-8.0)), NORMAL),
          ("n", -3.0, NORMAL)]
    return p


def _near_tie_sentences():
    fam = {
        "two_later_wins": ["ab", "abz", "abzz", "abab"],
        "two_later_loses": ["cd", "cdz", "cdzz", "cdab"],
        "exact_tie": ["ef", "efz", "efzz"],
        "three_deep": ["ghi", "ghiz", "zghi"],
        "cleared": ["jkl", "jklz", "jklzz", "jklab"],
        "ring_shift": ["rstuvwxy", "rstuvwxyz", "rstuvwxyzz", "rstuvwxm", "rstuvwxmz", "rstuvwxmzz"],
        "ring_shift_near_third": ["rstuvwxn", "rstuvwxnz"],
        # two open entries, then a third: the entry list overflows
        "overflow": ["ababab", "abzabzab", "abrstuvwxyab"],
        "two_open": ["abab", "abzzab", "abrstuvwxy"],
    }
    sents, tags = [], []
    for tag, words in fam.items():
        for w in words:
            for phase in range(4):
                sents.append(("q" * phase + w).encode())
                tags.append(tag)
    return sents, tags


def test_near_tie_entries():
    sents, tags = _near_tie_sentences()
    st, _, _, _ = _check(model(_near_tie_model(), UNIGRAM), sents)
    # The general kernel's share: "ghi" behind 0-3 fillers of score 0 is an
    # exact 3-deep chain (sums of small dyadic numbers), and the long last
    # sentence opens a near pair with each of its nine "ab".
    print("near-tie fixtures: general_path", int(st.general_path), "of", len(sents) + 1)
    assert st.general_path >= 4 + 1


def test_near_tie_stress_construction():
    """The near-tie stress model and 300 of its sentences."""
    mb, sents = _near_tie_case()
    st, _, _, _ = _check(mb, sents)
    assert st.general_path > 0


def test_estep_forward_mode():
    """The same fixtures through the E-step's forward mode of the byte kernel
    (spm_hip_estep, PARITY) against the oracle: expected counts, objective and
    token count bit-exact."""
    pieces, scores = [], []
    seen = set()
    for p, s, t in _site_model() + _unk_model()[3:] + _near_tie_model()[3:]:
        b = p.encode() if isinstance(p, str) else p
        if t == NORMAL and b not in seen:
            seen.add(b)
            pieces.append(b)
            scores.append(s)
    scores = np.array(scores, dtype=np.float32)
    tails = [b"\xe3\x81", b"\x80\x80ab", b"a\xffb", b"\xf0\x9f"]
    sents = _site_sentences()[::3] + _unk_sentences()[::5] + _near_tie_sentences()[0][::2] + tails + [LONG_LAST]
    sents = [s for s in sents if s]
    freqs = np.arange(len(sents)) % 3 + 1
    e_ref, obj_ref, nt_ref = O.estep(sents, freqs, pieces, scores, 1)
    dp = S.DevicePieces(pieces, scores)
    dp.set_forward(1)  # the encode byte kernel's E-step mode
    e, obj, nt = dp.estep(sents, freqs, mode=S.SPM_ESTEP_PARITY, threads=1)
    assert np.array_equal(e.view(np.uint32), e_ref.view(np.uint32))
    assert np.float32(obj).view(np.uint32) == np.float32(obj_ref).view(np.uint32), (obj, obj_ref)
    assert nt == nt_ref


# stats().general_path of the commit before the forward pass's instruction
# diet on these 100 k sentences (measured once on that commit, MI355X).
PARENT_GENERAL_PATH_100K = 0


def test_general_path_count_unchanged():
    """The near-tie predicate of the inserts is a superset of the parent's: it
    must not start sending c2 sentences to the general kernel."""
    import torch
    mb = open(os.path.join(ROOT, "data", "synth32k_unigram.model"), "rb").read()
    buf, off = synth.normalized(100000, seed=1234)
    dm = S.DeviceModel(mb)
    assert dm.info().fast_variant == 1
    dev = torch.device("cuda:0")
    n = len(off) - 1
    d_b = torch.from_numpy(buf).to(dev)
    d_o = torch.from_numpy(off.view(np.int64)).to(dev)
    d_ids = torch.empty(max(int(off[-1]), 1), dtype=torch.int32, device=dev)
    d_tok = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    dm.encode_device(d_b.data_ptr(), d_o.data_ptr(), n, d_ids.data_ptr(), d_tok.data_ptr())  # blocking
    torch.cuda.synchronize()
    got = int(dm.stats().general_path)
    print("general_path on 100k synth.normalized sentences:", got)
    assert got == PARENT_GENERAL_PATH_100K
