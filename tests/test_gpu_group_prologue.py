"""Byte kernel forward pass (unigram_fast_kernel<16, true>): the back-pointer
bytes of a group of four positions inside the LDS window (byte positions < 64)
leave as one word at the end of the group; past the window every char start
keeps its byte store.  Ids, piece lengths and token offsets bit-for-bit
against the oracle.

The inputs are the smallest at which that can go wrong: EOS at each of the
four positions of a group on both sides of byte 64, tokens that cross byte 64
and tokens that end or begin on it, multi-byte chars (in the vocabulary and
not) that start at each position of a group and straddle its end, chars cut
off by the sentence end, stray continuation bytes, 0xF8..0xFF bytes, near ties
whose resolved distance is written back over a byte of a group-written word,
and the corrupted-back-pointer knob on either side of byte 64.  Where nothing
is flagged on purpose the general kernel must not run at all.  Every batch
holds at most 600 sentences and ends with a sentence longer than 64 bytes.
"""
import os

import numpy as np
import pytest

import oracle_lib as O
import spm_amd as S
import synth
from model_builder import NORMAL, UNIGRAM, base_pieces, model
from test_gpu_balanced_output import (L16, LONG_LAST, P15, _check, _lengths_model, _near_tie_model, _tokens, _x_model,
                                      _xs)
from test_gpu_piece_table import _near_tie_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8] + list(range(59, 70))
# Fills of every group phase in the first two groups and on both sides of byte 64.
FILLS = list(range(0, 8)) + list(range(56, 72))
CHARS = {2: "ß", 3: "▁", 4: "🙂"}


# ---- sentence lengths: EOS at every position of a group ----------------------

def test_sentence_lengths_one_byte_tokens():
    """n one-byte tokens: every position is a char start and EOS is slot
    n % 4 of its group, in LDS up to 63 and in the scratch from 64 on."""
    sents = [_xs(n, k) for k, n in enumerate(LENGTHS)]
    oids, olens, oto = _check(_x_model(), sents + [LONG_LAST])
    for i, n in enumerate(LENGTHS):
        assert _tokens(i, olens, oto) == [1] * n


@pytest.mark.parametrize("k", [2, 5, 15])
def test_sentence_lengths_last_token_of_k_bytes(k):
    """The sentence ends with a k-byte token: the EOS back-pointer is k, set
    from k positions back, possibly from an earlier group and across byte 64."""
    ls = [n for n in LENGTHS if n >= k]
    sents = [b"q" * (n - k) + L16[:k].encode() for n in ls]
    oids, olens, oto = _check(_lengths_model(), sents + [LONG_LAST + b"q"])
    for i, n in enumerate(ls):
        assert _tokens(i, olens, oto) == [1] * (n - k) + [k]


# ---- chains across byte 64 -------------------------------------------------------

@pytest.mark.parametrize("n", [2, 5, 15])
def test_tokens_around_byte_64(n):
    """An n-byte token that begins at 49..66: it ends before byte 64, on it or
    after it, with nothing, one token or six tokens behind, so the backtrace
    steps from the scratch into a group-written LDS word at every phase (and,
    the reverse, from an LDS byte set by a position of an earlier group)."""
    cases = [(fill, tail) for fill in range(49, 67) for tail in (0, 1, 6)]
    sents = [b"q" * fill + L16[:n].encode() + b"q" * tail for fill, tail in cases]
    assert any(f < 64 < f + n for f, _ in cases) and any(f + n == 64 for f, _ in cases) and any(f == 64 for f, _ in cases)
    oids, olens, oto = _check(_lengths_model(), sents + [LONG_LAST + b"q"])
    for i, (fill, tail) in enumerate(cases):
        assert _tokens(i, olens, oto) == [1] * fill + [n] + [1] * tail


# ---- multi-byte chars at every group phase ----------------------------------------

def _chars_model(with_chars):
    p = base_pieces() + [("q", -3.0, NORMAL)] + [(c, -4.0 - 0.0625 * i, NORMAL) for i, c in enumerate(L16)]
    p += [(P15, -1.0, NORMAL)]
    if with_chars:
        p += [(c, -2.0 - 0.25 * w, NORMAL) for w, c in CHARS.items()]
        p += [(c + "ab", -2.5 - 0.25 * w, NORMAL) for w, c in CHARS.items()]  # beats char + a + b
    return model(p, UNIGRAM)


@pytest.mark.parametrize("width", [2, 3, 4])
@pytest.mark.parametrize("known", [True, False], ids=["piece", "unk"])
def test_multibyte_char_at_every_group_phase(known, width):
    """A char of `width` bytes that starts at p0, p0 + 1, p0 + 2 and p0 + 3 (it
    straddles the group's end from width + phase > 4 on): alone, followed by
    one-byte tokens, and as the head of a longer piece.  Not in the vocabulary
    it is an UNK token of its width."""
    ch = CHARS[width].encode()
    assert len(ch) == width
    cases = [(fill, tail) for fill in FILLS for tail in (b"", b"q", b"ab", b"qab")]
    sents = [b"q" * fill + ch + tail for fill, tail in cases]
    oids, olens, oto = _check(_chars_model(known), sents + [LONG_LAST])
    for i, (fill, tail) in enumerate(cases):
        if known and tail == b"ab":
            want = [1] * fill + [width + 2]
        else:
            want = [1] * fill + [width] + [1] * len(tail)
        assert _tokens(i, olens, oto) == want, (fill, tail)
    if not known:
        assert int((oids == 0).sum()) == len(cases)


# ---- malformed UTF-8 ----------------------------------------------------------------

def _malformed_sentences():
    cut = [b"\xc3", b"\xe2", b"\xe2\x96", b"\xf0", b"\xf0\x9f", b"\xf0\x9f\x99"]  # cut off by the sentence end
    stray = [b"\x80", b"\x96\x81", b"\xbf\xbf\xbf", b"\x81q\x81"]  # continuation bytes with no lead byte
    lone = [bytes([b]) for b in range(0xF8, 0xFF)]
    sents = []
    for fill in list(range(0, 8)) + list(range(60, 68)):
        pre = b"q" * fill
        sents += [pre + c for c in cut]
        sents += [pre + "ß".encode() + c for c in cut[:2]]
        sents += [pre + s + t for s in stray for t in (b"", b"q", b"abc")]
        sents += [pre + b"\xe2" + b"q\x81"]  # a lead byte whose tail bytes are no continuation bytes
    for fill in (0, 1, 2, 3, 61, 62, 63, 64):
        pre = b"q" * fill
        sents += [pre + c + t for c in lone for t in (b"", b"q", b"qabcd")]
    return sents


def test_malformed_utf8():
    """Expected output is the oracle's; how many of these the fast kernel
    flags is left open, the tokens are not."""
    sents = _malformed_sentences()
    for k in range(0, len(sents), 500):
        _check(_chars_model(True), sents[k:k + 500] + [LONG_LAST], general=None)


def test_ff_byte_is_flagged():
    """A 0xFF byte at each group phase on both sides of byte 64: exactly those
    sentences take the general kernel."""
    fills = [0, 1, 2, 3, 61, 62, 63, 64, 65, 66]
    sents = []
    for fill in fills:
        sents += [b"q" * fill + b"\xff" + b"ab", b"q" * fill + b"ab"]
    _check(_chars_model(True), sents + [LONG_LAST], general=len(fills))


# ---- near ties --------------------------------------------------------------------

def test_near_ties_at_every_group_phase():
    """Near ties resolved either way, the tie's end at every phase of a group
    on both sides of byte 64.  "abz": the counting pass redirects the step and
    writes the second setter's distance back over one byte of the word the
    group stored."""
    words = {"ab": [1, 1], "abz": [2, 1], "abq": [1, 1, 1], "abzq": [2, 1, 1], "cd": [2], "cdz": [2, 1]}
    sents = [b"q" * fill + w.encode() for fill in FILLS for w in words]
    oids, olens, oto = _check(_near_tie_model(), sents + [b"q" * 80])
    for i, s in enumerate(sents):
        fill = len(s) - len(s.lstrip(b"q"))
        assert _tokens(i, olens, oto) == [1] * fill + words[s[fill:].decode()], s


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_near_tie_stress_at_every_group_phase(shift):
    """The near-tie stress fixture with `shift` one-byte chars in front."""
    mb, sents = _near_tie_case()
    _check(mb, [b"a" * shift + s for s in sents], general=None)


# ---- the debug knob ------------------------------------------------------------------

@pytest.mark.parametrize("victim", [0, 1, 2], ids=["20_bytes", "63_bytes", "100_bytes"])
def test_corrupt_back_pointer_short_and_long(victim):
    """The EOS back-pointer zeroed after the forward pass, a byte store into a
    group-written LDS word (20 and 63 bytes) or into the scratch (100): exactly
    that sentence takes the general kernel."""
    sents = [_xs(20), _xs(63), _xs(100), _xs(7), LONG_LAST]
    oids, olens, oto = _check(_x_model(), sents, general=1, corrupt=victim)
    assert _tokens(victim, olens, oto) == [1] * len(sents[victim])


# ---- real text ---------------------------------------------------------------------

def test_c2_sentences():
    """2,000 sentences of the benchmark's corpus with its 32k model."""
    mb = open(os.path.join(ROOT, "data", "synth32k_unigram.model"), "rb").read()
    buf, off = synth.normalized(2000, seed=4321)
    b = buf.tobytes()
    sents = [b[int(off[i]):int(off[i + 1])] for i in range(2000)]
    long_last = max(sents, key=len)
    long_last = long_last if len(long_last) > 64 else long_last * (64 // len(long_last) + 1)
    for k in range(0, 2000, 500):
        _check(mb, sents[k:k + 500] + [long_last])


def test_botchan_lines():
    """The first 400 lines of botchan.txt, normalized by the model's host normalizer."""
    gold = os.path.join(ROOT, "tests", "golden")
    mb = open(os.path.join(gold, "test_model.model"), "rb").read()
    lines = O.read_lines_binary(os.path.join(gold, "botchan.txt"))[:400]
    dm = S.DeviceModel(mb)
    norm = list(dm.normalize(lines))
    dm.close()
    last = max(range(len(norm)), key=lambda i: len(norm[i]))
    norm.append(norm.pop(last))  # the batch ends with its longest line
    assert len(norm[-1]) > 64
    _check(mb, norm)
