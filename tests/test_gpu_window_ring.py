"""Byte kernel forward pass (unigram_fast_kernel<16, true>): the byte window
and the score ring as a group of four positions hands them to the next one.
Ids, piece lengths and token offsets bit-for-bit against the oracle.

The inputs are the smallest at which the shift and the window fetch can go
wrong: every sentence length 0..80 (both parities of the group count, the
sentence end at every byte of two consecutive window words, both sides of the
64-byte LDS back-pointer window) at every start offset mod 8; batches whose
byte count is 8k + r for every r, so the last sentence is served by every
form of the fetch near the end of the bytes; a 0xFF byte at each position of
the first fetched words, at the sentence's last byte and just behind it in
the next sentence; and the tie fixtures of test_gpu_merged_walk.py and
test_gpu_fast_forward.py, where a wrong slot or a lost -inf fill shows, with
the general-path counts measured on the kernel before this file was added.
Every batch holds at most 600 sentences.
"""
import os

import numpy as np
import pytest

import oracle_lib as O
import spm_amd as S
import synth
from model_builder import NORMAL, UNIGRAM, base_pieces, model
from test_gpu_balanced_output import L16, LONG_LAST, _check, _tokens, _x_model, _xs
from test_gpu_fast_forward import _site_model, _site_sentences
from test_gpu_merged_walk import FAMILIES, _near_tie_long_case, _tie_pieces
from test_gpu_merged_walk import _check as _check_stats
from test_gpu_piece_table import _encode_device, _near_tie_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SYNTH32K = os.path.join(ROOT, "data", "synth32k_unigram.model")


def _words_model():
    """One-byte tokens "x" / "y", the letters, and pieces of 2..15 letters that
    beat their splits: tokens of every length, so a sentence's last bytes are
    read through every depth of the window."""
    p = base_pieces() + [("x", -2.0, NORMAL), ("y", -2.5, NORMAL)]
    p += [(c, -4.0 - 0.0625 * i, NORMAL) for i, c in enumerate(L16)]
    p += [(L16[:n], -1.0 - 0.015625 * n, NORMAL) for n in range(2, 16)]
    return model(p, UNIGRAM)


def _length_sentence(n, k):
    """n bytes: one-byte tokens, then (from 4 bytes on) a piece of up to 15
    bytes that ends the sentence."""
    tail = min(n, 2 + (n + k) % 14) if n >= 4 else 0
    return _xs(n - tail, k) + L16[:tail].encode()


# ---- sentence lengths and the two-group rhythm -----------------------------------

@pytest.mark.parametrize("lead", range(8))
def test_every_length_at_every_start_offset(lead):
    """Lengths 0..80 in one batch behind a first sentence of `lead` bytes: the
    first length-0 sentence starts at offset `lead`, and the lengths that
    follow put starts at every offset mod 8 as well."""
    sents = [_xs(lead)] + [_length_sentence(n, n) for n in range(81)]
    mb = _words_model()
    oids, olens, oto = _check(mb, sents)
    for n in range(81):
        toks = _tokens(1 + n, olens, oto)
        assert sum(toks) == n
        tail = min(n, 2 + (2 * n) % 14) if n >= 4 else 0
        assert toks == [1] * (n - tail) + ([tail] if tail else []), n
    # The same lengths in descending order: other start offsets for each length.
    _check(mb, [_xs(lead)] + [_length_sentence(n, n) for n in range(80, -1, -1)] + [LONG_LAST])


# ---- the end of the resource -----------------------------------------------------

def _check_any_last(mb, sents):
    """As _check with no sentence flagged, for a batch whose last sentence may be short."""
    buf, off = S.to_csr(sents)
    oids, olens, oto = O.OracleModel(mb).encode_normalized_csr(buf, off, with_lens=True)
    dm = S.DeviceModel(mb)
    assert dm.info().fast_variant == 1
    ids, dlens, to = _encode_device(dm, buf, off)
    st = dm.stats()
    dm.close()
    assert np.array_equal(to, oto), "token counts differ"
    assert np.array_equal(ids, oids) and np.array_equal(dlens, olens)
    assert st.general_path == 0
    return oids, olens, oto


@pytest.mark.parametrize("last_len", [9, 12, 15, 71])
@pytest.mark.parametrize("r", range(8))
def test_total_bytes_mod_8(r, last_len):
    """The batch's bytes end at 8k + r, and its last sentence (9..15 bytes,
    and one longer than 64) is the one whose window fetches reach the end of
    the bytes: whole words, the last partial word byte by byte, or nothing.
    The sentence ends in a piece as long as the model allows."""
    piece = min(last_len, 15)
    last = _xs(last_len - piece) + L16[:piece].encode()
    body = [_length_sentence(n, n + 1) for n in (5, 17, 33, 70, 8, 1, 0, 26)]
    pad = (r - (sum(len(s) for s in body) + len(last))) % 8
    sents = [_xs(pad)] + body + [last]
    assert sum(len(s) for s in sents) % 8 == r
    oids, olens, oto = _check_any_last(_words_model(), sents)
    assert _tokens(len(sents) - 1, olens, oto) == [1] * (last_len - piece) + [piece]


# ---- the 0xFF flag ---------------------------------------------------------------

@pytest.mark.parametrize("lead", [0, 3, 4, 5])
def test_ff_byte_flags_its_own_sentence(lead):
    """A 0xFF byte at position 0, 3, 4, 7, 8 and at the last byte of
    sentences of several lengths: exactly those take the general kernel."""
    sents, flagged = [_xs(lead)], 0
    for n in (9, 10, 13, 16, 17, 24, 40, 66, 72):
        for pos in (0, 3, 4, 7, 8, n - 1):
            s = bytearray(_xs(n, pos))
            s[pos] = 0xFF
            sents += [bytes(s), _xs(n, pos)]
            flagged += 1
    _check(_x_model(), sents + [LONG_LAST], general=flagged)


@pytest.mark.parametrize("lead", range(8))
def test_ff_byte_of_the_next_sentence(lead):
    """A 0xFF byte as the first byte of the following sentence, within the
    bytes fetched for its predecessor (1..15 bytes long, so the byte lies in
    the first, second or third word of the window): it flags only its own."""
    sents, flagged = [_xs(lead)], 0
    for n in range(0, 16):
        sents += [_xs(n, n), b"\xff" + _xs(n % 5), _xs(3)]
        flagged += 1
    for n in (60, 63, 64, 67, 68):  # the predecessor ends near the LDS window's end
        sents += [_xs(n, n), b"\xff", _xs(2)]
        flagged += 1
    _check(_x_model(), sents + [LONG_LAST], general=flagged)


# ---- the ring --------------------------------------------------------------------

def test_every_insert_site_and_last_piece_of_15():
    """A piece of every length at every phase, last in its sentence and not
    (ring slots up to 18), and sentences of at least 15 bytes that end in a
    15-byte piece at every phase: a lost -inf fill or a wrong slot shows here."""
    sents = _site_sentences()
    sents += [b"q" * fill + "abcdefghijklmno".encode() for fill in range(0, 24)]
    st, oids, olens, oto = _check_stats(model(_site_model(), UNIGRAM), sents)
    n0 = len(_site_sentences())
    for fill in range(24):
        assert _tokens(n0 + fill, olens, oto) == [1] * fill + [15]
    assert st.general_path == 0


def test_deep_tie_families():
    words = FAMILIES[:7] + [FAMILIES[7] + "XYZ", FAMILIES[7] + "XY"]
    sents = [("q" * phase + w + tail).encode() for w in words for tail in ("", "z", "zz", "q" + w) for phase in range(4)]
    st, oids, olens, oto = _check_stats(model(_tie_pieces(), UNIGRAM), sents)
    print("deep ties: general_path", int(st.general_path), "of", len(sents) + 1)
    # Family 5 is an exact 3-deep chain at every phase and tail (16 sentences)
    # and is handed over; nothing else is (the count of the kernel before this
    # file was added, as test_gpu_merged_walk.py holds it).
    assert st.general_path == 16


# Measured on the kernel before this change (MI355X).
PARENT_GENERAL_NEAR_TIE_LONG = 233
PARENT_GENERAL_NEAR_TIE = 219


def test_near_tie_stress_long_words_count():
    mb, sents = _near_tie_long_case()
    st, _, _, _ = _check_stats(mb, sents, long_last=None)
    print("near-tie stress, long words: general_path", int(st.general_path), "of", len(sents))
    assert st.general_path == PARENT_GENERAL_NEAR_TIE_LONG


def test_near_tie_stress_count():
    mb, sents = _near_tie_case()
    st, _, _, _ = _check_stats(mb, sents, long_last=None)
    print("near-tie stress: general_path", int(st.general_path), "of", len(sents))
    assert st.general_path == PARENT_GENERAL_NEAR_TIE


def test_c2_sentences():
    """600 sentences of the benchmark's corpus with its 32k model."""
    mb = open(SYNTH32K, "rb").read()
    buf, off = synth.normalized(600, seed=97)
    b = buf.tobytes()
    sents = [b[int(off[i]):int(off[i + 1])] for i in range(600)]
    long_last = max(sents, key=len)
    long_last = long_last if len(long_last) > 64 else long_last * (64 // len(long_last) + 1)
    for k in range(0, 600, 300):
        _check(mb, sents[k:k + 300] + [long_last], general=0)
