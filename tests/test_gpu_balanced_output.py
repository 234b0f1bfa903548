"""Byte kernel output stage (unigram_fast_kernel<16, true>): the counting
backtrace leaves the final chain in the back-pointer bytes, the lanes list
their tokens as (offset, length) descriptors in LDS, a window of 1264 tile-local
token indices at a time and the last window first, and the block looks the
window's tokens up one per thread.  Ids, piece lengths and token offsets
bit-for-bit against the oracle.

The inputs are the smallest at which such a stage can go wrong: tile totals
around the block size and the window size, empty tiles and lanes, a tile's
tokens all in one lane, a chain that crosses from the global back-pointer
scratch into LDS, tokens of every length, UNK chars of every width, tokens in
the batch's last 20 bytes, near ties resolved either way on both sides of byte
64, and a flagged sentence in the middle of a multi-window tile.  Where
nothing is flagged on purpose the general kernel must not run at all, so it
cannot hide a broken fast path.  Batches go through the device-pointer API,
hold at most 600 sentences and end with a sentence longer than 64 bytes.
"""
import os

import numpy as np
import pytest
import torch

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
P15 = L16[:15].encode()
LONG_LAST = P15 * 5  # 75 bytes, five tokens
WINDOW = 1264  # kStageIds


def _encode_device_no_lens(dm, buf, off):
    dev = torch.device("cuda:0")
    n = len(off) - 1
    cap = max(int(off[-1]), 1)
    d_b = torch.from_numpy(buf).to(dev)
    d_o = torch.from_numpy(off.view(np.int64)).to(dev)
    d_ids = torch.full((cap,), -7, dtype=torch.int32, device=dev)
    d_tok = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    dm.encode_device(d_b.data_ptr(), d_o.data_ptr(), n, d_ids.data_ptr(), d_tok.data_ptr())
    torch.cuda.synchronize()
    to = d_tok.cpu().numpy().view(np.uint64)
    return d_ids.cpu().numpy()[:int(to[-1])], to


def _check(mb, sents, general=0, corrupt=None, lens=True):
    """Encodes sents with the byte kernel and with the oracle, asserts ids,
    piece lengths and offsets equal and that exactly `general` sentences took
    the general kernel; returns (oracle ids, oracle lens, oracle offsets)."""
    sents = list(sents)
    assert len(sents) <= 600 and len(sents[-1]) > 64
    buf, off = S.to_csr(sents)
    oids, olens, oto = O.OracleModel(mb).encode_normalized_csr(buf, off, with_lens=True)
    dm = S.DeviceModel(mb)
    assert dm.info().fast_variant == 1
    if corrupt is not None:
        dm.set_debug_corrupt_bp(corrupt)
    if lens:
        ids, dlens, to = _encode_device(dm, buf, off)
    else:
        ids, to = _encode_device_no_lens(dm, buf, off)
    st = dm.stats()
    dm.close()
    assert np.array_equal(to, oto), "token counts differ"
    bad = np.nonzero(ids != oids)[0]
    assert bad.size == 0, "first id mismatch at token %d" % bad[0]
    if lens:
        assert np.array_equal(dlens, olens)
    if general is not None:
        assert st.general_path == general
    return oids, olens, oto


def _tokens(i, olens, oto):
    return olens[int(oto[i]):int(oto[i + 1])].tolist()


def _tile_total(oto, tile=0):
    return int(oto[min(256 * (tile + 1), len(oto) - 1)]) - int(oto[256 * tile])


# ---- one-byte tokens: the counts are the sentence lengths -------------------

def _x_model():
    """"x" and "y" are pieces and no piece holds two of them: a sentence of n
    such bytes is n tokens.  P15 makes the long last sentence five tokens."""
    p = base_pieces() + [("x", -2.0, NORMAL), ("y", -2.5, NORMAL)]
    p += [(c, -4.0 - 0.0625 * i, NORMAL) for i, c in enumerate(L16)] + [(P15, -1.0, NORMAL)]
    return model(p, UNIGRAM)


def _xs(n, k=0):
    return bytes(b"xy"[(k + t) & 1] for t in range(n))


@pytest.mark.parametrize("lens", [True, False], ids=["lens", "ids_only"])
@pytest.mark.parametrize("total", [0, 1, 255, 256, 257, 512])
def test_tile_totals_around_the_block(total, lens):
    """A first tile of `total` tokens (sentences of 0, 1 or 2 one-byte tokens),
    then a second tile.  Total 0: a tile that runs no window at all."""
    if total <= 256:
        first = [_xs(1, k) for k in range(total)] + [b""] * (256 - total)
        first = first[::-1] if total == 255 else first  # the empty sentence first
    elif total == 257:
        first = [_xs(1, k) for k in range(100)] + [_xs(2)] + [_xs(1, k) for k in range(155)]
    else:
        first = [_xs(2, k) for k in range(256)]
    second = [_xs(k % 5, k) for k in range(40)]
    oids, olens, oto = _check(_x_model(), first + second + [LONG_LAST], lens=lens)
    assert _tile_total(oto) == total and len(first) == 256
    assert _tokens(len(first) + len(second), olens, oto) == [15] * 5


@pytest.mark.parametrize("n", [1, 257, 300])
def test_sentence_counts(n):
    """One sentence (255 invalid lanes); a second tile of one sentence; a
    second tile with 44 valid lanes."""
    sents = [_xs(k % 7, k) for k in range(n - 1)] + [_xs(70)]
    oids, olens, oto = _check(_x_model(), sents)
    assert int(oto[-1]) - int(oto[-2]) == 70


def _lengths_2816():
    """256 lengths, 11 on average, varied, no sentence boundary at token 1264 or 2528."""
    ls = [11 + ((k * 7) % 9 - 4) for k in range(256)]
    ls[-1] += 2816 - sum(ls)
    return ls


@pytest.mark.parametrize("name", ["6_each", "11_varied", "exactly_1264", "1265"])
def test_two_and_three_windows(name):
    ls = {"6_each": [6] * 256, "11_varied": _lengths_2816(), "exactly_1264": [5] * 240 + [4] * 16,
          "1265": [5] * 241 + [4] * 15}[name]
    want = {"6_each": 1536, "11_varied": 2816, "exactly_1264": 1264, "1265": 1265}[name]
    assert len(ls) == 256 and sum(ls) == want and min(ls) > 0
    if name == "11_varied":
        ends = set(np.cumsum(ls).tolist())
        assert WINDOW not in ends and 2 * WINDOW not in ends and len(set(ls)) > 4
    sents = [_xs(n, k) for k, n in enumerate(ls)] + [_xs(3), LONG_LAST]
    oids, olens, oto = _check(_x_model(), sents)
    assert _tile_total(oto) == want


@pytest.mark.parametrize("n", [60, 120])
def test_all_tokens_in_one_lane(n):
    """One sentence of n one-byte tokens among 255 one-token sentences.  60:
    its back-pointers are all in LDS; 120: the chain starts in the global
    scratch and crosses into LDS at byte 64."""
    sents = [_xs(1, k) for k in range(100)] + [_xs(n)] + [_xs(1, k) for k in range(155)]
    oids, olens, oto = _check(_x_model(), sents + [LONG_LAST])
    assert _tile_total(oto) == 255 + n and _tokens(100, olens, oto) == [1] * n


# ---- token lengths, UNK, the batch's last bytes ------------------------------

def _lengths_model():
    """Every prefix of L16 of 2..15 bytes is a piece that beats its split."""
    p = base_pieces() + [("q", -3.0, NORMAL)] + [(c, -4.0 - 0.0625 * i, NORMAL) for i, c in enumerate(L16)]
    p += [(L16[:n], -1.0 - 0.015625 * n, NORMAL) for n in range(2, 16)]
    return model(p, UNIGRAM)


def _lengths_sentences():
    sents = []
    for n in range(1, 16):
        for phase in range(4):
            sents += [("q" * phase + L16[:n]).encode(), ("q" * phase + L16[:n] + "q" + L16[:16 - n]).encode()]
    return sents + [LONG_LAST + b"q"]


@pytest.mark.parametrize("table", [True, False], ids=["table", "walk"])
def test_tokens_of_every_length(table, monkeypatch):
    """With the piece table and, with the knob set before the model loads,
    with the trie re-walk in the lookup pass."""
    if table:
        monkeypatch.delenv("SPM_HIP_NO_PIECE_TABLE", raising=False)
    else:
        monkeypatch.setenv("SPM_HIP_NO_PIECE_TABLE", "1")
    sents = _lengths_sentences()
    oids, olens, oto = _check(_lengths_model(), sents)
    assert set(range(1, 16)) <= set(olens.tolist())
    for n in range(1, 16):
        for phase in range(4):
            assert _tokens(8 * (n - 1) + 2 * phase, olens, oto) == [1] * phase + [n]


@pytest.mark.parametrize("lens", [True, False], ids=["lens", "ids_only"])
def test_unk_tokens(lens):
    """Bytes with no piece, 2-, 3- and 4-byte chars with no piece, alone, in
    runs, and next to a 15-byte piece."""
    unk = [b"Z", "ß".encode(), "漢".encode(), "🙂".encode()]
    sents = []
    for u in unk:
        for phase in range(4):
            pre = b"q" * phase
            sents += [pre + u, pre + u + u, pre + u + P15, pre + P15 + u, pre + P15 + u + P15, pre + b"a" + u + b"b"]
    sents.append(b"".join(unk) * 2 + P15)
    sents.append(P15 + b"".join(unk) * 6 + P15)
    oids, olens, oto = _check(_lengths_model(), sents, lens=lens)
    assert {1, 2, 3, 4, 15} <= set(olens.tolist())
    assert _tokens(8, olens, oto) == [1, 1, 15]  # "q" + "Z" + P15
    assert int((oids == 0).sum()) >= 4 * 4 * 7


@pytest.mark.parametrize("phase", [0, 1, 2, 3])
def test_tokens_in_the_batch_tail(phase):
    """The last sentence's tokens end within the batch's last 20 bytes (no
    aligned 16 + 4-byte load fits there), at every alignment of the end."""
    last = b"q" * 50 + P15 + L16[:7].encode() + b"q" + L16[:3].encode() + b"qa"
    sents = [b"q" * phase, L16[:9].encode()] + [last]
    oids, olens, oto = _check(_lengths_model(), sents)
    assert _tokens(2, olens, oto)[-6:] == [15, 7, 1, 3, 1, 1]
    assert int(oto[-1]) == phase + 1 + 50 + 6


# ---- near ties -------------------------------------------------------------------

def _near_tie_model():
    """Two setters of one end position an ulp apart; the filler "q" scores 0
    and the scores are small dyadic numbers, so sums are exact anywhere.
      ab = a + b - ulp: the later setter (begin 1) holds the maximum.  With
        nothing behind, it wins: [a, b].  A token behind ("z", -2) rounds the
        two sums together and the earlier begin wins: [ab], the step that the
        counting pass redirects and writes back.
      cd = c + d + ulp: the later setter loses outright, [cd] either way."""
    dn = lambda v: float(np.nextafter(f32(v), f32(-np.inf)))
    up = lambda v: float(np.nextafter(f32(v), f32(np.inf)))
    p = base_pieces() + [("q", 0.0, NORMAL), ("z", -2.0, NORMAL)]
    p += [("a", -1.0, NORMAL), ("b", -2.0, NORMAL), ("ab", dn(-3.0), NORMAL)]
    p += [("c", -1.0, NORMAL), ("d", -2.0, NORMAL), ("cd", up(-3.0), NORMAL)]
    return model(p, UNIGRAM)


def test_near_ties_resolved_either_way_before_and_after_byte_64():
    # (a token of score 0 behind the pair changes no sum: the later setter still wins)
    words = {"ab": [1, 1], "abz": [2, 1], "abq": [1, 1, 1], "abzq": [2, 1, 1], "cd": [2], "cdz": [2, 1]}
    fills = (0, 1, 2, 3, 40, 61, 62, 63, 64, 65, 70, 130)
    sents = [b"q" * fill + w.encode() for fill in fills for w in words]
    oids, olens, oto = _check(_near_tie_model(), sents + [b"q" * 80])
    for i, s in enumerate(sents):
        fill = len(s) - len(s.lstrip(b"q"))
        assert _tokens(i, olens, oto) == [1] * fill + words[s[fill:].decode()], s


def test_near_tie_stress_construction():
    mb, sents = _near_tie_case()
    _check(mb, sents, general=None)


# ---- flagged sentences in a multi-window tile ------------------------------------

def _multi_window_sentences():
    return [_xs(6, k) for k in range(256)] + [_xs(2), LONG_LAST]


def test_flagged_sentence_in_a_multi_window_tile():
    """A 0xFF byte flags sentence 128 of a 1536-token tile: it takes the
    general kernel, its neighbours stay where they are."""
    sents = _multi_window_sentences()
    sents[128] = b"xy\xffxyx"
    oids, olens, oto = _check(_x_model(), sents, general=1)
    assert _tokens(127, olens, oto) == [1] * 6 and _tokens(129, olens, oto) == [1] * 6


@pytest.mark.parametrize("victim", [3, 128, 250])
def test_corrupt_back_pointer_in_a_multi_window_tile(victim):
    """Debug knob: the sentence's EOS back-pointer is zeroed after the forward
    pass; the counting pass flags it before anything is described."""
    oids, olens, oto = _check(_x_model(), _multi_window_sentences(), general=1, corrupt=victim)
    assert _tile_total(oto) == 1536


# ---- differential ----------------------------------------------------------------

def test_differential_c2():
    """2,000 sentences of the benchmark's corpus with its 32k model."""
    mb = open(os.path.join(ROOT, "data", "synth32k_unigram.model"), "rb").read()
    buf, off = synth.normalized(2000, seed=1234)
    b = buf.tobytes()
    sents = [b[int(off[i]):int(off[i + 1])] for i in range(2000)]
    long_last = max(sents, key=len)
    long_last = long_last if len(long_last) > 64 else long_last * (64 // len(long_last) + 1)
    for k in range(0, 2000, 500):
        _check(mb, sents[k:k + 500] + [long_last])


def test_differential_botchan():
    """The first 400 lines of botchan.txt, normalized by the model's host
    normalizer: real text, every tile of several windows."""
    gold = os.path.join(ROOT, "tests", "golden")
    mb = open(os.path.join(gold, "test_model.model"), "rb").read()
    lines = O.read_lines_binary(os.path.join(gold, "botchan.txt"))[:400]
    dm = S.DeviceModel(mb)
    norm = list(dm.normalize(lines))
    dm.close()
    last = max(range(len(norm)), key=lambda i: len(norm[i]))
    norm.append(norm.pop(last))  # the batch ends with its longest line
    oids, olens, oto = _check(mb, norm)
    assert _tile_total(oto) > 2 * WINDOW
