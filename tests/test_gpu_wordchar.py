"""GPU: WORD and CHAR models load and encode on the device
(wordchar_kernels.hip), bit-equal to the restatement of the reference
(tests/wordchar_ref.py): ids, piece lengths and token offsets, in the tile
tier and in the general tier; the raw-text entry points equal the
`sentencepiece` package's golden rows."""
import numpy as np
import pytest

import model_builder as MB
import spm_amd as S
import wordchar_cases as C
import wordchar_ref as R

pytestmark = pytest.mark.gpu
WS = C.WS
TILE = 2048  # kWcTile


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _check(dm, ref, sents, general=None):
    """Both tiers equal the restatement; `general`: sentences the tile tier
    must hand to the general tier (None: as the restatement's condition says)."""
    sents = [bytes(s) for s in sents]
    buf, off = S.to_csr(sents)
    want = R.encode_csr(ref, sents)
    if general is None:
        general = sum(0 if R.shortcut_is_exact(s) else 1 for s in sents)
    tiers = dm.info().fast_variant == 1
    for force in (False, True):
        dm.set_force_general(force)
        try:
            ids, lens, tok = dm.encode_csr_host(buf, off, with_lens=True)
        finally:
            dm.set_force_general(False)
        assert np.array_equal(tok, want[2]), force
        assert np.array_equal(ids, want[0]), force
        assert np.array_equal(lens, want[1]), force
        st = dm.stats()
        assert st.sentences == len(sents)
        assert st.general_path == (general if tiers and not force else len(sents)), force


def test_load_and_info():
    for name, _corpus, kind in C.FIXTURES:
        info = S.DeviceModel(C.model_bytes(name)).info()
        assert info.model_type == kind and info.fast_variant == 1 and info.unk_id == 0


@pytest.mark.parametrize("name", [f[0] for f in C.FIXTURES])
def test_corpus_equals_restatement(name):
    """Every normalized corpus line; the normalizer's output is valid UTF-8,
    so nothing leaves the tile tier (a condition, not a measurement)."""
    dm = S.DeviceModel(C.model_bytes(name))
    norm = dm.normalize(C.corpus(name))
    _check(dm, C.ref_model(name), norm, general=0)


def _word_pieces():
    long_piece = WS + b"q" * 40  # the longest piece: 43 bytes
    return MB.base_pieces() + [
        (WS + b"a", 0.0, MB.NORMAL), (WS + b"ab", 0.0, MB.NORMAL), (WS + b"abc", 0.0, MB.NORMAL),
        (WS + b"abd", 0.0, MB.NORMAL), (long_piece, 0.0, MB.NORMAL), (WS + b"old", 0.0, MB.UNUSED),
        (WS, 0.0, MB.NORMAL), (b"first", 0.0, MB.NORMAL), (WS + "é€😀".encode(), 0.0, MB.NORMAL),
        (WS + b"<ctl>", 0.0, MB.CONTROL), (b"x" * TILE * 3, 0.0, MB.NORMAL)]


def _char_pieces():
    return MB.base_pieces() + [(WS, 0.0, MB.NORMAL), ("a", 0.0, MB.NORMAL), ("b", 0.0, MB.NORMAL),
                               ("é", 0.0, MB.NORMAL), ("€", 0.0, MB.NORMAL), ("😀", 0.0, MB.NORMAL),
                               ("z", 0.0, MB.UNUSED), ("c", 0.0, MB.CONTROL), ("ê", 0.0, MB.NORMAL)]


def _small_shapes(word):
    q = WS + b"q" * 40
    s = [b"", b"a", WS, WS * 3, b"a\x00b", "aé€😀bñ₩𝄞".encode(), WS + b"a" + WS + b"zz",
         q, q + b"q", q[:-1], WS + b"ab", WS + b"abc" + WS + b"abd" + WS + b"abe", WS + b"abcd",
         b"<s>", WS + b"<ctl>", WS + b"old", b"z", b"c", "éê".encode(), b"first" + WS + b"a", b"<unk>"]
    s += [b""] * 1000 + [b"tail" + WS + b"a"]
    s += [b"x" * (3 * TILE), b"y" * (3 * TILE) + WS + b"a"]              # a word of three tile lengths
    for n in (TILE - 1, TILE, TILE + 1):                                    # sentence lengths around the tile
        s.append((b"a" * n))
        s.append(b"a" * (n - 2) + "€".encode())                            # a 3-byte char ends at / over the edge
        s.append(b"b" * (n - 4) + WS + b"a")
    # a multi-byte char and a "▁" straddling a tile edge of the batch: pad to the edge first
    used = sum(len(x) for x in s)
    pad = (-used) % TILE
    s.append(b"a" * (pad + TILE - 1) + "€".encode() + b"a" * (TILE - 4) + WS + b"a" + WS)
    s.append(b"")
    return s


@pytest.mark.parametrize("kind", [R.WORD, R.CHAR])
def test_smallest_shapes(kind):
    pieces = _word_pieces() if kind == R.WORD else _char_pieces()
    dm = S.DeviceModel(MB.model(pieces, model_type=kind))
    assert dm.info().model_type == kind and dm.info().fast_variant == 1
    ref = R.Model(pieces, kind)
    _check(dm, ref, _small_shapes(kind == R.WORD), general=0)
    _check(dm, ref, [], general=0)                       # n = 0
    _check(dm, ref, [b""], general=0)
    _check(dm, ref, [b"", b"", b""], general=0)
    if kind == R.WORD:
        # tiles that hold no token start at all: one word over many tiles
        _check(dm, ref, [b"w" * (5 * TILE + 7)], general=0)
        _check(dm, ref, [b"x" * (3 * TILE)], general=0)   # equals the longest piece


@pytest.mark.parametrize("kind", [R.WORD, R.CHAR])
def test_long_lines_among_short_ones(kind):
    """Lines of many tiles (the wave-wide part of the per-tile sentence pass,
    a token that ends many tiles after it starts), with empty sentences and
    short ones around them, and a long line that ends the batch."""
    pieces = _word_pieces() if kind == R.WORD else _char_pieces()
    dm = S.DeviceModel(MB.model(pieces, model_type=kind))
    ref = R.Model(pieces, kind)
    long_word = b"w" * (70 * TILE + 5)                    # more than 64 tiles: two steps of the wave
    sents = [WS + b"a", long_word, b"", b"", WS + b"ab" + WS + b"a", b"a" * (9 * TILE) + WS + b"a", b"",
             "€".encode() * (3 * TILE), WS + b"a", b"b" * (12 * TILE + 1)]
    _check(dm, ref, sents, general=0)
    _check(dm, ref, [long_word], general=0)


def test_word_ids_of_special_pieces():
    """Known ids, not only equality with the restatement."""
    pieces = _word_pieces()
    dm = S.DeviceModel(MB.model(pieces, model_type=R.WORD))
    sents = [b"<s>", WS + b"<ctl>", WS + b"old", WS + b"abc" + WS + b"abd" + WS + b"abe", b"x" * (3 * TILE),
             b"x" * (3 * TILE + 1), b"x" * (3 * TILE - 1)]
    buf, off = S.to_csr(sents)
    ids, tok = dm.encode_csr_host(buf, off)
    assert ids.tolist() == [1, 12, 8, 5, 6, 0, 13, 0, 0]
    assert tok.tolist() == [0, 1, 2, 3, 6, 7, 8, 9]


MALFORMED = (b"ab\xe3", b"ab\xe3a", b"\x81ab", b"a\xffb", b"ab\xe2\x96", b"a\xf0" + WS + b"b", b"\xc3\x81\x81",
             b"\xbf", b"a\x80", b"\xf0\x9f\x98", b"\xe3\x81a\x81")


@pytest.mark.parametrize("kind", [R.WORD, R.CHAR])
def test_malformed_utf8(kind):
    """Each malformed sentence equals the restatement, alone and mixed among
    valid ones; the general tier runs exactly those the condition names."""
    pieces = _word_pieces() if kind == R.WORD else _char_pieces()
    dm = S.DeviceModel(MB.model(pieces, model_type=kind))
    ref = R.Model(pieces, kind)
    bad = [s for s in MALFORMED if not R.shortcut_is_exact(s)]
    assert len(bad) >= 6 and len(bad) < len(MALFORMED)   # cut-off runs at the sentence end stay in the tile tier
    mixed = []
    for k, s in enumerate(MALFORMED):
        mixed += [WS + b"a" + WS + b"ab", s, b"", "é€".encode() * (k * 37)]
    # the sentence after one that ends in a cut-off lead byte begins with the bytes that would complete it
    mixed += [b"ab\xe2", b"\x96\x81a", b"ab\xe2\x96", b"\x81a", b"a" * (TILE - 1) + b"\xe2", b"\x96\x81"]
    _check(dm, ref, mixed)
    for s in MALFORMED:
        _check(dm, ref, [s])


def test_char_user_defined():
    pieces = _char_pieces() + [("the", 0.0, MB.USER_DEFINED), ("<tag>", 0.0, MB.USER_DEFINED),
                               ("then", 0.0, MB.USER_DEFINED), ("aé€", 0.0, MB.USER_DEFINED)]
    dm = S.DeviceModel(MB.model(pieces, model_type=R.CHAR))
    assert dm.info().fast_variant == 0
    ref = R.Model(pieces, R.CHAR)
    sents = [b"athenb", b"thea", b"th", b"<tag>a<tag", WS + b"then" + WS + b"the", "aé€aéa".encode(), b"",
             b"a" * (TILE + 3) + b"then", b"\xe3the", b"the\x81"]
    _check(dm, ref, sents)
    buf, off = S.to_csr([b"athenb"])
    ids, tok = dm.encode_csr_host(buf, off)
    assert ids.tolist() == [4, 14, 5]   # longest match wins: "then", not "the" + unknown "n"


def _async(dm, sents, capacity, status_init=0):
    import torch
    dev = _dev()
    buf, off = S.to_csr(sents)
    n = len(sents)
    size = max(int(off[-1]), capacity, 1)
    d_b = torch.from_numpy(buf if buf.size else np.zeros(1, np.uint8)).to(dev)
    d_o = torch.from_numpy(off.view(np.int64)).to(dev)
    d_ids = torch.full((size + 64,), -7, dtype=torch.int32, device=dev)
    d_len = torch.full((size + 64,), -7, dtype=torch.int32, device=dev)
    d_tok = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
    d_st = torch.full((1,), status_init, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    dm.encode_device_async(d_b.data_ptr(), d_o.data_ptr(), n, capacity, d_ids.data_ptr(), d_tok.data_ptr(),
                           d_st.data_ptr(), d_len=d_len.data_ptr(), stream=s)
    torch.cuda.synchronize(dev)
    return d_ids.cpu().numpy(), d_len.cpu().numpy(), d_tok.cpu().numpy(), int(d_st.item())


@pytest.mark.parametrize("name", ["botchan_char60", "botchan_word2000"])
def test_async_entry(name):
    dm = S.DeviceModel(C.model_bytes(name))
    sents = [bytes(s) for s in dm.normalize(C.corpus(name)[:600])] + [b"ab\xe3a"]
    want = R.encode_csr(C.ref_model(name), sents)
    total = sum(len(s) for s in sents)
    for force in (False, True):
        dm.set_force_general(force)
        ids, lens, tok, st = _async(dm, sents, total + 100)
        assert st == 0
        k = int(want[2][-1])
        assert np.array_equal(tok.view(np.uint64), want[2])
        assert np.array_equal(ids[:k], want[0]) and np.array_equal(lens[:k].view(np.uint32), want[1])
        assert (ids[k:] == -7).all() and (lens[k:] == -7).all()
        # too small a capacity: RESOURCE_EXHAUSTED, nothing written
        ids, lens, tok, st = _async(dm, sents, total - 1)
        assert st == 8
        assert (ids == -7).all() and (lens == -7).all() and (tok == -7).all()
        # a later call of a failed chain does nothing and keeps the first error
        ids, lens, tok, st = _async(dm, sents, total + 100, status_init=11)
        assert st == 11
        assert (ids == -7).all() and (lens == -7).all() and (tok == -7).all()
    dm.set_force_general(False)
    # n = 0: the one token offset is written, but not in a chain that already failed
    ids, lens, tok, st = _async(dm, [], 0)
    assert st == 0 and tok.tolist() == [0]
    ids, lens, tok, st = _async(dm, [], 0, status_init=11)
    assert st == 11 and tok.tolist() == [-7]


@pytest.mark.parametrize("name", [f[0] for f in C.FIXTURES])
def test_raw_text_equals_package(name):
    """Normalize + encode + id epilogue on the device: the package's rows."""
    dm = S.DeviceModel(C.model_bytes(name))
    lines = C.corpus(name)
    assert dm.encode_lines_device(lines) == C.golden_ids(name)
    assert dm.encode_lines_device(lines, "bos:eos:reverse") == C.golden_ids(name, ".ids_ber.gz")


@pytest.mark.parametrize("name", [f[0] for f in C.FIXTURES])
def test_decode_equals_package(name):
    dm = S.DeviceModel(C.model_bytes(name))
    rows = C.golden_ids(name)
    ids = np.array([i for r in rows for i in r], np.int32)
    tok = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
    out, oo = dm.decode_csr_host(ids, tok)
    text = out.tobytes()
    got = [text[int(oo[i]):int(oo[i + 1])].decode("utf-8") for i in range(len(rows))]
    assert got == C.golden_decoded(name)


@pytest.mark.parametrize("name", ["botchan_char60", "botchan_word2000"])
def test_sample_and_nbest_unimplemented(name):
    dm = S.DeviceModel(C.model_bytes(name))
    buf, off = S.to_csr([WS + b"a"])
    with pytest.raises(S.SpmError) as e:
        dm.sample_encode_csr_host(buf, off, 0.5, 1)
    assert e.value.code == 12
    with pytest.raises(S.SpmError) as e:
        dm.nbest_encode_csr_host(buf, off, 3)
    assert e.value.code == 12
