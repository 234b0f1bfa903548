"""CPU: the WORD / CHAR restatement (tests/wordchar_ref.py) is pinned to (a)
the known answers of the reference's own tests and (b) the `sentencepiece`
package's output on the fixture models (tools/make_wordchar_golden.py); and
WORD / CHAR models load host-only."""
import numpy as np
import pytest

import model_builder as MB
import spm_amd as S
import wordchar_cases as C
import wordchar_ref as R


def _pieces(tokens):
    return [w for w, _ in tokens]


def test_char_model_known_answers():
    m = R.Model(C.char_test_model(), R.CHAR)
    for text, want in C.CHAR_KAT:
        assert _pieces(m.encode(text)) == want, text
    ids = [i for _, i in m.encode(C.WS + b"abABCcd")]
    assert ids == [3, 4, 5, 8, 6, 7]


def test_word_model_known_answers():
    m = R.Model(C.word_test_model(), R.WORD)
    for text, want in C.WORD_KAT:
        assert _pieces(m.encode(text)) == want, text
    assert [i for _, i in m.encode(C.WS + b"ab" + C.WS + b"cd" + C.WS + b"abc" + C.WS + b"zz")] == [3, 4, 5, 0]


def test_split_into_words_known_answers():
    for text, suffix, want in C.SPLIT_KAT:
        assert R.split_into_words(text, suffix) == want, (text, suffix)
    assert R.split_into_words(b"hello" + C.WS + C.WS, True) == [b"hello" + C.WS, C.WS]
    assert R.split_into_words(C.WS + C.WS + b"hello" + C.WS + C.WS, True) == [C.WS, C.WS, b"hello" + C.WS, C.WS]


def test_piece_to_id_precedence():
    """Reserved pieces first; an UNUSED piece keeps its id; a word that spells
    a CONTROL piece gives that piece's id."""
    pieces = MB.base_pieces() + [(C.WS + b"x", 0.0, MB.NORMAL), ("old", 0.0, MB.UNUSED)]
    m = R.Model(pieces, R.WORD)
    assert [i for _, i in m.encode(b"<s>" + C.WS + b"x" + C.WS + b"y")] == [1, 3, 0]
    assert [i for _, i in m.encode(b"old")] == [4]


def test_malformed_utf8_walk():
    """OneCharLen looks at the first byte only: a lead byte swallows what
    follows, a stray continuation byte is a char of its own."""
    m = R.Model(C.char_test_model(), R.CHAR)
    assert _pieces(m.encode(b"\xe3a\x81b")) == [b"\xe3a\x81", b"b"]
    assert _pieces(m.encode(b"\x81a")) == [b"\x81", b"a"]
    assert _pieces(m.encode(b"\xf0" + C.WS + b"a")) == [b"\xf0" + C.WS, b"a"]
    w = R.Model(C.word_test_model(), R.WORD)
    assert _pieces(w.encode(b"a\xf0" + C.WS + b"b")) == [b"a\xf0" + C.WS + b"b"]
    for s, ok in ((b"ab", True), (b"\x81a", False), (b"\xe3\x81", True), (b"\xe3a", False), (b"a\x81", False),
                  (b"\xff", True), (b"\xff\x81\x81\x81", True), (b"\xe2\x96", True), ("あ".encode(), True),
                  (b"\xc3\x81\x81", False), (b"", True)):
        assert R.shortcut_is_exact(s) == ok, s


def test_char_trainer_known_answers():
    """char_model_trainer_test.cc BasicTest through the restatement."""
    sentences = [(C.WS + line.replace(" ", "▁").encode(), 1) for line in C.TRAIN_LINES]
    for size, want in C.TRAIN_KAT:
        req = R.required_chars(R.char_counts(sentences), 0.9995, False)
        pieces, vocab = R.train_char(req, size, 3)
        assert " ".join(p.decode() for p, _ in pieces) == want
        assert vocab == size
    req = R.required_chars(R.char_counts(sentences), 0.9995, True)
    pieces, vocab = R.train_char(req, 5, 3, use_all_vocab=True)
    assert len(pieces) == 9 and vocab == 12
    # log(count) - float(log(sum)), narrowed to float
    assert pieces[0][1] == np.float32(np.log(10.0) - float(np.float32(np.log(39.0))))


@pytest.mark.parametrize("name", [f[0] for f in C.FIXTURES])
def test_restatement_equals_package(name):
    """Final ids (and pieces) of every corpus line equal the package's."""
    mb = C.model_bytes(name)
    lines = C.corpus(name)
    norm = S.DeviceModel(mb, host_only=True).normalize(lines)
    m = C.ref_model(name)
    want_ids = C.golden_ids(name)
    assert len(want_ids) == len(lines)
    want_pieces = C.golden_pieces(name)
    for k, s in enumerate(norm):
        toks = m.merge_unk(m.encode(bytes(s)))
        assert [i for _, i in toks] == want_ids[k], k
        assert [w.decode("utf-8") for w, _ in toks] == want_pieces[k], k


@pytest.mark.parametrize("name,kind", [(f[0], f[2]) for f in C.FIXTURES])
def test_host_only_load_and_info(name, kind):
    mb = C.model_bytes(name)
    dm = S.DeviceModel(mb, host_only=True)
    info = dm.info()
    pieces = C.ref_model(name)
    assert info.model_type == kind
    assert info.piece_size == len(pieces.types)
    assert info.unk_id == 0
    assert info.fast_variant == 1
    longest = max(len(p.decode("utf-8")) for p in list(pieces.pieces) + list(pieces.reserved))
    assert info.max_piece_chars == longest


@pytest.mark.parametrize("name", [f[0] for f in C.FIXTURES])
def test_host_only_decode_equals_package(name):
    """The decode table does not depend on the model type: the host loop on a
    host-only WORD / CHAR handle gives the package's text."""
    dm = S.DeviceModel(C.model_bytes(name), host_only=True)
    rows = C.golden_ids(name)
    ids = np.array([i for r in rows for i in r], np.int32)
    tok = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
    out, oo = dm.decode_csr_host(ids, tok)
    text = out.tobytes()
    assert [text[int(oo[i]):int(oo[i + 1])].decode("utf-8") for i in range(len(rows))] == C.golden_decoded(name)


def test_host_only_encode_is_refused():
    dm = S.DeviceModel(C.model_bytes("botchan_char60"), host_only=True)
    buf, off = S.to_csr([C.WS + b"a"])
    with pytest.raises(S.SpmError) as e:
        dm.encode_csr_host(buf, off)
    assert e.value.code == 9  # FAILED_PRECONDITION, as for every host-only handle


def test_host_only_info_user_defined():
    """A CHAR model with USER_DEFINED pieces has no tile tier; a WORD model
    never calls PrefixMatch, so it keeps it."""
    dm = S.DeviceModel(MB.model(C.char_test_model(), model_type=R.CHAR), host_only=True)
    assert dm.info().model_type == 4 and dm.info().fast_variant == 0 and dm.info().max_piece_chars == 5
    wm = S.DeviceModel(MB.model(C.char_test_model(), model_type=R.WORD), host_only=True)
    assert wm.info().model_type == 3 and wm.info().fast_variant == 1
