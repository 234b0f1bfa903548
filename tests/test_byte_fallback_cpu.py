"""CPU: byte fallback.  The restatement (byte_fallback_ref.py) equals the
`sentencepiece` package and its recorded answers; the load rules and the
host-only handle follow the package."""
import numpy as np
import pytest
import sentencepiece

import byte_fallback_ref as R
import model_builder as mb
import oracle_lib as O
import spm_amd as S

WS = "▁"

# Byte tokens the package produces under the unigram fixture: (tokens, lines holding one, lines).
BYTE_CENSUS = {"botchan": (5187, 2517, 4288), "wagahaiwa": (1108617, 2342, 2344)}

# ids of byte values, for the decode cases (hand-model numbering: R.FIRST_BYTE_ID + byte)
DECODE_CASES = [
    ([0xE6, 0x97], "��"),
    ([0x97, 0xE6, 0x97, 0xA5, 0x41], "�日A"),
    ([0xC0, 0x80], "��"),
    ([0xED, 0xA0, 0x80], "���"),
    ([0xF0, 0x9F, 0x98, 0x80], "😀"),
    ([0x20, 0x41], " A"),
    ([0xE2, 0x96, 0x81, 0x41], "▁A"),
]


@pytest.fixture(scope="module", params=R.FIXTURES)
def fixture(request):
    mbytes = R.fixture_model(request.param)
    return request.param, mbytes, sentencepiece.SentencePieceProcessor(model_proto=mbytes)


_RESTATED = {}


def restated_corpus(fixture_name, mbytes, corpus, corpus_file):
    """(off, ids, begins, ends) of the restatement over a whole corpus: oracle
    model-level encode of the CONTROL view, then the expansion."""
    key = (fixture_name, corpus)
    if key not in _RESTATED:
        lines = R.corpus_lines(corpus_file)
        om = O.OracleModel(R.control_view(mbytes))
        pairs = om.normalize_align(lines)
        norm = [p[0] for p in pairs]
        n2o = [p[1] if p[0] else [0] for p in pairs]  # (no vector for an empty text: no token reads it)
        buf, off = O.to_csr(norm)
        ids, lens, to = om.encode_normalized_csr(buf, off, threads=4, with_lens=True)
        bids = R.byte_ids(mbytes)
        unk = R.Model(mbytes).unk_id
        out_ids, out_b, out_e, out_off = [], [], [], [0]
        for i in range(len(lines)):
            t0, t1 = int(to[i]), int(to[i + 1])
            rows = R.expand(ids[t0:t1], lens[t0:t1], norm[i], unk, bids, n2o[i])
            out_ids.extend(r[0] for r in rows)
            out_b.extend(r[1] for r in rows)
            out_e.extend(r[2] for r in rows)
            out_off.append(len(out_ids))
        _RESTATED[key] = (np.array(out_off, np.uint64), np.array(out_ids, np.int32), np.array(out_b, np.uint32),
                          np.array(out_e, np.uint32))
    return _RESTATED[key]


@pytest.mark.parametrize("corpus,corpus_file", R.CORPORA)
def test_restatement_equals_the_recorded_package_answers(fixture, corpus, corpus_file):
    name, mbytes, sp = fixture
    off, ids, begins, ends = R.recorded_spt(corpus, name)
    r_off, r_ids, r_b, r_e = restated_corpus(name, mbytes, corpus, corpus_file)
    assert np.array_equal(off, r_off) and np.array_equal(ids, r_ids)
    assert np.array_equal(begins, r_b) and np.array_equal(ends, r_e)
    # Not vacuous: the byte tokens are there.
    is_byte = np.isin(ids, np.array(R.byte_ids(mbytes)))
    tokens, with_bytes, n = BYTE_CENSUS[corpus]
    per_line = np.add.reduceat(is_byte, off[:-1].astype(np.int64)) * (np.diff(off.astype(np.int64)) > 0)
    assert (int(is_byte.sum()), int((per_line > 0).sum()), len(off) - 1) == (tokens, with_bytes, n)


@pytest.mark.parametrize("corpus,corpus_file", R.CORPORA)
def test_recorded_answers_are_the_packages(fixture, corpus, corpus_file):
    """The fixtures against the live package, on a stride of lines: ids, pieces,
    surfaces, offsets and decoded text."""
    name, mbytes, sp = fixture
    lines = R.corpus_lines(corpus_file)
    off, ids, begins, ends = R.recorded_spt(corpus, name)
    texts = R.recorded_texts(corpus, name)
    assert len(texts) == len(lines) == len(off) - 1
    ref = R.Model(mbytes)
    for i in range(0, len(lines), 37):
        a, b = int(off[i]), int(off[i + 1])
        p = sp.encode(lines[i].decode(), out_type="proto")
        assert [x.id for x in p.pieces] == ids[a:b].tolist()
        assert [x.begin for x in p.pieces] == begins[a:b].tolist() and [x.end for x in p.pieces] == ends[a:b].tolist()
        assert [x.piece.encode() for x in p.pieces] == [ref.pieces[k][0] for k in ids[a:b]]
        assert [x.surface.encode() for x in p.pieces] == [lines[i][s:e] for s, e in zip(begins[a:b], ends[a:b])]
        assert sp.decode(ids[a:b].tolist()).encode() == texts[i]
        assert ref.decode_ids(ids[a:b].tolist())[0] == texts[i]


def test_restated_decode_of_every_recorded_line(fixture):
    name, mbytes, sp = fixture
    ref = R.Model(mbytes)
    for corpus, _ in R.CORPORA:
        off, ids, _, _ = R.recorded_spt(corpus, name)
        texts = R.recorded_texts(corpus, name)
        step = 1 if corpus == "botchan" else 9  # a wagahaiwa line is thousands of byte tokens
        for i in range(0, len(texts), step):
            assert ref.decode_ids(ids[int(off[i]):int(off[i + 1])].tolist())[0] == texts[i]


def _package_rows(sp, ids):
    p = sp.decode(ids, out_type="proto")
    return p.text.encode(), [(x.piece.encode(), x.id, x.surface.encode(), x.begin, x.end) for x in p.pieces]


def test_decode_cases(fixture):
    name, mbytes, sp = fixture
    ref = R.Model(mbytes)
    bids = R.byte_ids(mbytes)
    for seq, want in DECODE_CASES:
        ids = [bids[b] for b in seq]
        text, rows = ref.decode_ids(ids)
        assert text == want.encode()
        assert (text, rows) == _package_rows(sp, ids)
    he = sp.piece_to_id(WS + "he")
    assert not sp.is_unknown(he)
    ids = [bids[0xE6], he, bids[0x97], bids[0xA5]]
    assert ref.decode_ids(ids)[0] == "� he��".encode()
    assert ref.decode_ids(ids) == _package_rows(sp, ids)


def test_random_byte_and_ordinary_ids(fixture):
    name, mbytes, sp = fixture
    ref = R.Model(mbytes)
    bids = R.byte_ids(mbytes)
    rng = np.random.default_rng(7)
    pool = [0x41, 0x20, 0xE2, 0x96, 0x81, 0xE6, 0x97, 0xA5, 0xC0, 0x80, 0xED, 0xA0, 0xF0, 0x9F, 0x98, 0xF4, 0x90, 0xC3,
            0xA9, 0xEF, 0xBF, 0xBD, 0xFF, 0xF8, 0xC2, 0xE0, 0x9F, 0xBF]
    ordinary = [i for i, (p, _, t) in enumerate(ref.pieces) if t == mb.NORMAL][:200]
    for _ in range(600):
        ids = []
        for _ in range(int(rng.integers(1, 14))):
            r = rng.random()
            if r < 0.15:
                ids.append(int(rng.choice(ordinary)))
            elif r < 0.2:
                ids.append(int(rng.integers(0, 3)))
            else:
                ids.append(bids[int(rng.choice(pool))])
        assert ref.decode_ids(ids) == _package_rows(sp, ids)
        # ... and the host-only handle's loop, with the decode extra options
        for options in ("", "reverse", "bos:eos", "reverse:bos"):
            text, rows = ref.decode_ids(ids, options)
            hm = _host_model(name, mbytes)
            got, off, begins = hm.decode_csr_host(np.array(ids, np.int32), np.array([0, len(ids)], np.uint64), options,
                                                  with_begin=True)
            assert got.tobytes() == text and begins.tolist() == [r[3] for r in rows]


_HOST = {}


def _host_model(name, mbytes):
    if name not in _HOST:
        _HOST[name] = S.DeviceModel(mbytes, host_only=True)
    return _HOST[name]


def test_reserved_byte_pieces_are_not_matched(fixture):
    name, mbytes, sp = fixture
    bids = R.byte_ids(mbytes)
    want = [sp.piece_to_id(WS)] + [bids[b] for b in b"<0x41>"] + [sp.piece_to_id(WS), bids[ord("q")]]
    assert sp.encode("<0x41> q") == want
    assert sp.encode("aあいb", out_type=str)[1:7] == ["<0xE3>", "<0x81>", "<0x82>", "<0xE3>", "<0x81>", "<0x84>"]


# ---- load rules ----

def _package_error(model_bytes):
    with pytest.raises(Exception) as e:
        sentencepiece.SentencePieceProcessor(model_proto=model_bytes)
    return str(e.value)


def _our_error(model_bytes):
    with pytest.raises(S.SpmError) as e:
        S.DeviceModel(model_bytes, host_only=True)
    return str(e.value)


PIECES = [(WS, -1.0, mb.NORMAL), ("a", -1.5, mb.NORMAL), (WS + "a", -1.2, mb.NORMAL)]


def test_load_errors_equal_the_packages():
    cases = {
        "flag off": R.hand_model(PIECES, flag=False),
        "255 bytes": R.hand_model(PIECES, byte_pieces=R.byte_rows()[:255]),
        "one missing": R.hand_model(PIECES, byte_pieces=R.byte_rows()[:0x41] + R.byte_rows()[0x42:]),
        "lower-case name": R.hand_model(PIECES, byte_pieces=R.byte_rows() + [(b"<0xab>", 0.0, R.BYTE)]),
        "duplicate": R.hand_model(PIECES, byte_pieces=R.byte_rows() + [(b"<0x41>", 0.0, R.BYTE)]),
    }
    for what, m in cases.items():
        theirs, ours = _package_error(m), _our_error(m)
        assert theirs and ours, what
        # The package prefixes the source location; the message itself is ours.
        assert ours.split(": ")[-1] in theirs, (what, ours, theirs)
    assert "is found although `byte_fallback` is false." in _our_error(cases["flag off"])
    assert "there are not 256 byte pieces although `byte_fallback` is true." in _our_error(cases["255 bytes"])


def test_byte_ids_come_from_the_names():
    rows = list(reversed(R.byte_rows()))
    m = R.hand_model(PIECES, byte_pieces=rows)
    dm = S.DeviceModel(m, host_only=True)
    table = dm.byte_fallback()
    assert table.tolist() == [3 + 255 - b for b in range(256)] == R.byte_ids(m)
    sp = sentencepiece.SentencePieceProcessor(model_proto=m)
    assert [sp.piece_to_id("<0x%02X>" % b) for b in range(256)] == table.tolist()
    assert dm.is_byte(3) and not dm.is_byte(2) and not dm.is_byte(3 + 256)
    assert S.DeviceModel(mb.model(mb.base_pieces() + PIECES), host_only=True).byte_fallback() is None


def test_host_only_handle_types_and_vocabulary(fixture):
    name, mbytes, sp = fixture
    dm = S.DeviceModel(mbytes, host_only=True)
    bids = R.byte_ids(mbytes)
    types = dm.piece_types()
    assert (types[bids] == R.BYTE).all() and int((types == R.BYTE).sum()) == 256
    assert [i for i in range(len(types)) if sp.is_byte(i)] == sorted(bids)
    assert dm.decode_bound() >= 4
    # The vocabulary calls leave BYTE pieces alone (this engine's rule).
    dm.set_vocabulary([b"<0x41>", WS.encode() + b"the"])
    after = dm.piece_types()
    assert (after[bids] == R.BYTE).all() and int((after == mb.UNUSED).sum()) > 0
    dm.reset_vocabulary()
    assert np.array_equal(dm.piece_types(), types)
    bad = types.copy()
    bad[bids[0x41]] = mb.NORMAL
    with pytest.raises(S.SpmError):
        dm.set_piece_types(bad)
    assert np.array_equal(dm.piece_types(), types)
