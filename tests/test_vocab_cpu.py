"""CPU: SetVocabulary / ResetVocabulary / LoadVocabulary on host-only handles
(spm_hip_model_set_piece_types and the processor's three calls through
lib/vocab_selftest --host) against the restatement tests/vocab_ref.py: the
reference's VocabularyTest table, LoadVocabulary's parsing and errors, the
state the engine re-derives after a type change (tier, piece lengths, piece
table) and the state it must keep (the load-time scores)."""
import os
import subprocess

import numpy as np
import pytest

import vocab_ref as V
from model_builder import CONTROL, NORMAL, UNIGRAM, UNKNOWN, UNUSED, USER_DEFINED, base_pieces, model
from model_reader import read_pieces

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SELFTEST = os.path.join(ROOT, "sentencepiece-comments_amd", "lib", "vocab_selftest")
WORD, CHAR = 3, 4

# sentencepiece_processor_test.cc:1120-1220: the model and, per step, IsUnused of ids 0..7.
VOCAB_PIECES = base_pieces() + [(p, 0.0, NORMAL) for p in ("aa", "bb", "cc", "dd", "e")]
VOCAB_STEPS = [
    (None, [0, 0, 0, 0, 0, 0, 0, 0]),
    (("set", ["aa", "dd", "e"]), [0, 0, 0, 0, 1, 1, 0, 0]),
    (("reset",), [0, 0, 0, 0, 0, 0, 0, 0]),
    (("set", ["bb"]), [0, 0, 0, 1, 0, 1, 1, 0]),
    (("load", b"aa\t1\ndd\t2\n", 2), [0, 0, 0, 1, 1, 1, 0, 0]),
    (("load", b"aa\t1\ndd\t1\n", 2), [0, 0, 0, 1, 1, 1, 1, 0]),
    (("load", b"aa\t1\ndd\t1\n", 1), [0, 0, 0, 0, 1, 1, 0, 0]),
    (("load", b"aa\t0\ndd\t0\n", 0), [0, 0, 0, 0, 1, 1, 0, 0]),
    (("load", b"aa\ndd\n", 1), [0, 0, 0, 0, 1, 1, 0, 0]),  # no frequency: 1
]


@pytest.fixture(scope="module")
def S():
    import spm_amd
    spm_amd.lib()
    return spm_amd


def _selftest(tmp_path, model_bytes, commands):
    path = tmp_path / "m.model"
    path.write_bytes(model_bytes)
    p = subprocess.run([SELFTEST, str(path), "--host"], input="".join(c + "\n" for c in commands).encode(),
                       capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    return p.stdout.decode().splitlines()


def test_vocabulary_test_restatement():
    types = [t for _, _, t in VOCAB_PIECES]
    for step, want in VOCAB_STEPS:
        if step is None:
            pass
        elif step[0] == "set":
            types = V.set_vocabulary(VOCAB_PIECES, step[1])
        elif step[0] == "reset":
            types = V.reset_vocabulary(types)
        else:
            types = V.set_vocabulary(VOCAB_PIECES, V.parse_vocabulary(step[1], step[2]))
        assert [int(t == UNUSED) for t in types] == want, step


def test_vocabulary_test_processor(tmp_path):
    cmds, wants = [], []
    for k, (step, want) in enumerate(VOCAB_STEPS):
        if step is None:
            pass
        elif step[0] == "set":
            cmds.append("\t".join(["set"] + step[1]))
        elif step[0] == "reset":
            cmds.append("reset")
        else:
            f = tmp_path / ("vocab%d.txt" % k)
            f.write_bytes(step[1])
            cmds.append("load\t%s\t%d" % (f, step[2]))
        cmds.append("unused")
        wants.append(want)
    out = _selftest(tmp_path, model(VOCAB_PIECES), cmds)
    assert [l for l in out if l != "ok" and not l.startswith("unused")] == []
    got = [[int(x) for x in l.split()[1:]] for l in out if l.startswith("unused")]
    assert got == wants


def test_vocabulary_test_handle(S):
    d = S.DeviceModel(model(VOCAB_PIECES), host_only=True)
    types = [t for _, _, t in VOCAB_PIECES]
    for step, want in VOCAB_STEPS:
        if step is None:
            pass
        elif step[0] == "set":
            d.set_vocabulary(step[1])
        elif step[0] == "reset":
            d.reset_vocabulary()
        else:
            d.set_vocabulary(V.parse_vocabulary(step[1], step[2]))
        assert [int(t == UNUSED) for t in d.piece_types()] == want, step
    assert d.piece_types()[:3].tolist() == types[:3]


def test_load_vocabulary_errors(tmp_path):
    empty_line, lead_tab = tmp_path / "empty.txt", tmp_path / "tab.txt"
    empty_line.write_bytes(b"aa\t3\n\ndd\t3\n")
    lead_tab.write_bytes(b"\taa\nbb\t\t0\n")  # Split drops empty fields: pieces "aa" (no count) and "bb" (count 0)
    out = _selftest(tmp_path, model(VOCAB_PIECES), [
        "load\t%s\t0" % empty_line, "unused",
        "load\t%s\t0" % (tmp_path / "missing.txt"), "unused",
        "load\t%s\t1" % lead_tab, "unused"])
    assert out[0].startswith("error 13 ") and out[2].startswith("error 5 ")
    assert "No such file or directory" in out[2]
    assert out[1] == out[3] == "unused 0 0 0 0 0 0 0 0"  # a failed call changes nothing
    with pytest.raises(ValueError):
        V.parse_vocabulary(empty_line.read_bytes(), 0)
    assert V.parse_vocabulary(lead_tab.read_bytes(), 1) == [b"aa"]
    assert out[4:] == ["ok", "unused 0 0 0 0 1 1 1 0"]


@pytest.mark.parametrize("model_type", [WORD, CHAR])
def test_word_char_refused(tmp_path, S, model_type):
    pieces = VOCAB_PIECES[:-1] + [("ee", 0.0, UNUSED)]
    mb = model(pieces, model_type)
    out = _selftest(tmp_path, mb, ["set\taa", "unused", "reset", "unused"])
    assert out[0] == "error 13 Vocabulary constraint is only enabled in subword units."
    assert out[1] == "unused 0 0 0 0 0 0 0 1"
    assert out[2:] == ["ok", "unused 0 0 0 0 0 0 0 0"]  # ResetVocabulary works on any model type
    d = S.DeviceModel(mb, host_only=True)
    with pytest.raises(S.SpmError) as e:
        d.set_vocabulary(["aa"])
    assert e.value.code == 13


def test_set_piece_types_rejections(S):
    pieces = VOCAB_PIECES + [("<u>", 0.0, USER_DEFINED)]
    d = S.DeviceModel(model(pieces), host_only=True)
    t0 = d.piece_types()
    bad = []
    for i, new in ((0, NORMAL), (1, UNUSED), (8, NORMAL), (3, CONTROL), (3, UNKNOWN), (3, USER_DEFINED), (3, 0)):
        t = t0.copy()
        t[i] = new
        bad.append(t)
    bad += [t0[:-1], np.concatenate([t0, [NORMAL]]).astype(np.uint8)]
    for t in bad:
        with pytest.raises(S.SpmError) as e:
            d.set_piece_types(t)
        assert e.value.code == 3
        assert d.piece_types().tolist() == t0.tolist()
    t = t0.copy()
    t[3] = UNUSED
    d.set_piece_types(t)
    assert d.piece_types().tolist() == t.tolist()


def _state(inf):
    return (inf.fast_variant, inf.ring_width, inf.max_piece_chars)


def _check_piece_table(S, d, pieces, types, max_score):
    """piece_lookup finds every usable piece of <= 15 bytes and no other."""
    for (p, sc, _), t in zip(pieces, types):
        p = p if isinstance(p, bytes) else p.encode()
        got = d.piece_lookup(p)
        if t == NORMAL and len(p) <= 15:
            assert got is not None and got[1] == np.float32(sc), p
        elif t == USER_DEFINED and len(p) <= 15:
            assert got is not None and got[1] == np.float32(len(p.decode()) * max_score + 1.0), p
        else:
            assert got is None, p


def test_reset_vocabulary_and_the_tiers(S):
    """A piece of 20 bytes that is UNUSED in the file: the model loads into
    the byte tier; ResetVocabulary makes the piece live and the tier, ring
    and max_piece_chars must be those of a model with that piece; dropping
    it again gives the original ones back."""
    long_piece = "abcdefghijklmnopqrst"
    pieces = base_pieces() + [("a", -1.0, NORMAL), ("ab", -2.0, NORMAL), ("abc", -3.5, NORMAL), ("b", -1.5, NORMAL),
                              ("<u>", 0.0, USER_DEFINED), (long_piece, -4.0, UNUSED), ("bc", -2.5, UNUSED)]
    mb = model(pieces)
    d = S.DeviceModel(mb, host_only=True)
    at_load = _state(d.info())
    assert at_load[0] == 1 and at_load[2] == 3   # byte kernel; "abc" and "<u>"
    types = [t for _, _, t in pieces]
    _check_piece_table(S, d, pieces, types, d.info().max_score)
    d.reset_vocabulary()
    types = V.reset_vocabulary(types)
    assert d.piece_types().tolist() == types
    fresh = S.DeviceModel(V.retype(mb, types), host_only=True)
    assert _state(d.info()) == _state(fresh.info())
    assert d.info().fast_variant != 1 and d.info().max_piece_chars == 20
    with pytest.raises(S.SpmError) as e:   # no byte kernel, no piece table
        d.piece_lookup(b"a")
    assert e.value.code == 9
    d.set_vocabulary(["ab", "abc"])
    types = V.set_vocabulary(pieces, ["ab", "abc"])
    assert d.piece_types().tolist() == types and types[-2:] == [UNUSED, UNUSED]
    assert _state(d.info()) == at_load
    _check_piece_table(S, d, pieces, types, d.info().max_score)
    d.set_vocabulary(["bc"])
    types = V.set_vocabulary(pieces, ["bc"])
    assert _state(d.info()) == (1, 16, 3)   # "<u>" still counts
    _check_piece_table(S, d, pieces, types, d.info().max_score)


def test_piece_table_follows_on_a_trained_model(S):
    mb = open(os.path.join(GOLD, "test_model.model"), "rb").read()
    pieces = read_pieces(mb)
    d = S.DeviceModel(mb, host_only=True)
    max_score = d.info().max_score
    vocab = [p for k, (p, _, t) in enumerate(pieces) if t == NORMAL and k % 3 == 0]
    for step in (vocab, None, vocab[::2]):
        if step is None:
            d.reset_vocabulary()
            types = V.reset_vocabulary(d.piece_types().tolist())
        else:
            d.set_vocabulary(step)
            types = V.set_vocabulary(pieces, step)
        assert d.piece_types().tolist() == types
        _check_piece_table(S, d, pieces, types, max_score)


# The frozen-min_score model of the GPU test: see test_gpu_vocab.py.
FROZEN_PIECES = base_pieces() + [("a", 12.0, NORMAL), ("b", -3.0, NORMAL), ("xa", -2.0, NORMAL), ("zz", -20.0, NORMAL)]


def test_frozen_scores(S):
    """SetVocabulary keeps the scores the model took at load: min_score stays
    -20 (unknown score -30) although "zz" is UNUSED afterwards; the
    restatement shows that this decides the segmentation of "xa"."""
    mb = model(FROZEN_PIECES, UNIGRAM, add_dummy_prefix=False)
    d = S.DeviceModel(mb, host_only=True)
    before = (d.info().min_score, d.info().max_score)
    assert before == (-20.0, 12.0)
    d.set_vocabulary(["xa"])
    types = V.set_vocabulary(FROZEN_PIECES, ["xa"])
    assert d.piece_types().tolist() == types and types[6] == UNUSED
    assert (d.info().min_score, d.info().max_score) == before
    reloaded = S.DeviceModel(V.retype(mb, types), host_only=True)
    assert reloaded.info().min_score == -3.0
    assert V.viterbi(FROZEN_PIECES, types, b"xa", -30.0) == [5]
    assert V.viterbi(FROZEN_PIECES, types, b"xa", -13.0) == [0, 3]


def test_vocabulary_file_order():
    pieces = base_pieces() + [("b", 0.0, NORMAL), ("a", 0.0, NORMAL), ("▁c", 0.0, NORMAL), ("d", 0.0, UNUSED)]
    assert V.vocabulary_file([9, 9, 9, 2, 2, 5, 0], pieces) == "▁c\t5\na\t2\nb\t2\n".encode()
