"""Shared inputs of the WORD / CHAR tests: the fixture models of
tools/make_wordchar_golden.py with their golden rows, and the known answers of
the reference's own tests, transcribed as data (test infrastructure)."""
import gzip
import os

import model_builder as MB
import model_reader
import oracle_lib
import wordchar_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
WS = "▁".encode()

# (fixture name, corpus, model type)
FIXTURES = (
    ("botchan_char60", "botchan.txt", R.CHAR),
    ("wagahaiwa_char2000", "wagahaiwa_nekodearu.txt", R.CHAR),
    ("botchan_word2000", "botchan.txt", R.WORD),
)

_cache = {}


def model_bytes(name):
    return open(os.path.join(GOLD, name + ".model"), "rb").read()


def corpus(name):
    corpus_file = dict((f[0], f[1]) for f in FIXTURES)[name]
    key = ("lines", corpus_file)
    if key not in _cache:
        _cache[key] = oracle_lib.read_lines_binary(os.path.join(GOLD, corpus_file))
    return _cache[key]


def ref_model(name):
    key = ("ref", name)
    if key not in _cache:
        kind = dict((f[0], f[2]) for f in FIXTURES)[name]
        _cache[key] = R.Model(model_reader.read_pieces(model_bytes(name)), kind)
    return _cache[key]


def _gz_lines(name, suffix):
    key = (name, suffix)
    if key not in _cache:
        data = gzip.open(os.path.join(GOLD, name + suffix), "rb").read().decode("utf-8")
        rows = data.split("\n")
        assert rows[-1] == ""
        _cache[key] = rows[:-1]
    return _cache[key]


def golden_ids(name, suffix=".ids.gz"):
    return [[int(x) for x in row.split()] for row in _gz_lines(name, suffix)]


def golden_pieces(name):
    return [row.split("\t") if row else [] for row in _gz_lines(name, ".pieces.gz")]


def golden_decoded(name):
    return _gz_lines(name, ".decoded.gz")


# ---- the reference's own tests, as data -----------------------------------

def char_test_model():
    """char_model_test.cc EncodeTest: ids 3.. = ▁ a b c d ABC(USER_DEFINED)."""
    return MB.base_pieces() + [(WS, 0.0, MB.NORMAL), ("a", 0.1, MB.NORMAL), ("b", 0.2, MB.NORMAL),
                               ("c", 0.3, MB.NORMAL), ("d", 0.4, MB.NORMAL), ("ABC", 0.4, MB.USER_DEFINED)]


CHAR_KAT = (
    (b"", []),
    (WS + b"a" + WS + b"b" + WS + b"c", [WS, b"a", WS, b"b", WS, b"c"]),
    (WS + b"ab" + WS + b"cd" + WS + b"abc", [WS, b"a", b"b", WS, b"c", b"d", WS, b"a", b"b", b"c"]),
    ("あ".encode()[:1], ["あ".encode()[:1]]),  # broken UTF-8: one piece
    (WS + b"abABCcd", [WS, b"a", b"b", b"ABC", b"c", b"d"]),
)


def word_test_model():
    """word_model_test.cc EncodeTest."""
    return MB.base_pieces() + [(WS + w.encode(), s, MB.NORMAL) for w, s in
                               (("ab", 0.0), ("cd", 0.0), ("abc", 0.0), ("a", 0.1), ("b", 0.2), ("c", 0.3),
                                ("d", 0.4))]


WORD_KAT = (
    (b"", []),
    (WS + b"a" + WS + b"b" + WS + b"c", [WS + b"a", WS + b"b", WS + b"c"]),
    (WS + b"ab" + WS + b"cd" + WS + b"abc", [WS + b"ab", WS + b"cd", WS + b"abc"]),
)

# model_interface_test.cc SplitIntoWordsTest / SplitIntoWordsSuffixTest and the
# words word_model_trainer_test.cc counts: (text, suffix mode, words).
SPLIT_KAT = (
    (WS + b"this" + WS + b"is" + WS + b"a" + WS + b"pen", False, [WS + b"this", WS + b"is", WS + b"a", WS + b"pen"]),
    (b"this" + WS + b"is" + WS + b"a" + WS + b"pen", False, [b"this", WS + b"is", WS + b"a", WS + b"pen"]),
    (WS + b"this" + WS + WS + b"is", False, [WS + b"this", WS, WS + b"is"]),
    (b"", False, []),
    (b"hello", False, [b"hello"]),
    (b"this" + WS + b"is" + WS + b"a" + WS + b"pen" + WS, True, [b"this" + WS, b"is" + WS, b"a" + WS, b"pen" + WS]),
    (b"this" + WS + b"is" + WS + b"a" + WS + b"pen", True, [b"this" + WS, b"is" + WS, b"a" + WS, b"pen"]),
    (WS + b"this" + WS + WS + b"is", True, [WS, b"this" + WS, WS, b"is"]),
    (b"", True, []),
    (b"hello", True, [b"hello"]),
    (WS + b"I" + WS + b"have" + WS + b"a" + WS + b"pen", False, [WS + b"I", WS + b"have", WS + b"a", WS + b"pen"]),
)

# char_model_trainer_test.cc BasicTest: identity normalization, dummy prefix.
TRAIN_LINES = ("I have a pen", "I have an apple", "apple pen")
TRAIN_KAT = ((100, "▁ a e p n I h l v"), (5, "▁ a"))
