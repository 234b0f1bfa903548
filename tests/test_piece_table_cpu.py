"""The byte kernel's piece -> (id, node score) table, on host-only handles.

spm_hip_model_piece_lookup runs the kernel's hash and probe sequence over the
host copy of the table the writing backtrace reads instead of re-walking the
trie.  The table must answer exactly what the walk answers: the id and node
score of every usable trie node, a miss for everything else.
"""
import os

import numpy as np
import pytest

import model_reader
import oracle_lib as O
import spm_amd as S
from model_builder import CONTROL, NORMAL, UNIGRAM, UNKNOWN, UNUSED, USER_DEFINED, base_pieces, model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = [os.path.join(ROOT, "data", "synth32k_unigram.model"),
          os.path.join(ROOT, "tests", "golden", "test_model.model")]


def _key(p):
    """The trie's C-string key of a piece."""
    return p.split(b"\0")[0]


def _chars(b):
    return len(b.decode("utf-8", errors="replace"))


def _expected(pieces):
    """key -> (id, float32 node score) of the usable pieces, as
    unigram::Model builds its trie (first piece of a duplicated key wins)."""
    f32 = np.float32
    max_score = f32(np.finfo(np.float32).tiny)  # FLT_MIN, unigram_model.cc:683
    for p, s, t in pieces:
        if t == NORMAL:
            max_score = max(max_score, f32(s))
    out = {}
    for i, (p, s, t) in enumerate(pieces):
        if t in (UNKNOWN, CONTROL):
            continue
        k = _key(p)
        if not k or k in out:
            continue
        if t == NORMAL:
            out[k] = (i, f32(s))
        elif t == USER_DEFINED:
            out[k] = (i, f32(np.float64(f32(_chars(k)) * max_score) + 1.0))
        else:
            out[k] = None  # UNUSED: in the trie, never a lattice node
    return out


@pytest.fixture(scope="module", params=MODELS, ids=lambda p: os.path.basename(p))
def loaded(request):
    mb = open(request.param, "rb").read()
    pieces = model_reader.read_pieces(mb)
    dm = S.DeviceModel(mb, host_only=True)
    assert dm.info().fast_variant == 1  # a byte-kernel model
    return mb, pieces, _expected(pieces), dm


def test_every_usable_piece_is_found(loaded):
    mb, pieces, exp, dm = loaded
    usable = {k: v for k, v in exp.items() if v is not None}
    assert len(usable) > 900
    for k, (i, s) in usable.items():
        got = dm.piece_lookup(k)
        assert got is not None, k
        assert got[0] == i and np.float32(got[1]) == s, k


def test_single_token_pieces_match_the_oracle(loaded):
    """Where the oracle encodes a piece's own bytes as one token, that token's
    id is the table's."""
    mb, pieces, exp, dm = loaded
    keys = [k for k, v in exp.items() if v is not None]
    buf, off = S.to_csr(keys)
    ids, to = O.OracleModel(mb).encode_normalized_csr(buf, off, threads=8)
    single = 0
    for n, k in enumerate(keys):
        if int(to[n + 1]) - int(to[n]) == 1:
            single += 1
            assert dm.piece_lookup(k)[0] == int(ids[int(to[n])]), k
    assert single > len(keys) // 2


def test_unused_and_reserved_pieces_miss(loaded):
    mb, pieces, exp, dm = loaded
    for p, s, t in pieces:
        if t in (UNKNOWN, CONTROL) and _key(p) not in exp:
            assert dm.piece_lookup(_key(p)) is None, p
    for k, v in exp.items():
        if v is None:
            assert dm.piece_lookup(k) is None, k


def test_non_pieces_miss(loaded):
    mb, pieces, exp, dm = loaded
    usable = sorted(k for k, v in exp.items() if v is not None)
    step = max(1, len(usable) // 2000)
    prefixes = extended = 0
    for k in usable[::step]:
        for n in range(1, len(k)):  # proper prefixes that are no piece themselves
            if exp.get(k[:n]) is None:
                prefixes += 1
                assert dm.piece_lookup(k[:n]) is None, k[:n]
        for c in (b"a", b"\x01", b"\xff", b"\x80"):
            if len(k) < 15 and exp.get(k + c) is None:
                extended += 1
                assert dm.piece_lookup(k + c) is None, k + c
        assert dm.piece_lookup(k + b"\0") is None, k
        assert dm.piece_lookup(k[:1] + b"\0" + k[1:]) is None, k
    assert prefixes > 100 and extended > 100
    assert dm.piece_lookup(b"") is None
    long15 = b"qzqzqzqzqzqzqzq"
    assert len(long15) == 15 and long15 not in exp
    assert dm.piece_lookup(long15) is None
    assert dm.piece_lookup(long15 + b"q") is None  # 16 bytes: no key is that long
    assert dm.piece_lookup(usable[0] + b"\0" * 20) is None


def test_fifteenth_byte_resolves():
    """Two pieces that differ only in their 15th byte, a USER_DEFINED and an
    UNUSED piece, and a piece with an embedded NUL (its key ends there)."""
    stem = b"abcdefghijklmn"
    pieces = base_pieces() + [
        (stem + b"X", -1.5, NORMAL), (stem + b"Y", -2.5, NORMAL), ("a", -3.0, NORMAL),
        ("<tag>", 0.0, USER_DEFINED), ("abc", -0.5, UNUSED), (b"ab\0zz", -4.0, NORMAL),
        ("日本", -6.0, NORMAL),
    ]
    dm = S.DeviceModel(model(pieces, UNIGRAM), host_only=True)
    assert dm.info().fast_variant == 1
    f32 = np.float32
    assert dm.piece_lookup(stem + b"X") == (3, -1.5)
    assert dm.piece_lookup(stem + b"Y") == (4, -2.5)
    assert dm.piece_lookup(stem) is None and dm.piece_lookup(stem + b"Z") is None
    assert dm.piece_lookup(b"a") == (5, -3.0)
    # USER_DEFINED: chars * max_score + 1; max_score starts at FLT_MIN
    # (unigram_model.cc:683) and every NORMAL score here is below it
    assert dm.piece_lookup(b"<tag>") == (6, float(f32(np.float64(f32(5) * f32(np.finfo(f32).tiny)) + 1.0)))
    assert dm.piece_lookup(b"abc") is None
    assert dm.piece_lookup(b"ab") == (8, -4.0)  # the key of "ab\0zz"
    assert dm.piece_lookup(b"ab\0zz") is None and dm.piece_lookup(b"ab\0") is None
    assert dm.piece_lookup("日本".encode()) == (9, -6.0)
    assert dm.piece_lookup("日".encode()) is None


def test_models_of_other_kernels_have_no_table():
    mb = open(os.path.join(ROOT, "tests", "golden", "test_ja_model.model"), "rb").read()
    dm = S.DeviceModel(mb, host_only=True)
    assert dm.info().fast_variant != 1
    with pytest.raises(S.SpmError) as e:
        dm.piece_lookup(b"a")
    assert e.value.code == 9  # FAILED_PRECONDITION
