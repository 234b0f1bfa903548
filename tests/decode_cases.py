"""Models and id batches shared by the decode tests (test infrastructure)."""
import gzip
import os

import numpy as np

import model_builder as mb

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WS = "▁"
T = 1024       # spm_amd.DECODE_TILE_TOKENS
SUB = 256      # spm_amd.DECODE_SUBTILE_TOKENS
LONG = "L" + "0123456789" * 4  # the longest surface of the hand model

# The mock model of the reference's DecodeTest (sentencepiece_processor_test.cc:466-497).
BASE = mb.base_pieces() + [(WS + "ABC", -1.0, mb.NORMAL), (WS + "DE", -1.0, mb.NORMAL), ("F", -1.0, mb.NORMAL),
                           ("G" + WS + "H", -1.0, mb.NORMAL)]
UNK, BOS, EOS, ABC, DE, F, GH = range(7)
# ... and the pieces the hand cases add.
EXTRA = [(WS, -2.0, mb.NORMAL), (WS + WS + "A", -2.0, mb.NORMAL), (WS + "A", -2.0, mb.NORMAL),
         ("x▂y", -2.0, mb.NORMAL), ("H" + WS, -2.0, mb.NORMAL), ("UD", 0.0, mb.USER_DEFINED),
         ("UN", -2.0, mb.UNUSED), (LONG, -3.0, mb.NORMAL), (WS + "▂", -3.0, mb.NORMAL)]
BARE, WSWSA, WSA, LOWER, HWS, UD, UN, LONGID, WSLOWER = range(7, 16)


def with_unk_surface(model_bytes, surface):
    """A second trainer_spec occurrence (it merges) that sets unk_surface, field 44."""
    return model_bytes + mb._ld(2, mb._ld(44, surface))


def base_model(unk_surface=None):
    m = mb.model(BASE)
    return m if unk_surface is None else with_unk_surface(m, unk_surface)


def hand_model(unk_surface=None):
    m = mb.model(BASE + EXTRA)
    return m if unk_surface is None else with_unk_surface(m, unk_surface)


def _pattern(count):
    cycle = [ABC, DE, F, GH, UNK, BARE, WSA, LOWER, HWS, UD, UN, BOS, WSWSA]
    return [cycle[k % len(cycle)] for k in range(count)]


def hand_rows():
    """The smallest shapes at which the decode kernels can go wrong."""
    rows = [
        [ABC], [], [DE, F],                    # an empty sentence between non-empty ones
        [BOS, EOS, BOS],                       # control ids only
        [BOS, BARE, BARE, ABC],                # the empty-text state survives control and bare pieces
        [WSWSA],                               # only one U+2581 is consumed
        [BARE] * 70 + [WSA],                   # the state crosses a wave
        [BARE] * (SUB + 5) + [WSA, WSA],       # ... and a sub-tile
        [BARE] * (T + 5) + [WSA, WSA],         # ... and a tile (another block)
        [UNK], [UNK, ABC], [ABC, UNK, UNK, DE],
        [BARE, UNK, ABC],                      # a non-empty unk_surface ends the state, an empty one does not
        [LOWER], [WSLOWER, WSLOWER],           # U+2582 is not U+2581
        [GH, HWS, GH], [HWS],                  # U+2581 in the middle and at the end
        [UD, UN, UD], [UN],
        [], [],
    ]
    for count in (63, 64, 65, SUB - 1, SUB, SUB + 1, T - 1, T, T + 1, 2 * T + 1):
        rows.append(_pattern(count))
    for at in (SUB - 1, SUB, T - 1, T):        # the longest piece at a tile edge
        rows.append([F] * at + [LONGID, LONGID] + [DE] * 3)
    rows += [[], [ABC], []]                    # trailing empty sentence
    return rows


def to_csr(rows):
    ids = np.array([x for r in rows for x in r], dtype=np.int32)
    off = np.zeros(len(rows) + 1, dtype=np.uint64)
    if rows:
        off[1:] = np.cumsum([len(r) for r in rows], dtype=np.uint64)
    return ids, off


GOLDEN = (("botchan_test_model", "test_model.model"), ("wagahaiwa_test_ja_model", "test_ja_model.model"))


def golden_rows(name):
    return [[int(x) for x in line.split()] for line in open(os.path.join(GOLD, name + ".ids"))]


def golden_texts(name):
    data = gzip.open(os.path.join(GOLD, name + ".decoded.gz"), "rb").read()
    return data.split(b"\n")[:-1]


def golden_model(model):
    return open(os.path.join(GOLD, model), "rb").read()
