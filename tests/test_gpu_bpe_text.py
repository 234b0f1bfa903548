"""GPU: BPE Encode of real text (csrc/bpe_words.hip) against the CPU oracle.

The flagged sentences (over 64 bytes, or refused by a first kernel) go to the
word tier (word-closed models: words encoded one per lane), the wave tier
(one sentence per wave, <= 1024 bytes) or the literal kernel; ids, piece
lengths and token offsets must be the oracle's bit for bit, and
bpe_tier_stats() must count what bpe_text_cases.predict() derives from the
tiers' rules."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import bpe_cases as C
import bpe_text_cases as T
import byte_fallback_ref as R
import oracle_lib as O
import spm_amd as S

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _check(dm, om, sents):
    """Encodes on the device, requires the oracle's output; returns (general_path, tier stats)."""
    buf, off = S.to_csr(sents)
    ids, lens, to = dm.encode_csr_host(buf, off, with_lens=True)
    gp, tiers = dm.stats().general_path, dm.bpe_tier_stats()
    oids, olens, oto = om.encode_normalized_csr(buf, off, with_lens=True)
    assert np.array_equal(to, oto)
    bad = np.nonzero(ids != oids)[0]
    assert bad.size == 0, "ids differ first in sentence %d" % (int(np.searchsorted(oto, bad[0], side="right")) - 1)
    assert np.array_equal(lens, olens)
    assert sum(tiers) == gp
    return gp, tiers


@pytest.mark.parametrize("name", ["botchan_bpe1k", "botchan_bf_bpe1k"])
def test_botchan_lines_take_the_word_tier(name):
    mb = open(os.path.join(GOLD, name + ".model"), "rb").read()
    dm = S.DeviceModel(mb)
    assert dm.bpe_word_closed()
    norm = dm.normalize(R.corpus_lines("botchan.txt")[:600])
    gp, (word, wave, literal) = _check(dm, O.OracleModel(mb), norm)
    assert literal == 0 and wave == 0 and word == gp > 0


def test_wagahaiwa_giant_words():
    """Japanese lines under the byte-fallback model: a line is one or a few
    giant words, each encoded by the whole wave inside the word tier.  Only a
    line with a word of more than 1024 bytes reaches the literal kernel (74 of
    the 75 lines over 1024 bytes: one of them is made of shorter words)."""
    mb = R.fixture_model("botchan_bf_bpe1k")
    dm = S.DeviceModel(mb)
    lines = R.corpus_lines("wagahaiwa_nekodearu.txt")[:300]
    off, ids, _, _ = R.recorded_spt("wagahaiwa", "botchan_bf_bpe1k")
    got = dm.encode_lines_device(lines)
    assert [x for r in got for x in r] == ids[:int(off[300])].tolist()
    norm = dm.normalize(lines)
    want = sum(any(len(w) > T.WAVE_BYTES for w in T.words(s)) for s in norm)
    assert 0 < want <= sum(len(s) > T.WAVE_BYTES for s in norm)
    word, wave, literal = dm.bpe_tier_stats()
    assert (wave, literal) == (0, want) and word + literal == dm.stats().general_path


@pytest.fixture(scope="module")
def hand():
    mb = T.hand_model()
    return S.DeviceModel(mb), O.OracleModel(mb)


@pytest.mark.parametrize("arrangement", ["shuffled", "flagged_first"])
def test_hand_model_edges(hand, arrangement):
    dm, om = hand
    assert dm.bpe_word_closed()
    sents = T.edge_sentences() * 6 + [b"ab", T.W + b"abc", b"", T.W + b"de" * 9] * 40
    random.Random(5).shuffle(sents)
    if arrangement == "flagged_first":  # the lane kernel's first tile holds only flagged sentences
        sents.sort(key=lambda s: T.predict(s) is None)
        assert all(T.predict(s) for s in sents[:C.TILE])
    gp, tiers = _check(dm, om, sents)
    want = [T.predict(s) for s in sents]
    assert tiers == tuple(want.count(t) for t in ("word", "wave", "literal"))
    assert min(tiers) > 0 and gp < len(sents)


def test_model_that_is_not_word_closed():
    spec = C.build_model()
    dm = S.DeviceModel(spec.blob)
    assert not dm.bpe_word_closed()
    sents = C.batch("shuffled") + [b"ab" * 512, b"ab" * 513, "あ".encode() * 342]
    gp, (word, wave, literal) = _check(dm, O.OracleModel(spec.blob), sents)
    assert gp == C.flagged_count(sents, C.TIER_LANE_AFFINE)
    assert word == 0 and wave > 0
    assert literal == sum(len(s) > T.WAVE_BYTES for s in sents)


_CHILD = """
import sys
sys.path[:0] = [%r, %r]
import numpy as np, spm_amd as S, bpe_text_cases as T
dm = S.DeviceModel(T.hand_model())
ids, to = dm.encode_csr_host(*S.to_csr(T.edge_sentences()))
print(dm.stats().general_path, *dm.bpe_tier_stats())
print(" ".join(map(str, ids.tolist())))
"""


def test_knob_restores_the_literal_routing(hand):
    dm, _ = hand
    ids, _ = dm.encode_csr_host(*S.to_csr(T.edge_sentences()))
    env = dict(os.environ, SPM_HIP_BPE_TEXT="0")
    p = subprocess.run([sys.executable, "-c", _CHILD % (os.path.dirname(S.__file__), os.path.dirname(__file__))],
                       env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    head, row = p.stdout.strip().split("\n")
    gp, word, wave, literal = map(int, head.split())
    assert (word, wave) == (0, 0) and literal == gp > 0
    assert row.split() == [str(x) for x in ids.tolist()]
