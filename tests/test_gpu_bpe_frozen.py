"""GPU: BPE Encode of models with user-defined symbols (csrc/bpe_frozen.hip)
against the CPU oracle.

Every sentence is flagged (general_path == the batch); ids, piece lengths and
token offsets must be the oracle's, and bpe_frozen_stats() must count what the
tier's rules give: it takes a sentence of <= 1024 bytes whose OneCharLen walk
is its non-continuation bytes and that pushes no UNUSED piece, and hands the
others to the literal kernel.  set_piece_types exchanges NORMAL and UNUSED
only (test_vocab_cpu.py pins that), so no USER_DEFINED piece can be re-tagged
on a handle: the retag case re-tags a NORMAL piece beside the symbols."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bpe_cases as C
import model_reader
import oracle_lib as O
import spm_amd as S
import vocab_ref
from model_builder import BPE, NORMAL, UNUSED, USER_DEFINED, model

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# bpe_cases' pieces, the symbols' chars (the model stays regular), one UNUSED merge, the symbols.
SYMBOLS = ["<t", "<tag>", "<tag>>", "aé€", "b▁<"]
PIECES = (C.build_model().pieces + [(c, -2000.0 - k, NORMAL) for k, c in enumerate("<t>€")] +
          [("gt", -0.5, UNUSED)] + [(u, 0.0, USER_DEFINED) for u in SYMBOLS])
TAG = b"<tag>"
SENTS = [
    b"", TAG, TAG + b"abc", b"abc" + TAG, TAG + TAG, b"ab" + TAG + b"cd" + TAG + b"ef",
    b"<<tag>", b"<tag<tag>", b"ab<tab", b"ab<tag>ab", b"ab<tag>>ab", b"<tag>>>", b"<",
    "abaé€ab".encode(), "aéab".encode(), "aaé€€".encode(), "ab▁<tag>ab▁<".encode(),
    b"ab" * 30 + b"<tag>>ab",                  # a match from byte 60 to byte 66
    b"ab" * 29 + b"a" + TAG + TAG + b"ab",     # a match that ends on byte 64, the next starts there
    b"a" * 62 + TAG + TAG, b"ab" * 31 + b"<tag<tag>",
    (TAG + b"abc") * 16, (TAG + b"abc") * 16 + b"a",      # 128 and 129 bytes: the two launches
    (TAG + b"abc") * 128, (TAG + b"abc") * 128 + b"a",    # 1024 bytes (taken) and 1025 (literal)
    b"ab<ta\x00g>ab", b"<t\x00ag>", b"\x00" + TAG,        # a NUL byte ends the trie walk
    b"ab\xf0<tag>ab", b"\x80" + TAG, TAG + b"\xc3",       # walk-irregular (handed on); a cut char last is regular
    TAG + b"gt", b"gt" + TAG, b"g" + TAG + b"t",          # the UNUSED piece pushed next to a symbol (handed on), and not
]


def taken(s, unused=b"gt"):
    """unused: the model's one UNUSED piece, pushed wherever its two chars meet."""
    regular = C.walk_starts(s) == [q for q, b in enumerate(s) if (b & 0xC0) != 0x80]
    return regular and len(s) <= 1024 and not (unused and unused in s)


def check(dm, om, sents, host=True, unused=b"gt"):
    """One Encode; the oracle's output and the counts of the tier's rules."""
    buf, off = S.to_csr(sents)
    if host:
        ids, lens, to = dm.encode_csr_host(buf, off, with_lens=True)
    else:
        n, cap = len(sents), max(len(buf), 1)
        d = [torch.from_numpy(x.view(t)).cuda() for x, t in ((buf, np.uint8), (off, np.int64))]
        o = [torch.zeros(k, dtype=t, device="cuda") for k, t in ((cap, torch.int32), (cap, torch.int32), (n + 1, torch.int64))]
        dm.encode_device(d[0].data_ptr(), d[1].data_ptr(), n, o[0].data_ptr(), o[2].data_ptr(), d_len=o[1].data_ptr())
        to = o[2].cpu().numpy().view(np.uint64)
        ids, lens = (x.cpu().numpy()[:int(to[-1])] for x in o[:2])
        lens = lens.view(np.uint32)
    oids, olens, oto = om.encode_normalized_csr(buf, off, with_lens=True)
    assert np.array_equal(to, oto)
    bad = np.nonzero(ids != oids)[0]
    assert bad.size == 0, "ids differ first in sentence %d" % (int(np.searchsorted(oto, bad[0], side="right")) - 1)
    assert np.array_equal(lens, olens)
    want = sum(taken(s, unused) for s in sents)
    assert dm.stats().general_path == len(sents)
    assert dm.bpe_frozen_stats() == (want, len(sents) - want)
    return ids


@pytest.fixture(scope="module")
def hand():
    mb = model(PIECES, BPE)
    dm = S.DeviceModel(mb)
    assert dm.info().fast_variant == C.TIER_GENERAL
    return dm, O.OracleModel(mb)


@pytest.mark.parametrize("batch", [1, 129])
def test_hand_model(hand, batch):
    dm, om = hand
    assert [len(s) for s in SENTS[21:25]] == [128, 129, 1024, 1025] and not all(map(taken, SENTS))
    if batch == 1:
        for s in SENTS:
            check(dm, om, [s])
    else:
        check(dm, om, (SENTS * 4)[5:5 + batch])


@pytest.mark.parametrize("kw", [dict(irregular=True), dict(unused=True), dict(pad_to=32768)])
def test_bpe_cases_pool(kw):
    """bpe_cases' pool and model: an irregular vocabulary, UNUSED merges, ids past 16 bits."""
    spec = C.build_model(user_defined=True, **kw)
    dm, om = S.DeviceModel(spec.blob), O.OracleModel(spec.blob)
    sents = [s + TAG + s[:7] if k % 3 else s for k, s in enumerate(C.pool())]
    buf, off = S.to_csr(sents)
    ids, lens, to = dm.encode_csr_host(buf, off, with_lens=True)
    oids, olens, oto = om.encode_normalized_csr(buf, off, with_lens=True)
    assert np.array_equal(to, oto) and np.array_equal(ids, oids) and np.array_equal(lens, olens)
    t, h = dm.bpe_frozen_stats()
    assert t + h == len(sents) == dm.stats().general_path and t > 0
    assert h >= sum(not taken(s, None) for s in sents)


@pytest.mark.parametrize("host", [True, False])
def test_botchan_with_spliced_symbols(host):
    mb0 = open(os.path.join(GOLD, "botchan_bpe1k.model"), "rb").read()
    pieces = model_reader.read_pieces(mb0) + [("<tag>", 0.0, USER_DEFINED), ("<mask>", 0.0, USER_DEFINED)]
    mb = model(pieces, BPE, charsmap=model_reader.charsmap(mb0))
    dm, om = S.DeviceModel(mb), O.OracleModel(mb)
    sents = []
    for line in dm.normalize(O.read_lines_binary(os.path.join(GOLD, "botchan.txt"))[:300]):
        words = line.split("▁".encode())
        for k in range(7, len(words), 7):
            words[k] = (b"<mask>" if k % 2 else TAG) + words[k]
        sents.append("▁".encode().join(words))
    assert sum(TAG in s for s in sents) > 50
    check(dm, om, sents, host, unused=None)


_CHILD = """
import sys
sys.path[:0] = [%r, %r]
import spm_amd as S, test_gpu_bpe_frozen as T
from model_builder import BPE, model
dm = S.DeviceModel(model(T.PIECES, BPE))
ids, to = dm.encode_csr_host(*S.to_csr(T.SENTS))
print(dm.stats().general_path, *dm.bpe_frozen_stats())
print(" ".join(map(str, ids.tolist())))
"""


def test_knob_restores_the_host_sized_pass(hand):
    dm, om = hand
    ids = check(dm, om, SENTS)
    env = dict(os.environ, SPM_HIP_BPE_FROZEN="0")
    p = subprocess.run([sys.executable, "-c", _CHILD % (os.path.dirname(S.__file__), os.path.dirname(__file__))],
                       env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    head, row = p.stdout.strip().split("\n")
    assert list(map(int, head.split())) == [len(SENTS), 0, 0]
    assert row.split() == [str(x) for x in ids.tolist()]


def test_retag_next_to_a_symbol():
    """"ab" UNUSED and NORMAL again: the oracle on the retagged proto both times."""
    mb = model(PIECES, BPE)
    dm = S.DeviceModel(mb)
    t0 = dm.piece_types()
    t1 = t0.copy()
    t1[[p for p, _, _ in PIECES].index("ab")] = UNUSED
    for types in (t1, t0):
        dm.set_piece_types(types)
        om = O.OracleModel(vocab_ref.retype(mb, types))
        buf, off = S.to_csr(SENTS)
        ids, lens, to = dm.encode_csr_host(buf, off, with_lens=True)
        oids, olens, oto = om.encode_normalized_csr(buf, off, with_lens=True)
        assert np.array_equal(to, oto) and np.array_equal(ids, oids) and np.array_equal(lens, olens)
        assert sum(dm.bpe_frozen_stats()) == len(SENTS)
    assert dm.bpe_frozen_stats()[0] == sum(map(taken, SENTS))
