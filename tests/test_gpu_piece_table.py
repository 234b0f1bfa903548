"""Byte kernel: the backtrace's piece-table lookup against its trie re-walk.

The writing backtrace of unigram_fast_kernel<16, true> takes each token's id
(and, for near-tie lanes, its node score) from the piece -> (id, score) table;
SPM_HIP_NO_PIECE_TABLE (read at model load) keeps the exact-match trie walk.
Both must give the oracle's ids and piece lengths exactly.  Batches go through
the device-pointer API (the host API serves batches this small with another
kernel).
"""
import numpy as np
import pytest
import torch

import oracle_lib as O
import spm_amd as S
from model_builder import NORMAL, UNIGRAM, UNUSED, USER_DEFINED, base_pieces, model

pytestmark = pytest.mark.gpu

WS = "▁".encode()
P15 = WS + b"abcdefghabcd"  # a 15-byte piece


def _edge_case():
    pieces = base_pieces() + [(WS, -2.0, NORMAL)]
    pieces += [(c, -3.0 - 0.125 * i, NORMAL) for i, c in enumerate("abcdefgh")]
    pieces += [
        ("ab", -4.0, NORMAL), ("abc", -1.0, UNUSED), ("abcd", -7.5, NORMAL), ("cd", -5.0, NORMAL),
        (P15, -9.0, NORMAL), (P15[:14], -8.0, UNUSED), (WS + b"ab", -5.5, NORMAL),
        ("é", -4.5, NORMAL), ("日本", -6.0, NORMAL), ("日", -5.0, NORMAL), (WS + "é".encode(), -6.0, NORMAL),
        ("😀", -7.0, NORMAL), ("<tag>", 0.0, USER_DEFINED), (b"gh\0xx", -4.0, NORMAL),
    ]
    mb = model(pieces, UNIGRAM)
    sents = [
        b"", b"a", b"z", WS, P15, P15 + b"e", P15[:14], P15 * 3, b"abc", b"abcabcd", b"ghgh",
        "é日本日😀".encode(), WS + "éé".encode(), "本".encode(), b"<tag>ab<tag>", b"<ta", b"<tag>",
        # UNK chars of 1-4 bytes, between and next to pieces
        b"z", "ß".encode(), "漢".encode(), "🙂".encode(), "aßb漢c🙂dz".encode(), "zß漢🙂".encode(),
        # input NUL: after a piece, first, last, inside what would be a piece
        b"ab\0cd", b"\0", b"a\0", b"\0a", b"abc\0d", WS + b"abcdefg\0abcd", b"gh\0xx",
        # malformed UTF-8
        b"\xe3\x81", b"a\x80b", "é".encode()[:1] + b"a",
    ]
    # Sentence starts at all four byte alignments, tokens of every length on them.
    for k in range(1, 9):
        sents += [b"a" * k, P15 + b"b" * k, (WS + b"ab") * k]
    rng = np.random.default_rng(3)
    alpha = [b"a", b"b", b"c", b"d", b"e", b"f", b"g", b"h", WS, "é".encode(), "日".encode(), "本".encode(),
             b"z", P15, b"<tag>"]
    while len(sents) < 299:
        sents.append(b"".join(alpha[int(x)] for x in rng.integers(0, len(alpha), int(rng.integers(1, 12)))))
    # The batch ends with a sentence of more than 64 bytes whose last token's
    # 20-byte window is the batch's last bytes (the byte-load tail path).
    sents.append(WS + b"abcdefgh" * 9 + P15)
    return mb, sents


def _near_tie_case():
    """The model and sentences of test_gpu_parity.test_unigram_near_tie_stress
    (every multi-char piece one ulp below, or equal to, the sum of its first
    char and the rest), 299 sentences: lanes with a recorded near-tie resolve
    it in the counting backtrace with the node scores node_of returns."""
    rng = np.random.default_rng(5)
    alpha = "abcdef"
    f32 = np.float32
    sc = {"▁": f32(-1.0)}
    for c in alpha:
        sc[c] = f32(-rng.uniform(1.0, 3.0))
    for L in (2, 3, 4):
        for _ in range(60):
            w = "".join(alpha[int(x)] for x in rng.integers(0, len(alpha), L))
            if w in sc or w[1:] not in sc:
                continue
            tot = f32(sc[w[0]] + sc[w[1:]])
            sc[w] = np.nextafter(tot, f32(-np.inf)) if rng.random() < 0.7 else tot
    mb = model(base_pieces() + [(w, float(v), NORMAL) for w, v in sc.items()], UNIGRAM)
    sents = []
    for _ in range(299):
        L = int(rng.integers(0, 40))
        sents.append(("▁" + "".join(alpha[int(x)] for x in rng.integers(0, len(alpha), L))).encode())
    sents.append("▁".encode() + b"abcdef" * 12)
    return mb, sents


@pytest.fixture(scope="module", params=[_edge_case, _near_tie_case], ids=["edge", "near_tie"])
def case(request):
    mb, sents = request.param()
    assert len(sents) <= 300 and len(sents[-1]) > 64
    buf, off = S.to_csr(sents)
    oids, olens, oto = O.OracleModel(mb).encode_normalized_csr(buf, off, with_lens=True)
    for a in (oids, olens, oto):
        a.setflags(write=False)
    return request.param.__name__, mb, buf, off, oids, olens, oto


def _encode_device(dm, buf, off):
    dev = torch.device("cuda:0")
    n = len(off) - 1
    cap = max(int(off[-1]), 1)
    d_b = torch.from_numpy(buf).to(dev)
    d_o = torch.from_numpy(off.view(np.int64)).to(dev)
    d_ids = torch.full((cap,), -7, dtype=torch.int32, device=dev)
    d_len = torch.zeros(cap, dtype=torch.int32, device=dev)
    d_tok = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    dm.encode_device(d_b.data_ptr(), d_o.data_ptr(), n, d_ids.data_ptr(), d_tok.data_ptr(), d_len=d_len.data_ptr())
    torch.cuda.synchronize()
    to = d_tok.cpu().numpy().view(np.uint64)
    k = int(to[-1])
    return d_ids.cpu().numpy()[:k], d_len.cpu().numpy().view(np.uint32)[:k], to


@pytest.mark.parametrize("table", [False, True], ids=["walk", "table"])
def test_backtrace_lookup_matches_oracle(case, table, monkeypatch):
    name, mb, buf, off, oids, olens, oto = case
    if name == "_edge_case":
        starts = {int(off[i]) & 3 for i in range(len(off) - 1) if off[i + 1] > off[i]}
        assert starts == {0, 1, 2, 3}
        assert {1, 2, 3, 4, 15} <= set(olens.tolist())
    if table:
        monkeypatch.delenv("SPM_HIP_NO_PIECE_TABLE", raising=False)
    else:
        monkeypatch.setenv("SPM_HIP_NO_PIECE_TABLE", "1")
    live0 = S.device_bytes()[0]
    dm = S.DeviceModel(mb)
    grown = S.device_bytes()[0] - live0
    assert dm.info().fast_variant == 1
    ids, lens, to = _encode_device(dm, buf, off)
    assert np.array_equal(to, oto), "token counts differ"
    assert np.array_equal(ids, oids)
    assert np.array_equal(lens, olens)
    st = dm.stats()
    assert st.general_path < len(off) - 1  # the fast kernel wrote tokens itself
    dm.close()
    # The table is a device buffer of its own, counted by spm_hip_device_bytes;
    # the knob leaves it out.
    other = "1" if table else None
    if other:
        monkeypatch.setenv("SPM_HIP_NO_PIECE_TABLE", other)
    else:
        monkeypatch.delenv("SPM_HIP_NO_PIECE_TABLE", raising=False)
    live1 = S.device_bytes()[0]
    dm2 = S.DeviceModel(mb)
    grown2 = S.device_bytes()[0] - live1
    dm2.close()
    assert (grown > grown2) if table else (grown < grown2)
