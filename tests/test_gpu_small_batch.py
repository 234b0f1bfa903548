"""Small host batches (spm_hip_encode_batch_host with n <= 256: the single
tile path, one upload and one synchronization; a flagged sentence takes a
second round trip through the general kernel and the fix-up chain) stay
bit-exact against the oracle, including empty sentences, an all-empty batch,
flagged sentences and the 256/257 boundary."""
import os

import numpy as np
import pytest

import oracle_lib as O
import spm_amd as S
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _sents(n, seed):
    buf, off = synth.normalized(n, seed=seed)
    b = buf.tobytes()
    return [b[int(off[i]):int(off[i + 1])] for i in range(n)]


@pytest.mark.parametrize("model", ["synth32k_unigram.model", "synth32k_bpe.model"])
def test_small_batches_exact(model):
    mb = open(os.path.join(ROOT, "data", model), "rb").read()
    dm = S.DeviceModel(mb)
    om = O.OracleModel(mb)
    pool = _sents(3000, 41)
    pool[5] = pool[5] + b"\xff" + pool[5][:4]          # flagged by the byte kernel
    pool[300] = b"\xe3\x81" + pool[300]                # broken UTF-8
    pool[7] = b""
    start = 0
    for n in (1, 2, 3, 17, 255, 256, 257, 1, 64):
        batch = pool[start:start + n]
        start += n
        buf, off = S.to_csr(batch)
        ids, lens, tok = dm.encode_csr_host(buf, off, with_lens=True)
        rids, rlens, rtok = om.encode_normalized_csr(buf, off, with_lens=True)
        assert np.array_equal(tok, rtok) and np.array_equal(ids, rids) and np.array_equal(lens, rlens), n
    # single flagged sentence alone, and an all-empty batch
    for batch in ([pool[5]], [b"", b""], [b"\xff"]):
        buf, off = S.to_csr(batch)
        ids, lens, tok = dm.encode_csr_host(buf, off, with_lens=True)
        rids, rlens, rtok = om.encode_normalized_csr(buf, off, with_lens=True)
        assert np.array_equal(tok, rtok) and np.array_equal(ids, rids) and np.array_equal(lens, rlens), batch
    dm.close()


def test_small_paths_interleaved_on_one_workspace():
    """The three small-call paths share one workspace's staged image, device
    buffers and publication sequence: cooperative one-sentence calls (through
    the resident server), lane-path batches of 17 / 40 / 256 sentences while
    the server is alive, raw-line calls, a sentence the cooperative kernel
    hands back to the lane path, and calls that grow the shared buffers from
    either path (a 3000-byte sentence; a 256-sentence lane image past the 64
    KiB pinned minimum), each followed at once by a cooperative and a raw
    call -- with and without lengths, every result equal to the oracle's.  The
    oracle runs first, so the device calls come back to back, inside the
    server's idle window.  A second pass checks the published stats."""
    gold = os.path.join(ROOT, "tests", "golden")
    mb = open(os.path.join(gold, "test_model.model"), "rb").read()
    dm = S.DeviceModel(mb)
    om = O.OracleModel(mb)
    lines = O.read_lines_binary(os.path.join(gold, "botchan.txt"))[:300]
    raw_pool = [x for x in lines if len(x) <= 1024]  # a longer line is not taken
    norm = om.normalize(lines)
    sp = "▁".encode()
    # One-word sentences: a 256-sentence lane image inside the pinned minimum;
    # whole lines: one past it (with lengths, 9 bytes of image per input byte).
    short = [sp + w for s in norm for w in s.split(sp) if w][:256]
    big = norm[:256]
    assert len(short) == 256 and sum(map(len, short)) <= 5000 and sum(map(len, big)) >= 8000
    long_one = sp + b"x" * 2997

    def normalized(batch, with_lens):
        return ("norm", batch, with_lens)

    def after_growth(i):
        return [normalized([norm[i % len(norm)]], True), ("raw", [raw_pool[i % len(raw_pool)]], None)]

    plan = []
    for i in range(85):
        r, k = i % 5, i // 5
        if r == 0:
            plan.append(normalized([norm[i]], k % 2 == 1))
        elif r == 1:
            n = (17, 40, 256)[k % 3]
            plan.append(normalized(short if n == 256 else [norm[(i + j) % len(norm)] for j in range(n)], k % 2 == 1))
        elif r == 2:
            plan.append(("raw", [raw_pool[(i + j) % len(raw_pool)] for j in range(1 + k % 4)], None))
        elif r == 3:
            plan.append(normalized([b"\xff"], k % 2 == 0))
        elif i == 29:
            plan += [normalized([long_one], True)] + after_growth(i)
        elif i == 59:
            plan += [normalized(big, True)] + after_growth(i)
        else:
            plan.append(normalized([norm[(i + j) % len(norm)] for j in range(2 + k % 15)], False))
    timed = [normalized([norm[3]], True), normalized([norm[(7 + j) % len(norm)] for j in range(17)], False),
             ("raw", raw_pool[:2], None), normalized([b"\xff"], True), normalized(short, True),
             normalized([norm[5]], False), normalized([b"\xff"], False), normalized(norm[10:50], True),
             ("raw", raw_pool[2:3], None), normalized([norm[9], norm[11]], True)]

    def oracle(call):
        kind, batch, with_lens = call
        if kind == "raw":
            return [list(map(int, w)) for w in om.encode_lines(batch)]
        buf, off = S.to_csr(batch)
        return (buf, off) + tuple(om.encode_normalized_csr(buf, off, with_lens=with_lens))

    want = [oracle(c) for c in plan]
    want_timed = [oracle(c) for c in timed]

    def run(call, ref, where):
        kind, batch, with_lens = call
        if kind == "raw":
            got = dm.encode_raw_small(batch)
            assert got is not None and [list(map(int, g)) for g in got] == ref, where
            return None
        got = dm.encode_csr_host(ref[0], ref[1], with_lens=with_lens)
        assert len(got) == len(ref) - 2 and all(np.array_equal(g, r) for g, r in zip(got, ref[2:])), where
        return got[0]

    for t, (call, ref) in enumerate(zip(plan, want)):
        run(call, ref, t)
    dm.set_timing(True)
    for t, (call, ref) in enumerate(zip(timed, want_timed)):
        ids = run(call, ref, ("timed", t))
        if ids is not None:
            st = dm.stats()
            assert st.sentences == len(call[1]) and st.tokens == len(ids), ("timed", t)
            if call[1] == [b"\xff"]:
                assert st.general_path >= 1, ("timed", t)
    dm.close()
