"""GPU: spm_hip_window_ids (dense_window.hip) equals the Python restatement
(window_ref.py) exactly on every output.  Every output stands between 64
sentinel words (test_gpu_dense.Guarded); the sentinels, and every row at or
past the rows needed or the capacity, must come back untouched."""
import os
import subprocess

import numpy as np
import pytest

import spm_amd as S
import window_ref as R
from test_gpu_dense import CANARY, GOLD, LIB, Guarded, _dev, botchan, model, upload

pytestmark = pytest.mark.gpu
SHAPES = [(1, 0, 0), (3, 0, 3), (4, 1, 0), (4, 3, 0), (5, 1, 3), (8, 0, 1), (17, 5, 2), (257, 64, 3)]
ROW_OUTPUTS = ("out", "pos", "fresh", "lengths", "row_sentence")
NULLABLE = ROW_OUTPUTS[1:] + ("first_row", "stats")


def run_window(ids, off, L, stride, flags, spare=2, absent=(), skew=0, stream=None, want=None):
    """One device call against the restatement; capacity = the rows needed + spare."""
    import torch
    n = len(off) - 1
    want = want or R.window_ref(ids, off, L, stride, -1, flags)
    need = want[6][0]
    cap = max(need + spare, 0)
    d_ids, d_off = upload(ids, off)
    bufs = {"out": Guarded(cap * L, torch.int32, skew), "pos": Guarded(cap * L, torch.int32, skew),
            "fresh": Guarded(cap * L, torch.uint8, skew), "lengths": Guarded(cap, torch.int32, skew),
            "row_sentence": Guarded(cap, torch.int32, skew), "first_row": Guarded(n + 1, torch.int64),
            "stats": Guarded(2, torch.int64)}
    nbytes = S.window_ids_scratch_bytes(n)
    scratch = Guarded((nbytes + 15) // 16 * 2, torch.int64)  # 64 sentinel words = 512 bytes: stays 16-byte aligned
    ptr = {k: None if k in absent else bufs[k].ptr for k in NULLABLE}
    S.window_ids_device(d_ids.data_ptr(), d_off.data_ptr(), n, L, stride, -1, flags, cap, bufs["out"].ptr, scratch.ptr,
                        nbytes, ptr["pos"], ptr["fresh"], ptr["lengths"], ptr["row_sentence"], ptr["first_row"],
                        ptr["stats"], stream=stream)
    torch.cuda.synchronize()
    scratch.get()
    rows = min(need, cap)
    for name, w in zip(ROW_OUTPUTS, want[:5]):
        got = bufs[name].get().reshape((cap,) + w.shape[1:])
        if name in absent:
            assert (got == bufs[name].fill).all(), name
            continue
        assert np.array_equal(got[:rows], w[:rows]), name
        assert (got[rows:] == bufs[name].fill).all(), name + ": a row past the rows needed or the capacity was written"
    for name, w in (("first_row", want[5].view(np.int64)), ("stats", np.array(want[6], dtype=np.int64))):
        got = bufs[name].get()
        assert (got == bufs[name].fill).all() if name in absent else np.array_equal(got, w), name
    return want


@pytest.mark.parametrize("batch", ["one", "many", "mixed"])
@pytest.mark.parametrize("L,stride,flags", SHAPES)
def test_shapes(L, stride, flags, batch):
    """one: every edge length of the rule alone, and a sentence of 5000 tokens or more whose rows span three
    fill chunks.  many: one-row sentences over two scan tiles; at L < 4 a fill chunk holds more of them than
    the LDS segment.  mixed: the long sentence first, in the middle and last, the edge lengths between."""
    rng = np.random.default_rng(6000 + L)
    edge = R.edge_lens(L, stride, flags)
    big = max(5000, 3 * S.WINDOW_CHUNK_SLOTS * (L - (flags & 1) - (flags >> 1 & 1) - stride) // L + 7)
    if batch == "many":
        n = 2 * S.WINDOW_SCAN_TILE + 5 + (S.WINDOW_CHUNK_SLOTS if L < 4 else 0)
        assert L >= 4 or S.WINDOW_CHUNK_SLOTS // L > S.WINDOW_SEG
        assert run_window(*R.random_csr(rng, rng.integers(0, L + 1, size=n)), L, stride, flags)[6] == (n, 0)
        return
    mixed = [[big] + edge + [big] + edge[::-1] + [big]]
    for lens in mixed if batch == "mixed" else [[n] for n in edge + [big]] + [[]]:
        run_window(*R.random_csr(rng, lens), L, stride, flags)


def test_contracts():
    import torch
    rng = np.random.default_rng(6300)
    L, stride, flags = 5, 1, 3
    lens = [int(x) for x in rng.integers(0, 40, size=900)] + [5000]
    ids, off = R.random_csr(rng, lens, base=12345)  # offsets start above 0; the ids 4 bytes past a 16-byte boundary
    want = R.window_ref(ids, off, L, stride, -1, flags)
    for spare in (-want[6][0], -1000, -1, 0, 3):  # stats and first_row are complete when short
        run_window(ids, off, L, stride, flags, spare=spare, want=want)
    for absent in [(k,) for k in NULLABLE] + [NULLABLE]:
        run_window(ids, off, L, stride, flags, absent=absent, want=want)
    run_window(ids, off, L, stride, flags, skew=1, want=want)  # bases 4 bytes (fresh: 1 byte) past the alignment
    side = torch.cuda.Stream(_dev())
    with torch.cuda.stream(side):
        run_window(ids, off, L, stride, flags, stream=side.cuda_stream, want=want)


@pytest.mark.parametrize("name,sample", [("test_model", None), ("botchan_bpe1k", None), ("test_model", (0.5, 7, 0))])
def test_lines_to_windowed_tensors(name, sample):
    dm, lines = model(name), botchan()
    if sample is None:
        ids, off = __import__("dense_ref").csr(dm.encode_lines_device(lines, "bos:eos"))
    else:  # the draw itself, as encode_lines_packed lays it out
        out, seq, _ = dm.encode_lines_packed(lines, 64, -1, "bos:eos", sample=sample)
        flat, seq = out.cpu().numpy().reshape(-1), seq.cpu().numpy().reshape(-1)
        ids = flat[seq >= 0]
        off = np.concatenate([[0], np.cumsum(np.bincount(seq[seq >= 0], minlength=len(lines)))]).astype(np.uint64)
    got = dm.encode_lines_windowed(lines, 16, -1, 4, keep_first=True, keep_last=True, extra_options="bos:eos",
                                   sample=sample)
    want = R.window_ref(ids, off, 16, 4, -1, 3)
    assert want[6][1] > 10 and (want[3] < 16).any()  # lines of several rows, rows that end in padding
    for g, w, dt in zip(got, want[:5], ("int32", "int32", "bool", "int32", "int32")):
        assert str(g.dtype) == "torch." + dt and g.is_cuda and np.array_equal(g.cpu().numpy(), w.astype(dt))


def test_processor_encode_dense_window():
    short = ["I saw a girl with a telescope.", "", "hello world", "The quick brown fox jumps over the lazy dog again.",
             " ", "x"]
    p = subprocess.run([os.path.join(LIB, "window_selftest"), os.path.join(GOLD, "test_model.model"), "bos:eos", "6",
                        "-1", "1", "1", "1"] + short, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr.decode(errors="replace")
    body = {}
    for ln in p.stdout.decode().splitlines():
        body.setdefault(ln.split()[0], []).append([int(x) if x.lstrip("-").isdigit() else x for x in ln.split()[1:]])
    ids, off = __import__("dense_ref").csr(model("test_model").encode_lines_device([s.encode() for s in short], "bos:eos"))
    out, pos, fresh, lengths, row_sentence, first_row, stats = R.window_ref(ids, off, 6, 1, -1, 3)
    assert body["window"] == [["rows", stats[0], "row_len", 6, "tokens", int(off[-1]), "multi", stats[1]]]
    assert stats[1] >= 2 and (lengths < 6).any()
    assert body["ids"] == out.tolist() and body["pos"] == pos.tolist() and body["fresh"] == fresh.tolist()
    assert body["lengths"] == [lengths.tolist()] and body["row_sentence"] == [row_sentence.tolist()]
    assert body["first_row"] == [first_row.tolist()]
