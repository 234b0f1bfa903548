"""GPU: spm_hip_fit_ids (dense_fit.hip) equals the Python restatement
(fit_ref.py) exactly, on the smallest shapes at which its passes can go wrong.
Every output stands between 64 sentinel words (test_gpu_dense.Guarded); the
sentinels, and every row at or past the rows needed or the capacity, must
come back untouched.  T = S.FIT_TILE sentences are one level-0 tile."""
import os
import subprocess

import numpy as np
import pytest

import fit_ref as R
import spm_amd as S
from test_gpu_dense import CANARY, GOLD, LIB, Guarded, _dev, botchan, model, upload

pytestmark = pytest.mark.gpu
T = S.FIT_TILE
OUTPUTS = ("seq", "pos", "row_lengths", "place", "stats")


def run_fit(ids, off, L, flags=0, spare=2, absent=(), skew=0, stream=None, want=None):
    """One device call against the restatement; capacity = the rows needed + spare."""
    import torch
    n = len(off) - 1
    want = want or R.fit_ref(ids, off, L, -1, flags)
    need = want[5][0]
    cap = max(need + spare, 0)
    d_ids, d_off = upload(ids, off)
    bufs = {k: Guarded(cap * L, torch.int32, skew) for k in ("out", "seq", "pos")}
    bufs["row_lengths"] = Guarded(cap, torch.int32, skew)
    bufs["place"], bufs["stats"] = Guarded(n, torch.int64), Guarded(4, torch.int64)
    nbytes = S.fit_ids_scratch_bytes(n, L, cap)
    scratch = Guarded((nbytes + 15) // 16 * 2, torch.int64)  # 64 sentinel words = 512 bytes: stays 16-byte aligned
    ptr = {k: None if k in absent else bufs[k].ptr for k in OUTPUTS}
    S.fit_ids_device(d_ids.data_ptr(), d_off.data_ptr(), n, L, -1, flags, cap, bufs["out"].ptr, scratch.ptr, nbytes,
                     ptr["seq"], ptr["pos"], ptr["row_lengths"], ptr["place"], ptr["stats"], stream=stream)
    torch.cuda.synchronize()
    scratch.get()
    rows = min(need, cap)
    for name, w in zip(("out", "seq", "pos", "row_lengths"), want[:4]):
        got = bufs[name].get().reshape((cap, L) if name != "row_lengths" else (cap,))
        if name in absent:
            assert (got == CANARY).all(), name
            continue
        assert np.array_equal(got[:rows], w[:rows]), name
        assert (got[rows:] == CANARY).all(), name + ": a row past the rows needed or the capacity was written"
    for name, w in (("place", want[4].view(np.int64)), ("stats", np.array(want[5], dtype=np.int64))):
        got = bufs[name].get()
        assert (got == bufs[name].fill).all() if name in absent else np.array_equal(got, w), name
    return want


@pytest.mark.parametrize("L", [1, 2, 5, 64, 257])
def test_shapes(L):
    rng = np.random.default_rng(4000 + L)
    for n in (0, 1, 2, 1000):
        ids, off = R.random_csr(rng, R.mixed_lens(rng, n, L))
        for flags in (0, 2, 4, 6):
            run_fit(ids, off, L, flags)
    run_fit(*R.random_csr(rng, np.zeros(300, dtype=np.int64), base=4), L)  # every sentence empty


@pytest.mark.parametrize("n", [T - 1, T, T + 1, 3 * T + 7])
def test_tile_edges(n):
    """Lengths 1..3 at L = 4: a row start on every offset from a tile edge.
    Then every sentence a full row of its own: the most row starts a tile can hold."""
    rng = np.random.default_rng(n)
    run_fit(*R.random_csr(rng, rng.integers(1, 4, size=n)), 4)
    run_fit(*R.random_csr(rng, np.full(n, 4)), 4)


def test_rows_longer_than_tiles():
    """Lengths 0 / 1 at L = 3 T: tiles without a row start, exits that skip tiles."""
    rng = np.random.default_rng(12)
    want = run_fit(*R.random_csr(rng, rng.integers(0, 2, size=16 * T)), 3 * T)
    assert 2 <= want[5][0] <= 3


def test_every_level_of_the_composition(monkeypatch):
    """Two tiles per tile of the next level and at most two at the top: 5 tiles
    are 3 tiles of level 1 and 2 of level 2, which one thread walks."""
    monkeypatch.setenv("SPM_HIP_FIT_GEOMETRY", "2,2")
    rng = np.random.default_rng(13)
    n = 4 * T + 1
    ids, off = R.random_csr(rng, rng.integers(0, 9, size=n))
    plain = S.fit_ids_scratch_bytes(n, 64, 8)
    run_fit(ids, off, 64)
    monkeypatch.delenv("SPM_HIP_FIT_GEOMETRY")
    assert S.fit_ids_scratch_bytes(n, 64, 8) < plain  # the default geometry stops at level 0 here


def test_contracts():
    import torch
    rng = np.random.default_rng(14)
    ids, off = R.random_csr(rng, R.mixed_lens(rng, 900, 7), base=12345)  # offsets start above 0
    want = R.fit_ref(ids, off, 7, -1, 4)
    for spare in (-1, 0, 3):
        run_fit(ids, off, 7, 4, spare=spare, want=want)
    for absent in [(k,) for k in OUTPUTS] + [OUTPUTS]:
        run_fit(ids, off, 7, 4, absent=absent, want=want)
    run_fit(ids, off, 7, 4, skew=1, want=want)  # bases 4 bytes past a 16-byte boundary
    side = torch.cuda.Stream(_dev())
    with torch.cuda.stream(side):
        run_fit(ids, off, 7, 4, stream=side.cuda_stream, want=want)


@pytest.mark.parametrize("name,sample", [("test_model", None), ("botchan_bpe1k", None), ("test_model", (0.5, 7, 0))])
def test_lines_to_fitted_tensors(name, sample):
    dm, lines = model(name), botchan()
    if sample is None:
        rows = dm.encode_lines_device(lines, "bos:eos")
        ids, off = __import__("dense_ref").csr(rows)
    else:  # the draw itself, as encode_lines_packed lays it out
        out, seq, _ = dm.encode_lines_packed(lines, 64, -1, "bos:eos", sample=sample)
        flat, seq = out.cpu().numpy().reshape(-1), seq.cpu().numpy().reshape(-1)
        ids = flat[seq >= 0]
        off = np.concatenate([[0], np.cumsum(np.bincount(seq[seq >= 0], minlength=len(lines)))]).astype(np.uint64)
    got = dm.encode_lines_fitted(lines, 64, -1, "bos:eos", flags=S.SPM_DENSE_KEEP_END, sample=sample)
    want = R.fit_ref(ids, off, 64, -1, S.SPM_DENSE_KEEP_END)
    assert want[5][0] > 1 and (want[3] < 64).any()  # several rows, some end in padding
    for g, w in zip(got, want[:4]):
        assert str(g.dtype) == "torch.int32" and g.is_cuda and np.array_equal(g.cpu().numpy(), w)


@pytest.mark.parametrize("L,flags", [(40, 0), (6, 6)])
def test_processor_encode_dense_whole(L, flags):
    """One case whose rows end in padding, one whose long lines are cut."""
    short = ["I saw a girl with a telescope.", "", "hello world", "The quick brown fox jumps over the lazy dog again.",
             " ", "x"]
    p = subprocess.run([os.path.join(LIB, "fit_selftest"), os.path.join(GOLD, "test_model.model"), "bos:eos", str(L),
                        "-1", str(flags)] + short, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr.decode(errors="replace")
    body = {}
    for ln in p.stdout.decode().splitlines():
        body.setdefault(ln.split()[0], []).append([int(x) if x.lstrip("-").isdigit() else x for x in ln.split()[1:]])
    ids, off = __import__("dense_ref").csr(model("test_model").encode_lines_device([s.encode() for s in short], "bos:eos"))
    out, seq, pos, lengths, place, stats = R.fit_ref(ids, off, L, -1, flags)
    assert body["fit"] == [["rows", stats[0], "row_len", L, "tokens", int(off[-1]), "cut", stats[2], "dropped",
                            stats[3]]]
    assert (stats[2] > 0) == (L == 6) and (lengths < L).any()
    assert body["ids"] == out.tolist() and body["seq"] == seq.tolist() and body["pos"] == pos.tolist()
    assert body["row_lengths"] == [lengths.tolist()] and body["place"] == [place.view(np.int64).tolist()]
