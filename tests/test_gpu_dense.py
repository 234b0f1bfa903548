"""GPU: dense id batches (spm_hip_pad_ids / spm_hip_pack_ids, dense_kernels.hip)
equal the numpy restatement (dense_ref.py) exactly, on the smallest shapes at
which the kernels can go wrong.  Every output buffer stands between 64
sentinel words; the sentinels, and for pack every row past stats[0], must come
back untouched.

A thread owns 4 consecutive output slots and a launch has at most
S.DENSE_BLOCKS blocks of S.DENSE_TILE_SLOTS slots per step, so a pad output of
more than 2^20 slots makes the blocks take a second step (n = 32000 at L = 33,
beside the n = 5000 case), and a pack stream of more than
S.DENSE_PACK_BLOCKS tiles gives every block a range of two tiles."""
import os
import subprocess

import numpy as np
import pytest

import dense_ref as R
import spm_amd as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
LIB = os.path.join(ROOT, "sentencepiece-comments_amd", "lib")
pytestmark = pytest.mark.gpu
CANARY = 0x5A5A5A5A
GUARD_WORDS = 64
PASS_SLOTS = S.DENSE_BLOCKS * S.DENSE_TILE_SLOTS


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


class Guarded:
    """`count` elements between two runs of 64 sentinel words; skew: elements
    the base is moved by, to leave the allocation's alignment."""

    def __init__(self, count, dtype, skew=0):
        import torch
        self.size = torch.empty(0, dtype=dtype).element_size()
        self.fill = {4: CANARY, 1: 0x5A, 8: 0x5A5A5A5A5A5A5A5A}[self.size]
        guard = GUARD_WORDS * 4 if self.size == 1 else GUARD_WORDS  # elements
        self.lo, self.count = guard + skew, count
        self.t = torch.full((self.lo + count + guard,), self.fill, dtype=dtype, device=_dev())
        self.ptr = self.t.data_ptr() + self.lo * self.size

    def get(self):
        """The payload, after checking both sentinel runs."""
        h = self.t.cpu().numpy()
        assert (h[:self.lo] == self.fill).all(), "sentinel before the buffer overwritten"
        assert (h[self.lo + self.count:] == self.fill).all(), "sentinel after the buffer overwritten"
        return h[self.lo:self.lo + self.count]


def upload(ids, off):
    import torch
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    d_ids = torch.from_numpy(ids if ids.size else np.zeros(1, np.int32)).to(_dev())
    d_off = torch.from_numpy(np.ascontiguousarray(off, dtype=np.uint64).view(np.int64)).to(_dev())
    return d_ids, d_off


def run_pad(ids, off, L, pad_id, flags, absent=(), skew=0, stream=None):
    """One device call against the restatement; absent: nullable outputs passed as NULL."""
    import torch
    n = len(off) - 1
    d_ids, d_off = upload(ids, off)
    out = Guarded(n * L, torch.int32, skew)
    lengths = Guarded(n, torch.int32, skew)
    mask = Guarded(n * L, torch.uint8, skew)
    stats = Guarded(2, torch.int64)
    S.pad_ids_device(d_ids.data_ptr(), d_off.data_ptr(), n, L, pad_id, flags, out.ptr,
                     None if "lengths" in absent else lengths.ptr, None if "mask" in absent else mask.ptr,
                     None if "stats" in absent else stats.ptr, stream=stream)
    torch.cuda.synchronize()
    w_out, w_len, w_mask, w_stats = R.pad_ref(ids, off, L, pad_id, flags)
    assert np.array_equal(out.get().reshape(n, L), w_out)
    for name, buf, want in (("lengths", lengths, w_len), ("mask", mask, w_mask.reshape(-1)),
                            ("stats", stats, np.array(w_stats, dtype=np.int64))):
        got = buf.get()
        if name in absent:
            assert (got == buf.fill).all()
        else:
            assert np.array_equal(got, want), name


def random_csr(rng, lens, base=0):
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens, dtype=np.uint64)
    ids = rng.integers(0, 32000, size=base + int(off[-1]), dtype=np.int32)
    return ids, off + np.uint64(base)


def pad_lens(rng, n, L):
    """Lengths from {0, 1, L-1, L, L+1, 2L+3}, every second one random in [0, 3L]."""
    special = np.array([0, 1, L - 1, L, L + 1, 2 * L + 3])
    lens = special[rng.integers(0, len(special), size=n)]
    rnd = rng.integers(0, 3 * L + 1, size=n)
    return np.where(np.arange(n) % 2 == 1, rnd, lens)


@pytest.mark.parametrize("L", [1, 2, 3, 4, 5, 7, 8, 64, 65, 257])
def test_pad_shapes(L):
    rng = np.random.default_rng(1000 + L)
    for n in (0, 1, 2, 1000):
        ids, off = random_csr(rng, pad_lens(rng, n, L))
        for flags in range(8):
            run_pad(ids, off, L, -1, flags)


@pytest.mark.parametrize("n", [5000, 32000])
def test_pad_many_rows(n):
    """L = 33: rows straddle blocks and waves at odd alignment; n = 32000 is
    more slots than one step of the whole grid."""
    rng = np.random.default_rng(n)
    ids, off = random_csr(rng, pad_lens(rng, n, 33))
    assert (n * 33 > PASS_SLOTS) == (n == 32000)
    for flags in ((0, 7) if n == 32000 else range(8)):
        run_pad(ids, off, 33, -100, flags)


def test_pad_all_sentences_empty():
    off = np.full(301, 4, dtype=np.uint64)
    for flags in range(8):
        run_pad(np.arange(4, dtype=np.int32), off, 6, 9, flags)


@pytest.mark.parametrize("L", [4, 8, 33])
def test_pad_base_not_16_byte_aligned(L):
    """Bases 4 bytes (ids, lengths) and 1 byte (mask) past a 16-byte boundary: the scalar stores."""
    rng = np.random.default_rng(77)
    ids, off = random_csr(rng, pad_lens(rng, 700, L))
    for flags in (0, 3, 7):
        run_pad(ids, off, L, -1, flags, skew=1)
    # The same through a torch slice.
    import torch
    n = 700
    d_ids, d_off = upload(ids, off)
    whole = torch.full((n * L + 1,), CANARY, dtype=torch.int32, device=_dev())
    view = whole[1:]
    assert view.data_ptr() % 16 == 4
    S.pad_ids_device(d_ids.data_ptr(), d_off.data_ptr(), n, L, -1, 4, view.data_ptr())
    torch.cuda.synchronize()
    assert int(whole[0]) == CANARY
    assert np.array_equal(view.cpu().numpy().reshape(n, L), R.pad_ref(ids, off, L, -1, 4)[0])


def test_pad_csr_slice_offsets_start_at_12345():
    rng = np.random.default_rng(5)
    ids, off = random_csr(rng, pad_lens(rng, 500, 7), base=12345)
    assert int(off[0]) == 12345
    for flags in range(8):
        run_pad(ids, off, 7, -1, flags)


def test_pad_nullable_outputs():
    rng = np.random.default_rng(6)
    ids, off = random_csr(rng, pad_lens(rng, 300, 5))
    for absent in (("lengths",), ("mask",), ("stats",), ("lengths", "mask", "stats")):
        run_pad(ids, off, 5, -1, 5, absent=absent)


_MODELS = {}


def model(name):
    if name not in _MODELS:
        _MODELS[name] = S.DeviceModel(open(os.path.join(GOLD, name + ".model"), "rb").read())
    return _MODELS[name]


def botchan(count=300):
    return open(os.path.join(GOLD, "botchan.txt"), "rb").read().split(b"\n")[:count]


def test_pad_twice_after_finalize_async_on_a_side_stream():
    """The epilogue's stream call, then the pad call twice, on a stream that is
    not the default one, with no synchronization in between."""
    import torch
    dev = _dev()
    dm = model("test_model")
    norm = dm.normalize(botchan())
    buf, off = S.to_csr(norm)
    n, cap, L = len(norm), int(off[-1]) + 2 * len(norm), 16
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        s = side.cuda_stream
        d_b = torch.from_numpy(buf).to(dev)
        d_o = torch.from_numpy(off.view(np.int64)).to(dev)
        d_ids = torch.empty(cap, dtype=torch.int32, device=dev)
        d_tok = torch.empty(n + 1, dtype=torch.int64, device=dev)
        d_fin = torch.empty(cap, dtype=torch.int32, device=dev)
        d_foff = torch.empty(n + 1, dtype=torch.int64, device=dev)
        d_st = torch.zeros(1, dtype=torch.int32, device=dev)
        outs = [(Guarded(n * L, torch.int32), Guarded(n, torch.int32), Guarded(n * L, torch.uint8),
                 Guarded(2, torch.int64)) for _ in range(2)]
        dm.encode_device_async(d_b.data_ptr(), d_o.data_ptr(), n, cap, d_ids.data_ptr(), d_tok.data_ptr(),
                               d_st.data_ptr(), stream=s)
        dm.finalize_ids_device_async("bos:eos", d_ids.data_ptr(), d_tok.data_ptr(), n, d_fin.data_ptr(), cap,
                                     d_foff.data_ptr(), d_st.data_ptr(), stream=s)
        for o, ln, m, st in outs:
            S.pad_ids_device(d_fin.data_ptr(), d_foff.data_ptr(), n, L, -1, 4, o.ptr, ln.ptr, m.ptr, st.ptr, stream=s)
    side.synchronize()
    assert int(d_st.item()) == 0
    foff = d_foff.cpu().numpy().view(np.uint64)
    fin = d_fin.cpu().numpy()[:int(foff[-1])]
    w_out, w_len, w_mask, w_stats = R.pad_ref(fin, foff, L, -1, 4)
    assert w_stats[0] > 0  # some botchan lines are longer than 16 ids
    for o, ln, m, st in outs:
        assert np.array_equal(o.get().reshape(n, L), w_out) and np.array_equal(ln.get(), w_len)
        assert np.array_equal(m.get(), w_mask.reshape(-1)) and tuple(st.get().tolist()) == w_stats


# ---- pack ----

def run_pack(ids, off, L, pad_id, spare_rows=2, absent=()):
    """Capacity = the rows needed + spare_rows (negative: too few)."""
    import torch
    n = len(off) - 1
    w_out, w_seq, w_pos, w_stats = R.pack_ref(ids, off, L, pad_id)
    need = w_stats[0]
    cap = max(need + spare_rows, 0)
    d_ids, d_off = upload(ids, off)
    bufs = {k: Guarded(cap * L, torch.int32) for k in ("out", "seq", "pos")}
    stats = Guarded(2, torch.int64)
    S.pack_ids_device(d_ids.data_ptr(), d_off.data_ptr(), n, L, pad_id, cap, bufs["out"].ptr,
                      None if "seq" in absent else bufs["seq"].ptr, None if "pos" in absent else bufs["pos"].ptr,
                      None if "stats" in absent else stats.ptr)
    torch.cuda.synchronize()
    rows = min(need, cap)
    for name, want in (("out", w_out), ("seq", w_seq), ("pos", w_pos)):
        got = bufs[name].get().reshape(cap, L)
        if name in absent:
            assert (got == CANARY).all()
            continue
        assert np.array_equal(got[:rows], want[:rows]), name
        assert (got[rows:] == CANARY).all(), name + ": a row past the rows needed was written"
    got = stats.get()
    assert (got == stats.fill).all() if "stats" in absent else tuple(got.tolist()) == w_stats


def split_lens(rng, T, parts):
    """`parts` sentence lengths that sum to T, empty ones among them."""
    cuts = np.sort(rng.integers(0, T + 1, size=parts - 1)) if parts > 1 else np.zeros(0, np.int64)
    return np.diff(np.concatenate([[0], cuts, [T]]))


@pytest.mark.parametrize("L", [1, 4, 5, 64, 100])
def test_pack_token_counts(L):
    rng = np.random.default_rng(2000 + L)
    for T in (0, 1, L - 1, L, L + 1, 3 * L):
        for parts in (1, 2, 7):
            ids, off = random_csr(rng, split_lens(rng, T, parts))
            run_pack(ids, off, L, -1)
    run_pack(*random_csr(rng, split_lens(rng, 3 * L, 5)), L, -1, absent=("seq",))
    run_pack(*random_csr(rng, split_lens(rng, 3 * L, 5)), L, -1, absent=("pos",))
    run_pack(*random_csr(rng, split_lens(rng, 3 * L, 5)), L, -1, absent=("seq", "pos", "stats"))


def test_pack_sentence_spans_three_rows_and_empty_runs():
    rng = np.random.default_rng(8)
    run_pack(*random_csr(rng, [2, 13, 1]), 5, -1)  # slots 2..14: rows 0, 1 and 2
    run_pack(*random_csr(rng, [0, 0, 0, 3, 0, 0, 0, 0, 6, 1, 0, 0, 0]), 4, -1)
    run_pack(*random_csr(rng, [0] * 70 + [5] + [0] * 300 + [9, 2] + [0] * 65), 4, -1)
    run_pack(*random_csr(rng, [0] * 40), 4, -1)


def test_pack_random_sentences():
    rng = np.random.default_rng(9)
    ids, off = random_csr(rng, rng.integers(0, 41, size=3000))
    run_pack(ids, off, 128, -100)
    run_pack(ids, off, 128, -100, spare_rows=-3)  # too few rows: the need is reported, nothing beyond is written
    run_pack(ids, off, 128, -100, spare_rows=40)


def test_pack_offsets_base_and_short_capacity():
    rng = np.random.default_rng(10)
    ids, off = random_csr(rng, rng.integers(0, 12, size=900), base=12345)
    for spare in (0, 2, -1, -5):
        run_pack(ids, off, 7, -1, spare_rows=spare)


def test_pack_two_tiles_per_block():
    rng = np.random.default_rng(11)
    ids, off = random_csr(rng, rng.integers(0, 61, size=80000))
    assert int(off[-1]) > S.DENSE_PACK_BLOCKS * S.DENSE_TILE_SLOTS
    run_pack(ids, off, 2048, -1, spare_rows=1)


# ---- end to end ----

E2E_MODELS = ["test_model", "botchan_bpe1k", "botchan_bf_unigram1k", "botchan_char60"]


def check_tensors(dm, lines, rows, options, sample=None):
    """encode_lines_padded / _packed against the restatement of the id lists `rows`."""
    ids, off = R.csr(rows)
    for L, flags in ((16, S.SPM_DENSE_KEEP_END), (256, 0)):
        out, lengths, mask = dm.encode_lines_padded(lines, L, -1, options, flags=flags, sample=sample)
        w_out, w_len, w_mask, _ = R.pad_ref(ids, off, L, -1, flags)
        assert out.dtype == lengths.dtype and str(out.dtype) == "torch.int32" and str(mask.dtype) == "torch.bool"
        assert out.is_cuda and tuple(out.shape) == (len(lines), L)
        assert np.array_equal(out.cpu().numpy(), w_out) and np.array_equal(lengths.cpu().numpy(), w_len)
        assert np.array_equal(mask.cpu().numpy(), w_mask.astype(bool))
        out, seq, pos = dm.encode_lines_packed(lines, L, -1, options, sample=sample)
        w_out, w_seq, w_pos, w_stats = R.pack_ref(ids, off, L, -1)
        assert tuple(out.shape) == (w_stats[0], L) == tuple(seq.shape) == tuple(pos.shape)
        assert np.array_equal(out.cpu().numpy(), w_out) and np.array_equal(seq.cpu().numpy(), w_seq)
        assert np.array_equal(pos.cpu().numpy(), w_pos)


@pytest.mark.parametrize("options", ["bos:eos", "reverse:eos"])
@pytest.mark.parametrize("name", E2E_MODELS)
def test_lines_to_tensors(name, options):
    dm, lines = model(name), botchan()
    check_tensors(dm, lines, dm.encode_lines_device(lines, options), options)


def test_lines_to_tensors_of_empty_lines():
    dm = model("test_model")
    out, lengths, mask = dm.encode_lines_padded([b"", b" "], 8, -1)
    assert (out.cpu().numpy() == -1).all() and lengths.tolist() == [0, 0] and not mask.any()
    out, seq, pos = dm.encode_lines_packed([b"", b" "], 8, -1)
    assert tuple(out.shape) == (0, 8) == tuple(seq.shape) == tuple(pos.shape)


@pytest.mark.parametrize("name", E2E_MODELS[:3])
def test_sampled_lines_to_tensors(name):
    """sample=(0.5, 7, 0): the host-CSR sampler (BPE: BPE-dropout) call, then the id epilogue."""
    import torch
    dev = _dev()
    dm, lines = model(name), botchan()
    buf, off = S.to_csr(dm.normalize(lines))
    n = len(lines)
    host = dm.bpe_dropout_encode_csr_host if dm.info().model_type == S.SPM_BPE else dm.sample_encode_csr_host
    ids, lens, tok = host(buf, off, 0.5, 7, 0, with_lens=True)
    d = [torch.from_numpy(a).to(dev) for a in (ids if ids.size else np.zeros(1, np.int32), lens.view(np.int32)
                                               if lens.size else np.zeros(1, np.int32), tok.view(np.int64), buf,
                                               off.view(np.int64))]
    cap = int(off[-1]) + 2 * n + 1
    d_out = torch.empty(cap, dtype=torch.int32, device=dev)
    d_oo = torch.empty(n + 1, dtype=torch.int64, device=dev)
    options = "bos:eos"
    if dm.byte_fallback() is None:
        k = dm.finalize_ids_device(options, d[0].data_ptr(), d[2].data_ptr(), n, d_out.data_ptr(), cap,
                                   d_oo.data_ptr())
    else:
        k = dm.finalize_ids_bytes_device(options, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), n,
                                         d[3].data_ptr(), d[4].data_ptr(), d_out.data_ptr(), cap, d_oo.data_ptr())
    torch.cuda.synchronize()
    fin, oo = d_out[:k].cpu().numpy(), d_oo.cpu().numpy()
    rows = [fin[int(oo[i]):int(oo[i + 1])].tolist() for i in range(n)]
    assert rows != dm.encode_lines_device(lines, options)  # a draw, not the best path
    check_tensors(dm, lines, rows, options, sample=(0.5, 7, 0))


# ---- processor ----

SELFTEST = os.path.join(LIB, "dense_selftest")
SHORT = ["I saw a girl with a telescope.", "", "hello world", "The quick brown fox jumps over the lazy dog again.",
         " ", "x"]


def selftest(name, options, L, pad_id, flags, mode, lines):
    p = subprocess.run([SELFTEST, os.path.join(GOLD, name + ".model"), options, str(L), str(pad_id), str(flags), mode]
                       + lines, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr.decode(errors="replace")
    return [ln.split() for ln in p.stdout.decode().splitlines()]


def parse_dense(rows, at):
    """One "dense ..." block starting at rows[at] -> (header dict, {name: rows of ints}, next index)."""
    head = rows[at]
    assert head[0] == "dense"
    hd = {head[k]: int(head[k + 1]) for k in range(1, len(head), 2)}
    body, at = {}, at + 1
    while at < len(rows) and rows[at][0] in ("ids", "lengths", "mask", "seq", "pos"):
        body.setdefault(rows[at][0], []).append([int(x) for x in rows[at][1:]])
        at += 1
    return hd, body, at


@pytest.mark.parametrize("name", ["test_model", "botchan_bpe1k"])
def test_processor_encode_dense(name):
    dm = model(name)
    lines = [s.encode() for s in SHORT]
    ids, off = R.csr(dm.encode_lines_device(lines, "bos:eos"))
    for L, flags in ((6, 5), (40, 0)):
        hd, body, _ = parse_dense(selftest(name, "bos:eos", L, -1, flags, "pad", SHORT), 0)
        w_out, w_len, w_mask, w_stats = R.pad_ref(ids, off, L, -1, flags)
        assert (hd["rows"], hd["row_len"], hd["tokens"], hd["cut"], hd["dropped"]) == \
            (len(lines), L, int(off[-1]), w_stats[0], w_stats[1])
        assert body["ids"] == w_out.tolist() and body["lengths"] == [w_len.tolist()] and body["mask"] == w_mask.tolist()
    hd, body, _ = parse_dense(selftest(name, "bos:eos", 8, -100, 0, "pack", SHORT), 0)
    w_out, w_seq, w_pos, w_stats = R.pack_ref(ids, off, 8, -100)
    assert (hd["rows"], hd["tokens"]) == w_stats
    assert body["ids"] == w_out.tolist() and body["seq"] == w_seq.tolist() and body["pos"] == w_pos.tolist()


@pytest.mark.parametrize("name", ["test_model", "botchan_bpe1k"])
def test_processor_sample_encode_dense_replays_sample_encode_batch(name):
    rows = selftest(name, "eos", 12, -1, 4, "sample", SHORT)
    batches, at = [], 0
    while rows[at][0] == "batch":
        batches.append([[int(x) for x in r[1:]] for r in rows[at + 1:at + 1 + len(SHORT)]])
        assert all(r[0] == "ids" for r in rows[at + 1:at + 1 + len(SHORT)])
        at += 1 + len(SHORT)
    assert len(batches) == 2 and batches[0] != batches[1]  # the second call draws anew
    for want in batches:
        hd, body, at = parse_dense(rows, at)
        ids, off = R.csr(want)
        w_out, w_len, w_mask, w_stats = R.pad_ref(ids, off, 12, -1, 4)
        assert body["ids"] == w_out.tolist() and body["lengths"] == [w_len.tolist()] and body["mask"] == w_mask.tolist()
        assert (hd["tokens"], hd["cut"], hd["dropped"]) == (int(off[-1]), w_stats[0], w_stats[1])
    assert at == len(rows)


def test_processor_host_only_is_failed_precondition():
    assert selftest("test_model", "", 8, -1, 0, "hostonly", SHORT) == [["code", "9", "9"]]
