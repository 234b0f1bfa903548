"""GPU: spm_hip_decode_batch (decode_kernels.hip) equals the restatement of the
reference's Decode (tests/decode_ref.py): text bytes, sentence offsets and
piece begins, through the blocking entry, the pure stream entry and the host
-buffer entry; and its error paths leave a canary-filled output untouched."""
import numpy as np
import pytest

import decode_cases as C
import decode_ref
import spm_amd as S

pytestmark = pytest.mark.gpu
CANARY = 0xA5


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


class Buffers:
    """Device copies of an id batch and canary-filled outputs."""

    def __init__(self, ids, off, options="", capacity=0, with_begin=True):
        import torch
        dev = _dev()
        self.n = len(off) - 1
        self.extras = sum(1 for o in options.split(":") if o in ("bos", "eos"))
        self.tokens = int(off[-1]) - int(off[0]) + self.n * self.extras
        self.d_ids = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32) if ids.size else
                                      np.zeros(1, np.int32)).to(dev)
        self.d_tok = torch.from_numpy(off.view(np.int64)).to(dev)
        self.capacity = capacity
        self.d_out = torch.full((max(capacity, 1) + 64,), CANARY, dtype=torch.uint8, device=dev)
        self.d_off = torch.full((self.n + 1,), -7, dtype=torch.int64, device=dev)
        self.d_begin = torch.full((max(self.tokens, 1) + 16,), -7, dtype=torch.int32, device=dev) if with_begin else None
        self.stream = torch.cuda.current_stream(dev).cuda_stream

    def begin_ptr(self):
        return self.d_begin.data_ptr() if self.d_begin is not None else None

    def offsets(self):
        return self.d_off.cpu().numpy().view(np.uint64)

    def out(self):
        return self.d_out.cpu().numpy()

    def untouched(self):
        """No text byte, no begin and no offset was written."""
        ok = bool((self.out() == CANARY).all()) and bool((self.d_off.cpu().numpy() == -7).all())
        return ok and (self.d_begin is None or bool((self.d_begin.cpu().numpy() == -7).all()))


def _decode(dm, ids, off, options="", entry="blocking"):
    """(text bytes, out_off, begins) of one device call sized by a count-only call."""
    import torch
    count = Buffers(ids, off, options, with_begin=False)
    total = dm.decode_device(options, count.d_ids.data_ptr(), count.d_tok.data_ptr(), count.n, None, 0,
                             count.d_off.data_ptr(), stream=count.stream)
    assert (count.out() == CANARY).all()
    b = Buffers(ids, off, options, capacity=total)
    if entry == "blocking":
        got = dm.decode_device(options, b.d_ids.data_ptr(), b.d_tok.data_ptr(), b.n, b.d_out.data_ptr(), total,
                               b.d_off.data_ptr(), d_piece_begin=b.begin_ptr(), stream=b.stream)
        assert got == total
    else:
        d_st = torch.zeros(1, dtype=torch.int32, device=_dev())
        dm.decode_device_async(options, b.d_ids.data_ptr(), b.d_tok.data_ptr(), b.n, b.d_out.data_ptr(), total,
                               b.d_off.data_ptr(), d_st.data_ptr(), d_piece_begin=b.begin_ptr(), stream=b.stream)
        torch.cuda.synchronize(_dev())
        assert int(d_st.item()) == 0
    out_off = b.offsets()
    assert out_off.tolist() == count.offsets().tolist()  # the count-only call gives the same offsets
    out = b.out()
    assert (out[total:] == CANARY).all()
    begins = b.d_begin.cpu().numpy()
    assert (begins[b.tokens:] == -7).all()
    return out[:total].tobytes(), out_off.tolist(), begins[:b.tokens].view(np.uint32).tolist()


_REF = {}


def _reference(key, model_bytes, rows, options):
    """The restatement's answer, computed once per (batch, options)."""
    if (key, options) not in _REF:
        ids, off = C.to_csr(rows)
        _REF[(key, options)] = decode_ref.Model(model_bytes).decode_batch(ids, off, options)
    return _REF[(key, options)]


@pytest.mark.parametrize("entry", ["blocking", "async"])
@pytest.mark.parametrize("name,model", C.GOLDEN)
def test_golden_batches(name, model, entry):
    mbytes = C.golden_model(model)
    rows = C.golden_rows(name)
    ids, off = C.to_csr(rows)
    text, out_off, begins = _decode(S.DeviceModel(mbytes), ids, off, entry=entry)
    want_text, want_off, want_begins = _reference(name, mbytes, rows, "")
    assert want_text == b"".join(C.golden_texts(name))
    assert text == want_text and out_off == want_off and begins == want_begins


def test_more_than_one_tile_per_block():
    """Over DECODE_BLOCKS * DECODE_TILE_TOKENS tokens a block walks several
    tiles and carries its running offset from one to the next."""
    name, model = C.GOLDEN[1]
    mbytes = C.golden_model(model)
    rows = C.golden_rows(name)
    reps = S.DECODE_BLOCKS * S.DECODE_TILE_TOKENS // sum(len(r) for r in rows) + 1
    ids, off = C.to_csr(rows * reps)
    assert int(off[-1]) > S.DECODE_BLOCKS * S.DECODE_TILE_TOKENS
    text, out_off, begins = _decode(S.DeviceModel(mbytes), ids, off)
    want_text, want_off, want_begins = _reference(name, mbytes, rows, "")
    assert text == want_text * reps
    assert out_off == [k * want_off[-1] + o for k in range(reps) for o in want_off[:-1]] + [reps * want_off[-1]]
    assert begins == want_begins * reps


@pytest.mark.parametrize("options", ["", "reverse", "bos:eos", "reverse:bos:eos", "bos:reverse"])
@pytest.mark.parametrize("surface", [None, b"", b"<UNK>"])
def test_hand_cases(surface, options):
    assert (C.T, C.SUB) == (S.DECODE_TILE_TOKENS, S.DECODE_SUBTILE_TOKENS)
    mbytes = C.hand_model(surface)
    rows = C.hand_rows()
    ids, off = C.to_csr(rows)
    dm = S.DeviceModel(mbytes)
    want = _reference(("hand", surface), mbytes, rows, options)
    for entry in ("blocking", "async"):
        assert _decode(dm, ids, off, options, entry) == (want[0], want[1], want[2])
    text, out_off, begins = dm.decode_csr_host(ids, off, options, with_begin=True)  # upload, run, download
    assert (text.tobytes(), out_off.tolist(), begins.tolist()) == (want[0], want[1], want[2])


def test_id_csr_that_does_not_start_at_zero():
    mbytes = C.hand_model()
    rows = C.hand_rows()
    ids, off = C.to_csr(rows)
    pad = np.full(5, -1, dtype=np.int32)  # never read
    want = _reference(("hand", None), mbytes, rows, "bos:eos")
    got = _decode(S.DeviceModel(mbytes), np.concatenate([pad, ids]), off + np.uint64(5), "bos:eos")
    assert got == (want[0], want[1], want[2])


def test_empty_batch():
    import torch
    dm = S.DeviceModel(C.hand_model())
    b = Buffers(np.zeros(0, np.int32), np.zeros(1, np.uint64), capacity=8)
    assert dm.decode_device("", b.d_ids.data_ptr(), b.d_tok.data_ptr(), 0, b.d_out.data_ptr(), 8,
                            b.d_off.data_ptr(), stream=b.stream) == 0
    torch.cuda.synchronize(_dev())
    assert b.offsets().tolist() == [0] and (b.out() == CANARY).all()


@pytest.mark.parametrize("bad", [-1, len(C.BASE + C.EXTRA)])
@pytest.mark.parametrize("options", ["", "reverse:bos"])
def test_out_of_range_id(bad, options):
    import torch
    dm = S.DeviceModel(C.hand_model())
    rows = [[C.ABC], [C.DE] * 700 + [bad] + [C.F] * 700, [bad]]
    ids, off = C.to_csr(rows)
    b = Buffers(ids, off, options, capacity=1 << 16)
    with pytest.raises(S.SpmError) as e:
        dm.decode_device(options, b.d_ids.data_ptr(), b.d_tok.data_ptr(), b.n, b.d_out.data_ptr(), b.capacity,
                         b.d_off.data_ptr(), d_piece_begin=b.begin_ptr(), stream=b.stream)
    assert e.value.code == S.SPM_OUT_OF_RANGE
    assert "sentence 1" in str(e.value) and "id %d" % bad in str(e.value)
    assert b.untouched()
    d_st = torch.zeros(1, dtype=torch.int32, device=_dev())
    dm.decode_device_async(options, b.d_ids.data_ptr(), b.d_tok.data_ptr(), b.n, b.d_out.data_ptr(), b.capacity,
                           b.d_off.data_ptr(), d_st.data_ptr(), d_piece_begin=b.begin_ptr(), stream=b.stream)
    torch.cuda.synchronize(_dev())
    assert int(d_st.item()) == S.SPM_OUT_OF_RANGE and b.untouched()


def test_capacity():
    import torch
    mbytes = C.hand_model()
    rows = C.hand_rows()
    ids, off = C.to_csr(rows)
    dm = S.DeviceModel(mbytes)
    want_text, want_off, _ = _reference(("hand", None), mbytes, rows, "")
    total = len(want_text)
    b = Buffers(ids, off, capacity=total - 1)
    with pytest.raises(S.SpmError) as e:
        dm.decode_device("", b.d_ids.data_ptr(), b.d_tok.data_ptr(), b.n, b.d_out.data_ptr(), total - 1,
                         b.d_off.data_ptr(), d_piece_begin=b.begin_ptr(), stream=b.stream)
    assert e.value.code == S.SPM_RESOURCE_EXHAUSTED and e.value.total == total
    assert (b.out() == CANARY).all() and (b.d_begin.cpu().numpy() == -7).all()
    assert b.offsets().tolist() == want_off  # the sizes a second call needs
    d_st = torch.zeros(1, dtype=torch.int32, device=_dev())
    b = Buffers(ids, off, capacity=total - 1)
    dm.decode_device_async("", b.d_ids.data_ptr(), b.d_tok.data_ptr(), b.n, b.d_out.data_ptr(), total - 1,
                           b.d_off.data_ptr(), d_st.data_ptr(), d_piece_begin=b.begin_ptr(), stream=b.stream)
    torch.cuda.synchronize(_dev())
    assert int(d_st.item()) == S.SPM_RESOURCE_EXHAUSTED
    assert (b.out() == CANARY).all() and int(b.offsets()[-1]) == total
    # capacity == total succeeds (that is what _decode passes everywhere above)
    assert _decode(dm, ids, off)[0] == want_text


def test_async_call_after_an_error_writes_nothing():
    import torch
    dm = S.DeviceModel(C.hand_model())
    ids, off = C.to_csr(C.hand_rows())
    b = Buffers(ids, off, capacity=1 << 16)
    d_st = torch.full((1,), 3, dtype=torch.int32, device=_dev())  # an earlier call of the chain failed
    dm.decode_device_async("", b.d_ids.data_ptr(), b.d_tok.data_ptr(), b.n, b.d_out.data_ptr(), b.capacity,
                           b.d_off.data_ptr(), d_st.data_ptr(), d_piece_begin=b.begin_ptr(), stream=b.stream)
    torch.cuda.synchronize(_dev())
    assert int(d_st.item()) == 3 and b.untouched()


def test_decode_bound_sizes_the_output():
    mbytes = C.hand_model()
    dm = S.DeviceModel(mbytes)
    assert dm.decode_bound() == len(C.LONG)
    rows = C.hand_rows()
    ids, off = C.to_csr(rows)
    want_text, _, _ = _reference(("hand", None), mbytes, rows, "")
    assert len(want_text) <= int(off[-1]) * dm.decode_bound()


def test_encode_then_decode_round_trip():
    """Ids straight from spm_hip_encode_batch + spm_hip_finalize_ids decode to
    the package's text of the golden rows."""
    import oracle_lib as O
    import os
    name, model = C.GOLDEN[0]
    mbytes = C.golden_model(model)
    lines = O.read_lines_binary(os.path.join(C.GOLD, "botchan.txt"))[:500]
    dm = S.DeviceModel(mbytes)
    rows = dm.encode_lines_device(lines)
    assert rows == C.golden_rows(name)[:500]
    ids, off = C.to_csr(rows)
    text, out_off, _ = _decode(dm, ids, off)
    assert text == b"".join(C.golden_texts(name)[:500])
