"""GPU: text rows on the device (spm_hip_split_lines, spm_hip_format_id_rows,
spm_hip_format_piece_rows, text_rows.hip) equal plain Python exactly:
buf.split(b"\\n") with the getline rule, " ".join(map(str, row)) and a join of
piece bytes.  Every output buffer stands between sentinel bytes that must come
back untouched.

A pass runs S.TEXT_BLOCKS blocks; a block's range is a multiple of the tile
(T = S.TEXT_SPLIT_TILE bytes, S.TEXT_ID_TILE / S.TEXT_PIECE_TILE items), so an
input of k tiles runs on k blocks and one of more than S.TEXT_BLOCKS tiles
makes every block walk two tiles (the "big" cases)."""
import os

import numpy as np
import pytest

import model_builder as MB
import model_reader
import oracle_lib
import spm_amd as S

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
pytestmark = pytest.mark.gpu
T = S.TEXT_SPLIT_TILE
GUARD = 256
U = "▁".encode()


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


class Guarded:
    """`nbytes` bytes between two runs of GUARD sentinel bytes, the base moved by skew."""

    def __init__(self, nbytes, skew=0):
        import torch
        self.lo, self.n = GUARD + skew, nbytes
        self.t = torch.full((self.lo + nbytes + GUARD,), 0x5A, dtype=torch.uint8, device=_dev())
        self.ptr = self.t.data_ptr() + self.lo

    def get(self, dtype=np.uint8):
        h = self.t.cpu().numpy()
        assert (h[:self.lo] == 0x5A).all(), "sentinel before the buffer overwritten"
        assert (h[self.lo + self.n:] == 0x5A).all(), "sentinel after the buffer overwritten"
        return h[self.lo:self.lo + self.n].copy().view(dtype)


def _ctl():
    import torch
    return (torch.zeros(4, dtype=torch.int64, device=_dev()),
            torch.empty(S.TEXT_ROWS_SCRATCH_BYTES, dtype=torch.uint8, device=_dev()))


def getlines(buf):
    lines = buf.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    return lines


def run_split(buf, skew=0, short=0):
    """One device split against getlines; short: line capacity below the need."""
    import torch
    lines = getlines(buf)
    cap = len(lines) - short
    src = Guarded(len(buf), skew)
    src.t[src.lo:src.lo + len(buf)] = torch.from_numpy(np.frombuffer(buf + b"\0", dtype=np.uint8)[:len(buf)].copy())
    out, off = Guarded(len(buf), skew), Guarded(8 * (cap + 1), 8 * (skew & 1))
    ctl, scratch = _ctl()
    S.split_lines_device(src.ptr, len(buf), out.ptr, off.ptr, cap, ctl.data_ptr(), scratch.data_ptr(),
                         d_counts=ctl.data_ptr() + 8)
    status, n, nb = ctl.tolist()[:3]
    got, goff = out.get().tobytes(), off.get(np.uint64)
    assert (n, nb) == (len(lines), sum(map(len, lines)))
    assert status == (S.SPM_RESOURCE_EXHAUSTED if short else S.SPM_OK)
    assert got[:nb] == b"".join(lines) and got[nb:] == b"\x5a" * (len(buf) - nb)
    assert goff.tolist() == np.cumsum([0] + [len(x) for x in lines])[:cap + 1].tolist()


SPLIT = {
    "empty": b"", "nl": b"\n", "a": b"a", "a_nl": b"a\n", "nl_nl": b"\n\n", "crlf": b"a\r\n", "no_tail_nl": b"ab\ncd",
    "nul_ff": b"\x00\xff\n\xff\xfe\x00\n\x00",
    "tile_lines": b"a" * (T - 1) + b"\n" + b"b" * T + b"\n" + b"c" * (T + 1) + b"\n",
    "nl_tile_last": b"x" * (T - 1) + b"\ny\n", "nl_tile_first": b"x" * T + b"\ny",
    "nl_run": b"q" + b"\n" * (T + 37) + b"r", "long_line": b"ab\n" + b"L" * (3 * T + 5) + b"\ncd",
}


@pytest.mark.parametrize("name", sorted(SPLIT))
def test_split(name):
    run_split(SPLIT[name])


@pytest.mark.parametrize("skew", range(16))
def test_split_alignment(skew):
    run_split(b"k" * (T - 9) + b"\n\nmm\n" + b"z" * 40 + b"\n" * 3 + b"w" * T, skew=skew)


def test_split_capacity_short():
    run_split(SPLIT["tile_lines"] + b"tail", short=1)


def test_split_big():
    rng = np.random.default_rng(3)
    buf = rng.integers(0, 256, S.TEXT_BLOCKS * T + 3 * T + 11, dtype=np.uint8)
    buf[rng.random(buf.size) < 0.02] = 10
    run_split(buf.tobytes(), skew=5)


def run_id_rows(rows, base=0, short=0):
    import torch
    ids = np.array([9] * base + [x for r in rows for x in r], dtype=np.int32)
    off = np.cumsum([base] + [len(r) for r in rows]).astype(np.uint64)
    want = [" ".join(map(str, r)).encode() + b"\n" for r in rows]
    text = b"".join(want)
    cap = len(text) - short
    d_ids = torch.from_numpy(ids if ids.size else np.zeros(1, np.int32)).to(_dev())
    d_off = torch.from_numpy(off.view(np.int64)).to(_dev())
    out, roff = Guarded(cap, 3), Guarded(8 * (len(rows) + 1))
    ctl, scratch = _ctl()
    S.format_id_rows_device(d_ids.data_ptr(), d_off.data_ptr(), len(rows), out.ptr, cap, roff.ptr, ctl.data_ptr(),
                            scratch.data_ptr())
    assert ctl.tolist()[0] == (S.SPM_RESOURCE_EXHAUSTED if short else S.SPM_OK)
    assert out.get().tobytes() == text[:cap]
    assert roff.get(np.uint64).tolist() == np.cumsum([0] + [len(w) for w in want]).tolist()


EDGE_IDS = sorted({0, 2 ** 31 - 1} | {10 ** k for k in range(10)} | {10 ** k - 1 for k in range(1, 10)})
K = S.TEXT_ID_TILE
ID_ROWS = {
    "edges": [EDGE_IDS], "empties": [[], [5], [], [], [7, 8], []], "all_empty": [[]] * 5, "none": [],
    "long_row": [[1], list(range(2 * K + 50)), [2]],
    # items = tokens + one per row: row 0 ends on item K - 1, row 1 starts tile 1;
    # then a row whose last token is the tile's last item and its terminator opens the next.
    "tile_edges": [list(range(K - 1)), [11, 12], list(range(K - 3)), [99999]],
}


@pytest.mark.parametrize("name", sorted(ID_ROWS))
def test_id_rows(name):
    run_id_rows(ID_ROWS[name])


def test_id_rows_offset_base_and_capacity():
    run_id_rows(ID_ROWS["empties"] + ID_ROWS["edges"], base=3)
    run_id_rows(ID_ROWS["tile_edges"], base=1, short=1)


def test_id_rows_big():
    rng = np.random.default_rng(5)
    flat = (rng.integers(0, 2 ** 31, K * S.TEXT_BLOCKS, dtype=np.int64) >> rng.integers(0, 31, K * S.TEXT_BLOCKS))
    cuts = np.sort(rng.integers(0, flat.size + 1, flat.size // 4))
    run_id_rows([r.tolist() for r in np.split(flat, cuts)])


@pytest.mark.parametrize("form", ["image", "direct"])
def test_store_forms(monkeypatch, form):
    """The split and id rows in both store forms (through the LDS image, or every
    lane storing its own bytes): whichever is not the default still runs here."""
    monkeypatch.setenv("SPM_HIP_TEXT_ROWS_FORM", form)
    run_split(SPLIT["tile_lines"] + SPLIT["nl_run"], skew=7)
    run_id_rows(ID_ROWS["tile_edges"] + ID_ROWS["empties"] + ID_ROWS["edges"], base=2, short=1)


def botchan(k=300):
    return oracle_lib.read_lines_binary(os.path.join(GOLD, "botchan.txt"))[:k]


def golden_rows(name, k=300):
    rows = oracle_lib.read_lines_binary(os.path.join(GOLD, name))[:k]
    return b"".join(r + b"\n" for r in rows)  # spm_encode's own output (botchan's lines end in '\r')


def device_piece_rows(dm, lines, opts, short=0):
    """format_piece_rows_device over the records of spm_hip_encode_spt for `lines`."""
    import torch
    buf, off = S.to_csr(lines)
    d_in, d_off = torch.from_numpy(buf).to(_dev()), torch.from_numpy(off.view(np.int64)).to(_dev())
    d_norm, d_noff, d_p, d_po, tn, tp = dm._spt_records_device(d_in, d_off, len(lines), int(off[-1]), opts)
    ctl, scratch = _ctl()
    roff = Guarded(8 * (len(lines) + 1))
    probe = Guarded(0)  # the count first: capacity 0 writes no text and reports the need
    dm.format_piece_rows_device(d_p.data_ptr(), d_po.data_ptr(), len(lines), d_norm.data_ptr(), d_noff.data_ptr(),
                                probe.ptr, 0, roff.ptr, ctl.data_ptr(), scratch.data_ptr())
    need = int(roff.get(np.uint64)[-1])
    probe.get()
    assert ctl.tolist()[0] == (S.SPM_RESOURCE_EXHAUSTED if need else S.SPM_OK)
    ctl.zero_()
    out = Guarded(need - short, 1)
    dm.format_piece_rows_device(d_p.data_ptr(), d_po.data_ptr(), len(lines), d_norm.data_ptr(), d_noff.data_ptr(),
                                out.ptr, need - short, roff.ptr, ctl.data_ptr(), scratch.data_ptr())
    assert ctl.tolist()[0] == (S.SPM_RESOURCE_EXHAUSTED if short else S.SPM_OK)
    return out.get().tobytes(), roff.get(np.uint64)


def joined_records(dm, mb, lines, opts):
    strings = [p for p, _, _ in model_reader.read_pieces(mb)]
    rows = dm.encode_spt_device(lines, opts)
    return [b" ".join(strings[r[0]] if r[1] is None else r[1] for r in row) + b"\n" for row in rows]


@pytest.mark.parametrize("opts", ["", "bos:eos", "reverse"])
@pytest.mark.parametrize("model", ["test_model", "botchan_bf_bpe1k", "botchan_char60"])
def test_piece_rows(model, opts):
    mb = open(os.path.join(GOLD, model + ".model"), "rb").read()
    dm = S.DeviceModel(mb)
    lines = botchan()
    want = joined_records(dm, mb, lines, opts)
    text, roff = device_piece_rows(dm, lines, opts)
    assert text == b"".join(want)
    assert roff.tolist() == np.cumsum([0] + [len(w) for w in want]).tolist()
    if model == "test_model" and not opts:
        assert text == golden_rows("botchan_test_model.pieces")


@pytest.mark.parametrize("wave_over", ["0", "1", "16", "152", "153"])
def test_piece_rows_long_pieces(monkeypatch, wave_over):
    """A piece longer than a wave, an unknown run longer than a tile of items
    and than the block's 256 lanes, empty lines between, and a short capacity;
    in the layout over output bytes (0) and with pieces over wave_over bytes
    copied by the wave (the 153-byte piece on either side of the bound)."""
    monkeypatch.setenv("SPM_HIP_TEXT_ROWS_PIECE_WAVE", wave_over)
    long_piece = U + b"x" * 150
    pieces = MB.base_pieces() + [(long_piece, -1.0, MB.NORMAL), (U, -2.0, MB.NORMAL), ("x", -3.0, MB.NORMAL),
                                 ("a", -3.0, MB.NORMAL)]
    mb = MB.model(pieces)
    dm = S.DeviceModel(mb)
    lines = [b"x" * 150 + b" a", b"", b"a " + b"z" * 5000 + b" a", b"", b""] + [b"a x"] * 300
    want = b"".join(joined_records(dm, mb, lines, "bos:eos"))
    assert long_piece in want and b"z" * 5000 in want
    assert device_piece_rows(dm, lines, "bos:eos")[0] == want
    assert device_piece_rows(dm, lines, "bos:eos", short=1)[0] == want[:-1]


@pytest.mark.parametrize("fmt,golden", [("id", "botchan_test_model.ids"), ("piece", "botchan_test_model.pieces")])
def test_encode_text_rows(fmt, golden):
    dm = S.DeviceModel(open(os.path.join(GOLD, "test_model.model"), "rb").read())
    lines, want = botchan(), golden_rows(golden)
    text = b"\n".join(lines) + b"\n"
    assert dm.encode_text_rows(text, fmt) == want
    assert dm.encode_text_rows(text[:-1], fmt) == want
    cr = [x + b"\r" for x in lines[:40]]  # the '\r' stays in the line, as with std::getline
    if fmt == "id":
        rows = [" ".join(map(str, r)).encode() + b"\n" for r in dm.encode_lines_device(cr, "bos")]
    else:
        rows = joined_records(dm, open(os.path.join(GOLD, "test_model.model"), "rb").read(), cr, "bos")
    assert dm.encode_text_rows(b"\n".join(cr) + b"\n", fmt, "bos") == b"".join(rows)
    assert dm.encode_text_rows(b"", fmt) == b""


LIB = os.path.join(os.path.dirname(GOLD), os.pardir, "sentencepiece-comments_amd", "lib")


def run_tool(tool, args, env_extra=None):
    import subprocess
    env = {k: v for k, v in os.environ.items() if not k.startswith("SPM_HIP_TEXT_ROWS")}
    env.update(env_extra or {})
    return subprocess.run([os.path.join(LIB, tool)] + args, env=env, stdout=subprocess.PIPE, check=True).stdout


@pytest.mark.parametrize("lines", [300, 17, 16])
@pytest.mark.parametrize("chunk", [None, "2048"])  # about 30 lines a chunk: every chunk takes the device path
@pytest.mark.parametrize("fmt,golden", [("id", "botchan_test_model.ids"), ("piece", "botchan_test_model.pieces")])
def test_spm_encode_text_rows(tmp_path, fmt, golden, chunk, lines):
    """spm_encode writes the same bytes with the device text rows (SPM_HIP_TEXT_ROWS
    unset) as with the host path (=0): one chunk, a chunk size that cuts the
    file many times, and files on both sides of the 16-line small-call bound."""
    src = tmp_path / "in.txt"
    src.write_bytes(b"\n".join(botchan(lines)) + b"\n")
    args = ["--model=" + os.path.join(GOLD, "test_model.model"), "--output_format=" + fmt, str(src)]
    knob = {"SPM_HIP_TEXT_ROWS_CHUNK": chunk} if chunk else {}
    host = run_tool("spm_encode", args, dict(knob, SPM_HIP_TEXT_ROWS="0"))
    assert run_tool("spm_encode", args, knob) == host == golden_rows(golden, lines)


@pytest.mark.parametrize("fmt,golden", [("id", "botchan_test_model.ids"), ("piece", "botchan_test_model.pieces")])
def test_text_rows_selftest(tmp_path, fmt, golden):
    src = tmp_path / "in.txt"
    src.write_bytes(b"\n".join(botchan()))  # no final newline
    rows = run_tool("text_rows_selftest", [os.path.join(GOLD, "test_model.model"), fmt, "", str(src)])
    assert rows == golden_rows(golden)
