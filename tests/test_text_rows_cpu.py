"""CPU: the _host loops of the text-row calls (text_rows.h) against plain Python:
buf.split(b"\\n") with the getline rule, " ".join(map(str, row)) and a join of
piece bytes."""
import os

import numpy as np
import pytest

import model_reader
import spm_amd as S

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def getlines(buf):
    lines = buf.split(b"\n")
    if lines[-1] == b"":
        lines.pop()  # a final '\n' ends the last line, it opens no new one
    return lines


SPLIT = [b"", b"\n", b"a", b"a\n", b"\n\n", b"a\r\n", b"ab\ncd", b"\x00\xff\n\xff\xfe\x00", b"x\n" * 70 + b"tail"]


@pytest.mark.parametrize("buf", SPLIT)
def test_split_lines_host(buf):
    rc, out, off, counts = S.split_lines_host(buf)
    lines = getlines(buf)
    assert rc == S.SPM_OK and counts.tolist() == [len(lines), sum(map(len, lines))]
    assert [out.tobytes()[int(off[i]):int(off[i + 1])] for i in range(len(lines))] == lines


def test_split_lines_host_capacity():
    rc, out, off, counts = S.split_lines_host(b"a\nbc\nd", line_capacity=2)
    assert rc == S.SPM_RESOURCE_EXHAUSTED and counts.tolist() == [3, 4]
    assert off.tolist() == [0, 1, 3] and out.tobytes() == b"abcd"


EDGE_IDS = sorted({0, 2 ** 31 - 1} | {10 ** k for k in range(10)} | {10 ** k - 1 for k in range(1, 10)})


@pytest.mark.parametrize("rows", [[EDGE_IDS], [[], [5], [], [], [7, 8], []], [[], []], []])
def test_format_id_rows_host(rows):
    ids = np.array([3, 3] + [x for r in rows for x in r], dtype=np.int32)  # off[0] = 2
    off = np.cumsum([2] + [len(r) for r in rows]).astype(np.uint64)
    want = [" ".join(map(str, r)).encode() + b"\n" for r in rows]
    rc, text, row_off = S.format_id_rows_host(ids, off)
    assert rc == S.SPM_OK and text == b"".join(want)
    assert row_off.tolist() == np.cumsum([0] + [len(w) for w in want]).tolist()
    if want:
        rc, text, row_off2 = S.format_id_rows_host(ids, off, capacity=len(b"".join(want)) - 1)
        assert rc == S.SPM_RESOURCE_EXHAUSTED and text == b"".join(want)[:-1] and (row_off2 == row_off).all()


def test_format_id_rows_host_negative():
    with pytest.raises(S.SpmError) as e:
        S.format_id_rows_host([1, -1], [0, 2])
    assert e.value.code == 11  # SPM_OUT_OF_RANGE


def test_format_piece_rows_host():
    mb = open(os.path.join(GOLD, "test_model.model"), "rb").read()
    strings = [p for p, _, _ in model_reader.read_pieces(mb)]
    dm = S.DeviceModel(mb, host_only=True)
    norm = [b"\xe2\x96\x81hello\xe2\x96\x81zz", b"", b"\xe2\x96\x81a"]
    # (id, begin, end, norm_begin, norm_end): spans, and empty spans that name a piece.
    rows = [[(1, 0, 0, 0, 0), (9, 0, 5, 0, 8), (0, 5, 8, 8, 13), (2, 8, 8, 0, 0)], [], [(7, 0, 1, 0, 4)]]
    want = b"".join(b" ".join(norm[i][p[3]:p[4]] if p[4] > p[3] else strings[p[0]] for p in r) + b"\n"
                    for i, r in enumerate(rows))
    flat = np.array([p for r in rows for p in r], dtype=np.int32)
    poff = np.cumsum([0] + [len(r) for r in rows])
    noff = np.cumsum([0] + [len(x) for x in norm])
    rc, text, row_off = dm.format_piece_rows_host(flat, poff, b"".join(norm), noff, len(want))
    assert rc == S.SPM_OK and text == want and int(row_off[-1]) == len(want)
    rc, text, _ = dm.format_piece_rows_host(flat, poff, b"".join(norm), noff, len(want) - 3)
    assert rc == S.SPM_RESOURCE_EXHAUSTED and text == want[:-3]
    flat[0, 0] = len(strings)  # an empty span whose id is outside the table
    with pytest.raises(S.SpmError):
        dm.format_piece_rows_host(flat, poff, b"".join(norm), noff, len(want))
