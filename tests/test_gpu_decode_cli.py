"""GPU: the spm_decode drop-in CLI (SentencePieceProcessor::DecodeBatch over
spm_hip_decode_batch) undoes spm_encode on the golden fixtures, on the device
path and on the host loop, and keeps the reference's flags and messages."""
import os
import subprocess

import pytest

import decode_cases as C
import decode_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sentencepiece-comments_amd", "lib")
ENCODE, DECODE = os.path.join(LIB, "spm_encode"), os.path.join(LIB, "spm_decode")
MODEL = os.path.join(C.GOLD, "test_model.model")
LINES = 200
pytestmark = pytest.mark.gpu


def _decode(args, data, path):
    env = dict(os.environ, SPM_HIP_DECODE_PATH=path)
    return subprocess.run([DECODE, "--model=" + MODEL] + args, input=data, capture_output=True, timeout=120, env=env)


@pytest.fixture(scope="module")
def head(tmp_path_factory):
    """The first LINES botchan lines, and spm_encode's ids and pieces of them."""
    d = tmp_path_factory.mktemp("decode_cli")
    lines = open(os.path.join(C.GOLD, "botchan.txt"), "rb").read().split(b"\n")[:LINES]
    src = d / "head.txt"
    src.write_bytes(b"".join(l + b"\n" for l in lines))
    enc = {}
    for fmt in ("id", "piece"):
        enc[fmt] = subprocess.run([ENCODE, "--model=" + MODEL, "--output_format=" + fmt, str(src)],
                                  capture_output=True, timeout=120, check=True).stdout
    want = b"".join(t + b"\n" for t in C.golden_texts("botchan_test_model")[:LINES])
    return d, enc, want


@pytest.mark.parametrize("path", ["device", "host"])
@pytest.mark.parametrize("fmt", ["id", "piece"])
def test_encode_piped_to_decode(head, fmt, path):
    _, enc, want = head
    p = _decode(["--input_format=" + fmt], enc[fmt], path)
    assert p.returncode == 0, p.stderr
    if fmt == "id":
        assert p.stdout == want
        return
    # Decode(pieces) hands a piece outside the vocabulary through verbatim
    # (sentencepiece_processor.cc:683-687), where Decode(ids) writes
    # unk_surface: botchan's first line starts with a byte-order mark.  So the
    # lines without an unknown id reproduce the golden text, and every line
    # equals the reference's rules applied to the pieces.
    ref = decode_ref.Model(open(MODEL, "rb").read())
    got = p.stdout.split(b"\n")[:-1]
    rows = [[int(x) for x in l.split()] for l in enc["id"].split(b"\n")[:-1]]
    pieces = [[f for f in l.split(b" ") if f] for l in enc["piece"].split(b"\n")[:-1]]
    golden = want.split(b"\n")[:-1]
    assert len(got) == len(rows) == len(pieces) == len(golden) == LINES
    known = [i for i in range(LINES) if ref.unk_id not in rows[i]]
    assert len(known) >= LINES - 10
    assert [got[i] for i in known] == [golden[i] for i in known]
    assert got == [ref.decode_pieces(r)[0] for r in pieces]


@pytest.mark.parametrize("path", ["device", "host"])
@pytest.mark.parametrize("options", ["bos:eos", "reverse"])
def test_extra_options_and_proto(head, options, path):
    _, enc, _ = head
    ref = decode_ref.Model(open(MODEL, "rb").read())
    rows = [[int(x) for x in l.split()] for l in enc["id"].split(b"\n")[:-1]]
    want = b"".join(ref.decode_ids(r, options)[0] + b"\n" for r in rows)
    p = _decode(["--input_format=id", "--extra_options=" + options, "--batch_lines=64"], enc["id"], path)
    assert p.returncode == 0 and p.stdout == want
    p = _decode(["--input_format=id", "--output_format=proto", "--extra_options=" + options], enc["id"], path)
    assert p.returncode == 0 and p.stdout == b""  # decodes and prints nothing, as the reference does


@pytest.mark.parametrize("path", ["device", "host"])
def test_pieces_outside_the_vocabulary_and_split(path):
    ref = decode_ref.Model(open(MODEL, "rb").read())
    ws = C.WS.encode()
    lines = [ws + b"I  " + ws + b"saw \xe7\x8c\xab " + ws, b"", b" <unk> <s> " + ws + b"a", ws + b"I"]
    want = b"".join(ref.decode_pieces([f for f in l.split(b" ") if f])[0] + b"\n" for l in lines)
    p = _decode([], b"".join(l + b"\n" for l in lines), path)  # --input_format=piece is the default
    assert p.returncode == 0 and p.stdout == want
    assert b"\xe7\x8c\xab" in p.stdout  # the out-of-vocabulary piece came through verbatim


def test_errors_and_two_files(head, tmp_path):
    d, enc, want = head
    bad = _decode(["--extra_options=foo"], b"x\n", "host")
    assert bad.returncode != 0 and b'option "foo" is not available.' in bad.stderr
    bad = _decode(["--input_format=id"], b"3 100000\n", "device")
    assert bad.returncode != 0 and b"id 100000" in bad.stderr
    assert _decode(["--input_format=nope"], b"", "host").returncode != 0
    rows = enc["id"].split(b"\n")[:-1]
    a, b = tmp_path / "a.ids", tmp_path / "b.ids"
    a.write_bytes(b"".join(r + b"\n" for r in rows[:120]))
    b.write_bytes(b"".join(r + b"\n" for r in rows[120:]))
    out = tmp_path / "out.txt"
    p = _decode(["--input_format=id", "--output=%s" % out, "--batch_lines=50", str(a), str(b)], b"", "device")
    assert p.returncode == 0 and out.read_bytes() == want
