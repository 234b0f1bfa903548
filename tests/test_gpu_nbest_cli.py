"""GPU: spm_encode --output_format=nbest_id|nbest_piece against the fixtures
made with the pip sentencepiece, and the C++ processor's NBestEncode."""
import os
import subprocess

import pytest

import nbest_ref as NB
import oracle_lib as O
import spm_amd as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
LIB = os.path.join(ROOT, "sentencepiece-comments_amd", "lib")
CLI = os.path.join(LIB, "spm_encode")
pytestmark = pytest.mark.gpu

CASES = [("test_model.model", "botchan.txt", 200, 5, "botchan_test_model.nbest5.gz"),
         ("test_ja_model.model", "wagahaiwa_nekodearu.txt", 60, 4, "wagahaiwa_test_ja_model.nbest4.gz")]


def _input(tmp_path, text, count):
    lines = O.read_lines_binary(os.path.join(GOLD, text))[:count]
    p = tmp_path / "in.txt"
    p.write_bytes(b"".join(l + b"\n" for l in lines))
    return str(p), lines


def _run(model, args, tmp_path, name="out.txt"):
    out = tmp_path / name
    subprocess.check_call([CLI, "--model=" + os.path.join(GOLD, model)] + args + ["--output=%s" % out], timeout=120)
    return out.read_bytes()


def _fixture_rows(fixture):
    return NB.read_fixture(os.path.join(GOLD, fixture))


@pytest.mark.parametrize("model,text,count,nbest,fixture", CASES)
def test_nbest_id_is_the_fixture(tmp_path, model, text, count, nbest, fixture):
    path, _ = _input(tmp_path, text, count)
    _, want = _fixture_rows(fixture)
    assert _run(model, ["--output_format=nbest_id", "--nbest_size=%d" % nbest, path], tmp_path) == want
    # Batches of 33 lines print the same rows.
    assert _run(model, ["--output_format=nbest_id", "--nbest_size=%d" % nbest, "--batch_lines=33", path], tmp_path,
                "b.txt") == want


def test_nbest_piece_rows_join_back(tmp_path):
    model, text, count, nbest, fixture = CASES[0]
    path, lines = _input(tmp_path, text, count)
    rows, _ = _fixture_rows(fixture)
    got = _run(model, ["--output_format=nbest_piece", "--nbest_size=%d" % nbest, path], tmp_path).split(b"\n")[:-1]
    norm = S.DeviceModel(open(os.path.join(GOLD, model), "rb").read(), host_only=True).normalize(lines)
    k = 0
    for line_rows, want in zip(rows, norm):
        for ids in line_rows:
            # (split on the separator only: "\r" is a piece of this model)
            assert len(got[k].split(b" ")) == len(ids)
            assert got[k].replace(b" ", b"") == want
            k += 1
    assert k == len(got)


def test_extra_options_bracket_every_path(tmp_path):
    model, text, count, nbest, fixture = CASES[0]
    path, _ = _input(tmp_path, text, count)
    rows, _ = _fixture_rows(fixture)
    got = _run(model, ["--output_format=nbest_id", "--nbest_size=%d" % nbest, "--extra_options=bos:eos", path],
               tmp_path)
    bos, eos = 1, 2  # <s>, </s> of test_model.model
    assert got == "".join(" ".join(map(str, [bos] + r + [eos])) + "\n" for line in rows for r in line).encode()


def test_processor_status_codes():
    run = lambda model, n: subprocess.run([os.path.join(LIB, "nbest_selftest"), "proc", os.path.join(GOLD, model),
                                           str(n), "hello world"], capture_output=True, timeout=60)
    p = run("botchan_bpe1k.model", 5)
    assert p.returncode == 0 and p.stdout.split() == [b"13"]  # INTERNAL "NBestEncode returns empty result."
    p = run("test_model.model", 5)
    assert p.returncode == 0 and p.stdout.split() == [b"0"]
