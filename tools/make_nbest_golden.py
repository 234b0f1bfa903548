"""Generate the n-best id fixtures (test infrastructure).

As tools/make_golden.py does for the plain encode, this writes small fixtures
under tests/golden/ with the installed reference-family pip `sentencepiece`
(v0.2.2), whose Lattice::NBest is the reference's except that it shrinks the
agenda at 10 000 entries instead of 100 000:

  botchan_test_model.nbest5.gz        first 200 botchan lines, nbest_size 5
  wagahaiwa_test_ja_model.nbest4.gz   first 60 wagahaiwa lines, nbest_size 4

Format, per input line: the path count, then one row of ids per path (what
`spm_encode --output_format=nbest_id` prints for the line).  The rows are
processor level (unknown runs merged).  Scores are not recorded: 0.2.2
reports fx, the reference the left-to-right sum.

Guard: the restatement (tests/nbest_ref.py) is run over every chosen line and
must never see an agenda of 10 000 entries, so the 0.2.2 threshold cannot
matter; it must also reproduce every row.  The files are gzip streams
(277 KB of digits as text) written with a zero timestamp, so a re-run gives
the same bytes.

Usage: python tools/make_nbest_golden.py
"""
import gzip
import hashlib
import os
import sys

import sentencepiece as spm

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "..", "tests", "golden")
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, os.path.join(HERE, "..", "sentencepiece-comments_amd"))

FIXTURES = [("test_model.model", "botchan.txt", 200, 5, "botchan_test_model.nbest5.gz"),
            ("test_ja_model.model", "wagahaiwa_nekodearu.txt", 60, 4, "wagahaiwa_test_ja_model.nbest4.gz")]


def make(model, text, count, nbest, out):
    import nbest_ref
    import sample_ref
    import spm_amd
    mb = open(os.path.join(GOLD, model), "rb").read()
    sp = spm.SentencePieceProcessor()
    sp.LoadFromSerializedProto(mb)
    lines = open(os.path.join(GOLD, text), "rb").read().split(b"\n")[:count]
    norm = spm_amd.DeviceModel(mb, host_only=True).normalize(lines)
    ref = sample_ref.Model(mb)
    text = []
    for ln, nz in zip(lines, norm):
        rows = sp.NBestEncodeAsIds(ln.decode("utf-8"), nbest)
        paths, (_, agenda) = nbest_ref.nbest(ref, nz, nbest)
        assert agenda < 10000, (out, ln, agenda)
        assert [nbest_ref.merge_unknown(p[0], ref.unk_id) for p in paths] == rows, (out, ln)
        text.append("%d\n" % len(rows))
        text += [" ".join(map(str, r)) + "\n" for r in rows]
    with open(os.path.join(GOLD, out), "wb") as raw:
        with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
            f.write("".join(text).encode())
    h = hashlib.sha256(open(os.path.join(GOLD, out), "rb").read()).hexdigest()
    print(out, len(lines), "lines sha256", h, "spm", spm.__version__)


if __name__ == "__main__":
    for fx in FIXTURES:
        make(*fx)
