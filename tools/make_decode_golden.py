#!/usr/bin/env python3
"""Writes the decode fixtures tests/golden/<name>.decoded.gz.

Each committed golden id file (one line of space-separated ids per input
line) is decoded with the Python `sentencepiece` package, row by row, and the
texts are stored one per line.  The fixtures guard tests/decode_ref.py, the
restatement the decode tests compare against, from a misreading shared with
the code under test.  Run once, by hand, where the package is installed:

    python tools/make_decode_golden.py
"""
import gzip
import os

import sentencepiece

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SETS = (("botchan_test_model", "test_model.model"), ("wagahaiwa_test_ja_model", "test_ja_model.model"))


def main():
    for name, model in SETS:
        sp = sentencepiece.SentencePieceProcessor(model_file=os.path.join(GOLD, model))
        rows = [[int(x) for x in line.split()] for line in open(os.path.join(GOLD, name + ".ids"))]
        texts = [sp.decode(r) for r in rows]
        assert not any("\n" in t for t in texts)
        data = "".join(t + "\n" for t in texts).encode("utf-8")
        path = os.path.join(GOLD, name + ".decoded.gz")
        with open(path, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", mtime=0, filename="") as g:
            g.write(data)
        print("%s: %d rows, %d bytes (sentencepiece %s)" % (path, len(rows), len(data), sentencepiece.__version__))


if __name__ == "__main__":
    main()
