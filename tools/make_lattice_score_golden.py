#!/usr/bin/env python3
"""Records the `sentencepiece` package's calculate_entropy answers as
tests/golden/*.entropy.gz: for every line of a corpus under a unigram fixture,
at alpha 0, 0.5 and 1, the float32 the package returns.  A file holds the
three alphas one after the other (3 * lines raw little-endian float32,
gzipped); results only.

  python tools/make_lattice_score_golden.py [--check]
"""
import argparse
import gzip
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ALPHAS = (0.0, 0.5, 1.0)
# (name of the golden, corpus, model)
FIXTURES = (
    ("botchan_test_model", "botchan.txt", "test_model.model"),
    ("botchan_bf_unigram1k", "botchan.txt", "botchan_bf_unigram1k.model"),
    ("wagahaiwa_test_ja_model", "wagahaiwa_nekodearu.txt", "test_ja_model.model"),
)


def corpus_lines(name):
    """The corpus' lines as the package sees them (text, no newline)."""
    with open(os.path.join(GOLD, name), "rb") as f:
        return [l.rstrip(b"\n") for l in f.read().split(b"\n")[:-1]]


def package_entropies(model_name, corpus, alphas=ALPHAS, lines=None):
    import sentencepiece
    sp = sentencepiece.SentencePieceProcessor(model_file=os.path.join(GOLD, model_name))
    texts = [l.decode() for l in (corpus_lines(corpus) if lines is None else lines)]
    return np.array([[sp.calculate_entropy(t, a) for t in texts] for a in alphas], dtype=np.float32)


def golden_path(name):
    return os.path.join(GOLD, name + ".entropy.gz")


def read_golden(name):
    """float32[len(ALPHAS), lines]."""
    with gzip.open(golden_path(name), "rb") as f:
        return np.frombuffer(f.read(), dtype="<f4").reshape(len(ALPHAS), -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare instead of writing")
    args = ap.parse_args()
    for name, corpus, model_name in FIXTURES:
        h = package_entropies(model_name, corpus)
        if args.check:
            ok = np.array_equal(read_golden(name).view(np.uint32), h.view(np.uint32))
            print("%s: %s" % (name, "equal" if ok else "DIFFERENT"))
            if not ok:
                sys.exit(1)
            continue
        with gzip.GzipFile(golden_path(name), "wb", mtime=0) as f:
            f.write(h.astype("<f4").tobytes())
        print("%s: %d lines x %d alphas, %d bytes" % (name, h.shape[1], h.shape[0], os.path.getsize(golden_path(name))))


if __name__ == "__main__":
    main()
