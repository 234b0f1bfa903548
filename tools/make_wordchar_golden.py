#!/usr/bin/env python3
"""Writes the WORD / CHAR fixtures under tests/golden/.

Three small models are trained with the Python `sentencepiece` package from
the committed corpora only (identity normalization keeps them small), and
every line of the model's corpus is encoded and decoded with the package:

    <name>.model        the trained model
    <name>.ids.gz       final ids, one row per line (unknown runs merged)
    <name>.ids_ber.gz   the same under extra options bos:eos:reverse
    <name>.pieces.gz    final pieces, tab-separated
    <name>.decoded.gz   the package's decode of the plain id rows

The fixtures pin tests/wordchar_ref.py, the restatement the WORD / CHAR tests
compare against, to the package.  Run once, by hand, where it is installed:

    python tools/make_wordchar_golden.py
"""
import gzip
import os

import sentencepiece as spm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SETS = (
    ("botchan_char60", "botchan.txt", "char", 60),
    ("wagahaiwa_char2000", "wagahaiwa_nekodearu.txt", "char", 2000),
    ("botchan_word2000", "botchan.txt", "word", 2000),
)


def _gz(path, text):
    with open(path, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", mtime=0, filename="") as g:
        g.write(text.encode("utf-8"))


def _rows(rows):
    return "".join(" ".join(str(i) for i in r) + "\n" for r in rows)


def main():
    for name, corpus, kind, vocab in SETS:
        src = os.path.join(GOLD, corpus)
        # The trainer spec keeps `input` and `model_prefix` as given: relative
        # names from the fixture directory keep the model free of local paths
        # and the same on every run.
        cwd = os.getcwd()
        os.chdir(GOLD)
        try:
            prefix = "_" + name
            spm.SentencePieceTrainer.train(input=corpus, model_prefix=prefix, model_type=kind, vocab_size=vocab,
                                           normalization_rule_name="identity", minloglevel=2)
            model = open(prefix + ".model", "rb").read()
            os.remove(prefix + ".model")
            os.remove(prefix + ".vocab")
        finally:
            os.chdir(cwd)
        open(os.path.join(GOLD, name + ".model"), "wb").write(model)
        lines = [l.decode("utf-8") for l in open(src, "rb").read().split(b"\n")]
        if lines and lines[-1] == "":
            lines.pop()
        sp = spm.SentencePieceProcessor(model_proto=model)
        ids = sp.encode(lines, out_type=int)
        _gz(os.path.join(GOLD, name + ".ids.gz"), _rows(ids))
        # The extra options apply in order, so "bos:eos:reverse" reverses the
        # row with its bos and eos; the package's own `reverse` flag reverses
        # first, so the rows are encoded with bos and eos and reversed here.
        ber = spm.SentencePieceProcessor(model_proto=model, add_bos=True, add_eos=True)
        _gz(os.path.join(GOLD, name + ".ids_ber.gz"), _rows(r[::-1] for r in ber.encode(lines, out_type=int)))
        pieces = sp.encode(lines, out_type=str)
        assert not any("\t" in p or "\n" in p or " " in p for r in pieces for p in r)
        _gz(os.path.join(GOLD, name + ".pieces.gz"), "".join("\t".join(r) + "\n" for r in pieces))
        texts = [sp.decode(r) for r in ids]
        assert not any("\n" in t for t in texts)
        _gz(os.path.join(GOLD, name + ".decoded.gz"), "".join(t + "\n" for t in texts))
        print("%s: %d bytes, %d lines (sentencepiece %s)" % (name, len(model), len(lines), spm.__version__))


if __name__ == "__main__":
    main()
