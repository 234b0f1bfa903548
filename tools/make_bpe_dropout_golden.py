#!/usr/bin/env python3
"""Records the `sentencepiece` package's BPE-dropout draw counts as
tests/golden/bpe_dropout_counts.json.gz: for a dozen short inputs under the
BPE fixtures (and two hand models of tests/bpe_cases.py, where the package
loads them), at alpha 0.1 and 0.5, DRAWS calls of
encode(text, enable_sampling=True, alpha=alpha, nbest_size=-1) counted by
segmentation.  A segmentation is written as its pieces' byte lengths in the
normalized sentence, a run of unknown tokens (byte pieces under byte fallback)
as one piece, as the package merges them.  Results only; runs on the CPU, by
hand, once: the package's generator cannot be seeded per call, so a second
run gives other counts of the same distribution.

  python tools/make_bpe_dropout_golden.py
"""
import collections
import gzip
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUT = os.path.join(GOLD, "bpe_dropout_counts.json.gz")
DRAWS = 200000
ALPHAS = (0.1, 0.5)
TEXTS = ("the teacher", "hello world", "Botchan", "unbelievable", "a", "zzz qqq", "I am 日本", "xyz ß", "it's 東京 now",
         "Mr. Brown", "school", "ん")
# model key -> (loader, texts): a fixture file, or a hand model by its
# bpe_cases.build_model keywords.
HAND_TEXTS = {
    "hand:unused": ("aaaa", "abcabc", "bbbb cc", "aabbaacc", "éüあい", "abzab"),
    "hand:user_defined": ("ab<tag>cd", "<tag>", "aa<tag><tag>bb", "a<tagb"),
}
HAND_KW = {"hand:unused": dict(unused=True), "hand:user_defined": dict(user_defined=True)}


def model_blob(key):
    if key.startswith("hand:"):
        import bpe_cases
        return bpe_cases.build_model(**HAND_KW[key]).blob
    with open(os.path.join(GOLD, key), "rb") as f:
        return f.read()


def hand_texts(key):
    """HAND_TEXTS plus, for the UNUSED model, some of its UNUSED pieces as
    whole inputs (each pushes itself and is resegmented)."""
    out = list(HAND_TEXTS[key])
    if key == "hand:unused":
        import bpe_cases
        out += bpe_cases.UNUSED_PIECES[:4]
    return out


def count(sp, text, alpha, draws, byte_fallback):
    unk = sp.unk_id()
    c = collections.Counter()
    for pieces in sp.encode([text] * draws, out_type=str, enable_sampling=True, alpha=alpha, nbest_size=-1):
        lens, in_unk = [], False
        for p in pieces:
            i = sp.piece_to_id(p)
            is_byte = byte_fallback and sp.is_byte(i)
            u = i == unk or is_byte
            n = 1 if is_byte else len(p.encode())
            if u and in_unk:
                lens[-1] += n
            else:
                lens.append(n)
            in_unk = u
        c[tuple(lens)] += 1
    return c


def main():
    import sentencepiece
    cases = []
    for key in ("botchan_bpe1k.model", "botchan_bf_bpe1k.model", "hand:unused", "hand:user_defined"):
        try:
            sp = sentencepiece.SentencePieceProcessor(model_proto=model_blob(key))
        except Exception as e:  # the package refuses the hand model: leave it out
            print("%s: not loaded by the package (%s)" % (key, e))
            continue
        texts = hand_texts(key) if key.startswith("hand:") else TEXTS
        for text in texts:
            norm = sp.normalize(text)
            for alpha in ALPHAS:
                c = count(sp, text, alpha, DRAWS, "bf_" in key)
                assert all(sum(k) == len(norm.encode()) for k in c), (key, text)
                cases.append({"model": key, "text": text, "norm": norm, "alpha": alpha, "draws": DRAWS,
                              "counts": sorted(([list(k), v] for k, v in c.items()), key=lambda kv: (-kv[1], kv[0]))})
                print("%s %r alpha %.1f: %d segmentations" % (key, text, alpha, len(c)))
    with gzip.GzipFile(OUT, "wb", mtime=0) as f:
        f.write(json.dumps({"cases": cases}, ensure_ascii=False, separators=(",", ":")).encode())
    print("%s: %d cases, %d bytes" % (OUT, len(cases), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
