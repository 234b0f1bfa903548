#!/usr/bin/env python3
"""CPU model of the unigram byte kernel's output stage: what a per-lane
backtrace pays for wave lockstep, and what a tile-balanced lookup would, for a
model file and a corpus.

  tools/backtrace_model.py MODEL --synth N [--seed S]      N sentences of tools/synth.py
  tools/backtrace_model.py MODEL --corpus FILE [--lines K] lines of a text file, each taken
                                                           as "▁" + its words joined by "▁"

The model follows the kernel's tiling (unigram_encode.hip): tiles of 256
sentences sorted by length, 64 lanes per wave.  Sentences are encoded with the
CPU oracle; only token counts enter.  A per-lane backtrace runs in a wave as
many rounds as its longest lane has tokens; a lookup that takes the tile's
tokens 256 at a time runs ceil(tile tokens / 256) rounds with every lane busy
(but the last round's).

Printed (means over all waves, or tiles):
  lockstep rounds per wave     max over the wave's 64 lanes of their token count
  tokens per lane              the work a lane really has; its ratio to the
                               rounds is the backtrace's lane occupancy
  tile tokens mean / max       against the LDS stage of 1264 entries
  tiles over the stage         tiles whose tokens need more than one window
  balanced rounds per wave     ceil(tile tokens / 256)
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "sentencepiece-comments_amd"))

WS = "▁".encode()
STAGE = 1264


def token_counts(model_bytes, sents):
    import numpy as np
    import oracle_lib
    import spm_amd
    counts = []
    om = oracle_lib.OracleModel(model_bytes)
    for k in range(0, len(sents), 65536):
        buf, off = spm_amd.to_csr(sents[k:k + 65536])
        to = om.encode_normalized_csr(buf, off, with_lens=True)[2]
        counts += np.diff(to.astype(np.int64)).tolist()
    return counts


def run(name, sents, counts, out):
    n = len(sents) // 256 * 256
    if n == 0:
        sys.exit("need at least 256 sentences")
    rounds = tokens = balanced = over = 0
    totals = []
    for t in range(n // 256):
        order = sorted(range(t * 256, (t + 1) * 256), key=lambda i: len(sents[i]))
        tile = [counts[i] for i in order]
        tot = sum(tile)
        totals.append(tot)
        over += tot > STAGE
        balanced += -(-tot // 256)
        for w in range(4):
            lanes = tile[w * 64:(w + 1) * 64]
            rounds += max(lanes)
            tokens += sum(lanes)
    waves, tiles = n // 64, n // 256
    print("## %s: %d sentences, %d waves, %d tiles" % (name, n, waves, tiles), file=out)
    print("lockstep rounds per wave %.2f, tokens per lane %.2f (lane occupancy %.0f %%)" % (
        rounds / waves, tokens / (64.0 * waves), 100.0 * tokens / (64.0 * rounds)), file=out)
    print("tile tokens mean %.0f max %d, tiles over the %d-entry stage %d of %d" % (
        sum(totals) / tiles, max(totals), STAGE, over, tiles), file=out)
    print("balanced rounds per wave %.2f" % (balanced / tiles), file=out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("model")
    ap.add_argument("--synth", type=int, default=0, help="sentences of tools/synth.py (normalized)")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--corpus", default=None, help="text file, one sentence per line")
    ap.add_argument("--lines", type=int, default=0, help="use the first K lines of the corpus (0: all)")
    ap.add_argument("--out", default=None, help="append the report to this file instead of printing it")
    a = ap.parse_args()
    mb = open(a.model, "rb").read()
    if a.corpus:
        lines = [l for l in open(a.corpus, "rb").read().split(b"\n") if l.strip()]
        if a.lines:
            lines = lines[:a.lines]
        sents = [WS + WS.join(l.split()) for l in lines]
        name = "%s with %s" % (os.path.basename(a.corpus), os.path.basename(a.model))
    else:
        import synth
        buf, off = synth.normalized(a.synth or 102400, seed=a.seed)
        bb = buf.tobytes()
        sents = [bb[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]
        name = "synth.normalized seed %d with %s" % (a.seed, os.path.basename(a.model))
    out = open(a.out, "a") if a.out else sys.stdout
    run(name, sents, token_counts(mb, sents), out)


if __name__ == "__main__":
    main()
