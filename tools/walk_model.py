#!/usr/bin/env python3
"""CPU model of the unigram byte kernel's forward walk: what a wave's walk
steps are spent on, for a model file and a corpus.

  tools/walk_model.py MODEL --synth N [--seed S]      N sentences of tools/synth.py
  tools/walk_model.py MODEL --corpus FILE [--lines K] lines of a text file, each taken
                                                      as "▁" + its words joined by "▁"

The model follows the kernel's tiling (unigram_encode.hip): tiles of 256
sentences sorted by length, 64 lanes per wave, groups of four byte positions,
two positions (a pair) walked together, walks of at most 15 bytes.  A walk
from a char start that matches L bytes of the trie takes L + 1 label tests
(the last one fails; 15 at most); a pair takes as many steps as the longest
walk of its 128 (lane, position) chains.  Only trie prefixes are modelled,
not scores: the figures say where steps go, not what they cost.

Printed per wave (means over all waves):
  pair-steps by depth d    pairs whose walk reaches step d (their sum is the
                           wave's pair-steps)
  alive lanes by depth d   lanes (of 64) whose walk matched d bytes, summed over
                           all positions and divided (row 1) by the positions
                           at which some lane of the wave starts a char, (row 2)
                           by the positions the wave still walks at depth d, that
                           is where some lane tests a label there.  Row 2 is the
                           occupancy of a deep step and is the larger one; the
                           figures quoted when the merged walk was proposed (46,
                           13, 9.2, ...) came from a normalisation that was not
                           written down; they lie near row 2 and are not
                           reproduced digit for digit.
  two-chain lanes at D     (lane, pair) with both chains alive at depth D, and
                           the share of pairs that hold such a lane, D = 3..6
  merged scheme at D       steps 1..D walk both chains; past D a lane carries
                           one chain (pass A) and the lanes with two chains
                           alive at D walk the second in pass B: two-chain
                           steps, pass-A steps, pass-B steps per wave
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

W = 16
WS = "▁".encode()
DEPTHS = (3, 4, 5, 6)


def load_prefixes(path):
    import model_reader
    pref = set()
    for p in model_reader.read_pieces(open(path, "rb").read()):
        b = p[0] if isinstance(p[0], bytes) else p[0].encode()
        if len(b) >= W:
            continue
        for n in range(1, len(b) + 1):
            pref.add(b[:n])
    return pref


def walk_steps(s, pref):
    """steps[p]: label tests of the walk from byte position p (matched bytes +
    the failing test, at most W - 1); 0 where p is no char start."""
    nb = len(s)
    steps = [0] * (nb + 8)
    p = 0
    while p < nb:
        c = s[p]
        cl = 1 if c < 0x80 else 2 if c < 0xE0 else 3 if c < 0xF0 else 4
        n = 0
        while n < W - 1 and p + n < nb and s[p:p + n + 1] in pref:
            n += 1
        steps[p] = min(n + 1, W - 1)
        p += min(cl, nb - p)
    return steps


def run(name, sents, pref, out):
    n = len(sents) // 256 * 256
    if n == 0:
        sys.exit("need at least 256 sentences")
    pair_by_depth = [0] * W
    alive = [0] * W
    positions = 0
    positions_at = [0] * W
    pairs = 0
    scheme = {d: dict(two=0, a=0, b=0, lanes2=0, pairs2=0) for d in DEPTHS}
    for t in range(n // 256):
        tile = sorted(sents[t * 256:(t + 1) * 256], key=len)
        for w in range(4):
            lanes = [walk_steps(s, pref) for s in tile[w * 64:(w + 1) * 64]]
            longest = max(len(s) for s in tile[w * 64:(w + 1) * 64])
            for p0 in range(0, longest + 1, 4):
                for jb in (0, 2):
                    a = [x[p0 + jb] if p0 + jb < len(x) else 0 for x in lanes]
                    b = [x[p0 + jb + 1] if p0 + jb + 1 < len(x) else 0 for x in lanes]
                    for col in (a, b):
                        if max(col):
                            positions += 1
                            for d in range(1, max(col) + 1):
                                positions_at[d] += 1
                            for x in col:
                                for d in range(1, x):  # matched x - 1 bytes
                                    alive[d] += 1
                    m = max(max(a), max(b))
                    if m == 0:
                        continue
                    pairs += 1
                    for d in range(1, m + 1):
                        pair_by_depth[d] += 1
                    for D, r in scheme.items():
                        r["two"] += min(m, D)
                        # alive at depth D: the walk matched >= D bytes, steps > D
                        two = [(x, y) for x, y in zip(a, b) if x > D and y > D]
                        r["lanes2"] += len(two)
                        r["pairs2"] += bool(two)
                        if m > D:
                            r["a"] += max(x if x > D else y for x, y in zip(a, b)) - D
                            if two:
                                r["b"] += max(y for _, y in two) - D
    waves = n // 64
    now = sum(pair_by_depth)
    print("## %s: %d sentences, %d waves" % (name, n, waves), file=out)
    print("pair-steps per wave %.1f over %.1f pairs" % (now / waves, pairs / waves), file=out)
    print("pair-steps per wave by depth 1..%d: %s" % (W - 1, " ".join("%.1f" % (pair_by_depth[d] / waves)
                                                                     for d in range(1, W))), file=out)
    print("alive lanes of 64 per position by depth 1..%d: %s" % (W - 2, " ".join("%.1f" % (alive[d] / max(positions, 1))
                                                                                for d in range(1, W - 1))), file=out)
    print("alive lanes of 64 per position still walked at that depth, 1..%d: %s" % (
        W - 2, " ".join("%.1f" % (alive[d] / max(positions_at[d], 1)) for d in range(1, W - 1))), file=out)
    for D, r in scheme.items():
        print("D=%d: two-chain lanes per wave %.3f, in %.2f %% of pairs | steps per wave: two-chain %.1f, pass A %.1f, "
              "pass B %.2f (now %.1f pair-steps)" % (D, r["lanes2"] / waves, 100.0 * r["pairs2"] / max(pairs, 1),
                                                     r["two"] / waves, r["a"] / waves, r["b"] / waves, now / waves),
              file=out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("model")
    ap.add_argument("--synth", type=int, default=0, help="sentences of tools/synth.py (normalized)")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--corpus", default=None, help="text file, one sentence per line")
    ap.add_argument("--lines", type=int, default=0, help="use the first K lines of the corpus (0: all)")
    ap.add_argument("--out", default=None, help="append the report to this file instead of printing it")
    a = ap.parse_args()
    pref = load_prefixes(a.model)
    if a.corpus:
        lines = [l for l in open(a.corpus, "rb").read().split(b"\n") if l.strip()]
        if a.lines:
            lines = lines[:a.lines]
        sents = [WS + WS.join(l.split()) for l in lines]
        name = "%s with %s" % (os.path.basename(a.corpus), os.path.basename(a.model))
    else:
        import synth
        buf, off = synth.normalized(a.synth or 256 * 120, seed=a.seed)
        bb = buf.tobytes()
        sents = [bb[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]
        name = "synth.normalized seed %d with %s" % (a.seed, os.path.basename(a.model))
    out = open(a.out, "a") if a.out else sys.stdout
    run(name, sents, pref, out)


if __name__ == "__main__":
    main()
