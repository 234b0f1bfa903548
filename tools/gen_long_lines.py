#!/usr/bin/env python3
"""Long raw lines for per-line latency runs (lib/spm_latency): consecutive
lines of a corpus joined with single spaces until a length drawn uniformly
from [--min, --max] bytes would be passed.  Fixed seed, so the file is the
same everywhere.

  tools/gen_long_lines.py tests/golden/botchan.txt out.txt [--lines 500] [--min 200] [--max 1000]
"""
import argparse
import random


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("corpus")
    ap.add_argument("out")
    ap.add_argument("--lines", type=int, default=500)
    ap.add_argument("--min", type=int, default=200)
    ap.add_argument("--max", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=24)
    a = ap.parse_args()
    src = [l for l in open(a.corpus, "rb").read().split(b"\n") if l]
    rng = random.Random(a.seed)
    out, k = [], 0
    while len(out) < a.lines:
        want = rng.randint(a.min, a.max)
        line = src[k % len(src)]
        k += 1
        while len(line) + 1 + len(src[k % len(src)]) <= want:
            line += b" " + src[k % len(src)]
            k += 1
        if len(line) < a.min:  # the next corpus line alone would pass `want`: cut it
            line = (line + b" " + src[k % len(src)])[:want]
            k += 1
        out.append(line)
    with open(a.out, "wb") as f:
        f.write(b"".join(l + b"\n" for l in out))
    sizes = [len(l) for l in out]
    print("%d lines, %d..%d bytes, mean %.0f" % (len(out), min(sizes), max(sizes), sum(sizes) / len(sizes)))


if __name__ == "__main__":
    main()
