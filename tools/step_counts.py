#!/usr/bin/env python3
"""Static instruction counts per walk step of a kernel, from device assembly.

  hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S csrc/unigram_encode.hip -o k.s
  tools/step_counts.py k.s [kernel-symbol-substring]

A walk step of the unigram byte kernel issues one pair of buffer_load_dwordx2
(the two positions' (unit, score) gathers).  For every stretch of the kernel's
text between two consecutive pairs this prints the number of lines whose
mnemonic starts with v_ and with s_ (by prefix only: s_waitcnt, s_cbranch and
s_nop count as s_), plus how many of the v_ lines are v_cndmask / v_cmp and
how many s_ lines are saveexec.  The counts are static: both sides of a branch
inside a stretch are counted.
"""
import re
import sys

DEFAULT = "unigram_fast_kernelILi16ELb1ELi7ELb0ELb0E"


def kernel_body(lines, sub):
    start = end = None
    for n, ln in enumerate(lines):
        if start is None and ln.startswith("_Z") and sub in ln and ln.split(";")[0].rstrip().endswith(":"):
            start = n
        elif start is not None and ln.startswith(".Lfunc_end"):
            end = n
            break
    if start is None or end is None:
        sys.exit("kernel %r not found" % sub)
    return lines[start + 1:end]


def main():
    path = sys.argv[1]
    sub = sys.argv[2] if len(sys.argv) > 2 else DEFAULT
    body = kernel_body(open(path).read().split("\n"), sub)
    ops = []
    for ln in body:
        m = re.match(r"\s+([a-z_0-9]+)", ln)
        if m and not ln.lstrip().startswith((".", ";")):
            ops.append(m.group(1))
    loads = [n for n, o in enumerate(ops) if o == "buffer_load_dwordx2"]
    # A pair: two gathers at most 8 instructions apart.
    pairs, n = [], 0
    while n < len(loads):
        if n + 1 < len(loads) and loads[n + 1] - loads[n] <= 8:
            pairs.append((loads[n], loads[n + 1]))
            n += 2
        else:
            pairs.append((loads[n], loads[n]))
            n += 1
    print("# %s: %d instructions, %d buffer_load_dwordx2, %d pairs" % (sub, len(ops), len(loads), len(pairs)))
    print("# step  v_  s_  v_cndmask  v_cmp  saveexec  v_mov  (between the second load of a pair and the first of the next)")
    tv = ts = 0
    for k in range(len(pairs) - 1):
        seg = ops[pairs[k][1] + 1:pairs[k + 1][0]]
        v = sum(o.startswith("v_") for o in seg)
        s = sum(o.startswith("s_") for o in seg)
        print("%4d %4d %4d %6d %6d %6d %6d" % (
            k, v, s, sum(o.startswith("v_cndmask") for o in seg), sum(o.startswith("v_cmp") for o in seg),
            sum("saveexec" in o for o in seg), sum(o.startswith("v_mov") for o in seg)))
        tv += v
        ts += s
    print("# total between pairs: v_ %d  s_ %d" % (tv, ts))
    print("# whole kernel: v_ %d  s_ %d" % (sum(o.startswith("v_") for o in ops), sum(o.startswith("s_") for o in ops)))


if __name__ == "__main__":
    main()
