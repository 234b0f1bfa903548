#!/usr/bin/env python3
"""Static instruction counts per walk step of a kernel, from device assembly.

  hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S csrc/unigram_encode.hip -o k.s
  tools/step_counts.py k.s [kernel-symbol-substring]
  tools/step_counts.py --prologue k.s [kernel-symbol-substring]   (see prologue())

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


def count(seg):
    return {"v_": sum(o.startswith("v_") for o in seg), "s_": sum(o.startswith("s_") for o in seg),
            "branch": sum(o.startswith(("s_cbranch", "s_branch")) for o in seg),
            "lds": sum(o.startswith("ds_") for o in seg),
            "store": sum(o.startswith(("buffer_store", "global_store")) for o in seg)}


def fmt(c):
    return "v_ %3d  s_ %3d (branches %2d)  ds_ %d  stores %d" % (c["v_"], c["s_"], c["branch"], c["lds"], c["store"])


REG = re.compile(r"^(v\d+|v\[\d+:\d+\]|s\d+|s\[\d+:\d+\])$")


def is_reg_move(op, arg):
    """A vector move whose source is a register: it computes nothing."""
    if not op.startswith(("v_mov_b32", "v_mov_b64", "v_pk_mov_b32")):
        return False
    parts = [x.strip() for x in arg.split(",")]
    return len(parts) >= 2 and bool(REG.match(parts[1]))


def prologue(ops, sub, args):
    """--prologue: the byte kernel's forward pass outside its walk steps.

    pair prologue k: the stretch that ends at pair k's two root-table reads
      (two adjacent ds_read_b64) and starts after the nearest unconditional
      s_branch before them: char starts, the first position's back-pointer
      store, the root reads' addresses (pair 0's stretch begins with the
      loop's latch).
    back-pointer store: every byte store of the forward loop with its guard,
      from the s_and_saveexec that opens it to the s_or_b64 exec that closes it.
    group epilogue: the stretch between two unconditional branches that holds
      the window's splice (the first v_alignbyte_b32 after the last root
      read): back-pointer word store, ring shift, window advance.  Blocks laid
      out behind the closing branch (the byte-wise tail of the batch's last
      partial dword, a guarded load) are not in it.
    The three rows under it split the group's end, from the branch before the
    shift to the closing branch:
      ring shift: the last cluster of three or more register-to-register
        vector moves before the splice (at most 8 instructions apart): score ring,
        back-pointer words and whatever of the window's rotation sits there,
        32-bit and 64-bit moves counted apart.
      window advance: the vector instructions other than such moves from the
        last back-pointer store (or the stretch's start) to the closing
        branch, and the loads among them.  It holds the one compare of the
        near-tie mask's refresh.
      the rest: every other vector instruction from the branch before the
        shift to the closing branch (back-pointer stores, defaults)."""
    roots = [n for n in range(len(ops) - 1) if ops[n] == "ds_read_b64" and ops[n + 1] == "ds_read_b64"]
    if not roots:
        sys.exit("no root-table reads (not a byte-kernel instantiation)")
    print("# %s: %d instructions, %d pair prologues" % (sub, len(ops), len(roots)))

    def back_to_branch(n):
        while n > 0 and ops[n - 1] != "s_branch":
            n -= 1
        return n

    for k, r in enumerate(roots):
        print("pair prologue %d        %s" % (k, fmt(count(ops[back_to_branch(r):r]))))
    win = next(n for n in range(roots[-1], len(ops)) if ops[n] == "v_alignbyte_b32")
    stores = [n for n in range(roots[0] - 80, win) if ops[n] in ("ds_write_b8", "ds_write_b8_d16_hi", "buffer_store_byte")]
    # A site: the stores at most 12 instructions apart (the scratch and the LDS side of one guarded store).
    groups = []
    for n in stores:
        if groups and n - groups[-1][-1] <= 12:
            groups[-1].append(n)
        else:
            groups.append([n])
    sites = []
    for g in groups:
        a, b = g[0], g[-1]
        while a > 0 and not ops[a].startswith("s_and_saveexec"):
            a -= 1
        while b + 1 < len(ops) and ops[b] != "s_or_b64":
            b += 1
        sites.append((a, b))
    for k, (a, b) in enumerate(sites):
        print("back-pointer store %d   %s" % (k, fmt(count(ops[a:b + 1]))))
    if not sites:
        print("back-pointer store     none in the forward loop")
    e0 = back_to_branch(win)
    e1 = next(n for n in range(win, len(ops)) if ops[n] == "s_branch")
    seg = ops[e0:e1 + 1]
    c = count(seg)
    # (The word store's block may be laid out behind the stretch's closing branch.)
    print("group epilogue         %s  (v_mov %d; ds_write_b32 in it or in the 60 instructions behind it: %d)" % (
        fmt(c), sum(o.startswith("v_mov") for o in seg), sum(o == "ds_write_b32" for o in ops[e0:e1 + 61])))
    moves = [n for n in range(roots[-1], win) if is_reg_move(ops[n], args[n])]
    clusters = []
    for n in moves:
        if clusters and n - clusters[-1][-1] <= 8:
            clusters[-1].append(n)
        else:
            clusters.append([n])
    # (A lone copy that widens an offset for a 64-bit compare is no shift.)
    shift = next((c for c in reversed(clusters) if len(c) >= 3), [])
    g0 = back_to_branch(shift[0]) if shift else e0
    last_store = max([n for n in range(g0, win) if ops[n] in ("ds_write_b32", "buffer_store_byte")], default=e0 - 1)
    w0 = max(e0, last_store + 1)
    adv = [n for n in range(w0, e1 + 1) if ops[n].startswith("v_") and n not in shift and not is_reg_move(ops[n], args[n])]
    rest = [n for n in range(g0, e1 + 1) if ops[n].startswith("v_") and n not in shift and n not in adv]
    print("  ring shift           v_ %3d  (v_mov_b32 %d, v_mov_b64 %d, v_pk_mov_b32 %d)" % (
        len(shift), sum(ops[n].startswith("v_mov_b32") for n in shift), sum(ops[n].startswith("v_mov_b64") for n in shift),
        sum(ops[n].startswith("v_pk_mov") for n in shift)))
    print("  window advance       v_ %3d  (loads: %s)" % (
        len(adv), ", ".join(sorted({ops[n] for n in range(w0, e1 + 1) if "_load_" in ops[n]})) or "laid out behind"))
    print("  the rest             v_ %3d  (from the branch before the shift, %d instructions before the splice)" % (
        len(rest), win - g0))


def main():
    argv = [x for x in sys.argv[1:] if x != "--prologue"]
    path = argv[0]
    sub = argv[1] if len(argv) > 1 else DEFAULT
    body = kernel_body(open(path).read().split("\n"), sub)
    ops, args = [], []
    for ln in body:
        m = re.match(r"\s+([a-z_0-9]+)(.*)", ln)
        if m and not ln.lstrip().startswith((".", ";")):
            ops.append(m.group(1))
            args.append(m.group(2).split(";")[0].strip())
    if "--prologue" in sys.argv[1:]:
        prologue(ops, sub, args)
        return
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
