#!/usr/bin/env python3
"""Compare the shipped estep_backward_kernel instantiations of two assembly files.

  compare_backward_asm.py BEFORE.s AFTER.s

Both files are estep_kernels.hip compiled device-only to AMDGPU assembly with
the Makefile's flags:

  hipcc $(HIPFLAGS) -S --cuda-device-only csrc/estep_kernels.hip -o X.s

For each shipped instantiation the text from the function's label to its
.Lfunc_end<n> label (itself left out: <n> is the function index again) is
taken, comments (';' to end of line) are stripped and the
function index in local labels (.LBB<n>_) is removed.  Exit status 0 if the
five bodies are equal, 1 otherwise (a unified diff of the first differing
lines is printed).
"""
import difflib
import re
import sys

SHIPPED = [(16, 4, 42), (16, 4, 10), (16, 3, 40), (16, 3, 8), (32, 1, 0)]


def is_label(line):
    return line.startswith("_Z") and line.split(";", 1)[0].rstrip().endswith(":")


def body(lines, w, wpe, var):
    want = f"estep_backward_kernelILi{w}ELi{wpe}ELi{var}EE"
    start = [i for i, l in enumerate(lines) if is_label(l) and want in l]
    if len(start) != 1:
        return None
    out = []
    for l in lines[start[0]:]:
        l = re.sub(r"\.LBB\d+_", ".LBB_", l.split(";", 1)[0]).rstrip()
        if l.startswith(".Lfunc_end"):
            return out
        if l:
            out.append(l)
    return None


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    before, after = (open(p).read().split("\n") for p in sys.argv[1:])
    for name, lines in (("before", before), ("after", after)):
        n = sum(1 for l in lines if is_label(l) and "estep_backward_kernelILi" in l)
        print(f"{name}: {n} estep_backward_kernel instantiations")
    bad = 0
    for w, wpe, var in SHIPPED:
        a, b = body(before, w, wpe, var), body(after, w, wpe, var)
        tag = f"estep_backward_kernel<{w}, {wpe}, {var}>"
        if a is None or b is None:
            print(f"{tag}: MISSING ({'before' if a is None else 'after'})")
            bad += 1
        elif a == b:
            print(f"{tag}: identical ({len(a)} lines)")
        else:
            print(f"{tag}: DIFFERENT")
            d = list(difflib.unified_diff(a, b, "before", "after", lineterm="", n=2))
            print("\n".join(d[:60]))
            bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
