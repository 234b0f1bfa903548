#!/usr/bin/env python3
"""Throughput of the device n-best search on bench.py's c2 workload (synthetic
sentences of tools/synth.py seed 1234, the 32k unigram model) at several
nbest sizes: per size, the HIP-event time of the two search kernel launches,
the wall time of the whole blocking call (search, scans, gather), sentences/s,
paths and tokens returned, and the share of sentences the second device tier
and the host took.  For scale, in the same run: the plain encode's fast
kernel on the same resident batch, and the single-thread rate of the host
implementation (csrc/host_nbest.h through `nbest_selftest host`) on a slice.

  python tools/nbest_bench.py [--sentences N] [--sizes 2,5,16,64] [--out FILE]
"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sentencepiece-comments_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, default=1_000_000)
    ap.add_argument("--sizes", default="2,5,16,64")
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-slice", type=int, default=10_000)
    ap.add_argument("--model", default=os.path.join(ROOT, "data", "synth32k_unigram.model"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import spm_amd
    import synth
    dev = torch.device("cuda", 0)
    dm = spm_amd.DeviceModel(open(args.model, "rb").read())
    dm.set_timing(True)
    buf, off = synth.normalized(args.sentences, seed=1234)
    n, total = len(off) - 1, int(off[-1])
    d_bytes = torch.from_numpy(buf).to(dev)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    d_po = torch.empty(n + 1, dtype=torch.int64, device=dev)
    lines = ["c2 workload: %d sentences, %d bytes, longest %d bytes, model %s, %d calls after %d warm-up"
             % (n, total, int(np.diff(off.view(np.int64)).max()), os.path.basename(args.model), args.launches,
                args.warmup)]
    d_ids = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    d_tok = torch.empty(n + 1, dtype=torch.int64, device=dev)
    ms = []
    for k in range(args.warmup + 5):
        dm.encode_device(d_bytes.data_ptr(), d_off.data_ptr(), n, d_ids.data_ptr(), d_tok.data_ptr())
        if k >= args.warmup:
            ms.append(float(dm.stats().fast_kernel_ms))
    lines.append("encode      fast kernel median %.3f ms, %.3e sentences/s" % (statistics.median(ms), n / (statistics.median(ms) * 1e-3)))
    del d_ids, d_tok
    slice_n = min(args.host_slice, n)
    with tempfile.NamedTemporaryFile(suffix=".txt") as f:
        f.write(b"".join(buf[int(off[i]):int(off[i + 1])].tobytes() + b"\n" for i in range(slice_n)))
        f.flush()
        selftest = os.path.join(ROOT, "sentencepiece-comments_amd", "lib", "nbest_selftest")
        host = {}
        for N in [int(x) for x in args.sizes.split(",")]:
            with open(f.name, "rb") as fin:
                p = subprocess.run([selftest, "host", args.model, str(N)], stdin=fin, stdout=subprocess.DEVNULL,
                                   stderr=subprocess.PIPE, check=True)
            m = re.search(r"host_nbest: (\d+) lines in ([0-9.]+) s", p.stderr.decode())
            host[N] = int(m.group(1)) / float(m.group(2))
    for N in [int(x) for x in args.sizes.split(",")]:
        # A first call with small capacities returns the totals; the buffers are sized by them.
        try:
            P, T = dm.nbest_encode_device(d_bytes.data_ptr(), d_off.data_ptr(), n, N, 0, 0, d_po.data_ptr(), 0, 0,
                                          d_po.data_ptr())
        except spm_amd.SpmError as e:
            if e.code != 8:
                raise
            P, T = e.totals
        d_ids = torch.empty(max(T, 1), dtype=torch.int32, device=dev)
        d_tok = torch.empty(P + 1, dtype=torch.int64, device=dev)
        d_sc = torch.empty(max(P, 1), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        kern, wall = [], []
        for k in range(args.warmup + args.launches):
            t0 = time.perf_counter()
            dm.nbest_encode_device(d_bytes.data_ptr(), d_off.data_ptr(), n, N, d_ids.data_ptr(), T, d_tok.data_ptr(),
                                   d_sc.data_ptr(), P, d_po.data_ptr())
            dt = (time.perf_counter() - t0) * 1e3
            if k >= args.warmup:
                wall.append(dt)
                kern.append(float(dm.stats().general_kernel_ms))
        second, hostn = dm.nbest_stats()
        km, wm = statistics.median(kern), statistics.median(wall)
        lines.append("nbest N=%-3d search kernels median %.1f ms (min %.1f, max %.1f), call %.1f ms, %.3e sentences/s "
                     "per call, %d paths, %d tokens, second tier %d (%.4f %%), host %d (%.4f %%); host_nbest.h alone, "
                     "one thread, %d sentences: %.3e sentences/s"
                     % (N, km, min(kern), max(kern), wm, n / (wm * 1e-3), P, T, second, 100.0 * second / n, hostn,
                        100.0 * hostn / n, slice_n, host[N]))
        del d_ids, d_tok, d_sc
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
