#!/usr/bin/env python3
"""Time of the lattice-score calls next to the sampler, on bench.py's c2
workload (10 M synthetic sentences of tools/synth.py seed 1234, the 32k
unigram model, alpha 0.5), all on one resident batch and one build:

  spm_hip_sample_encode_batch                      (the yardstick)
  spm_hip_entropy_batch
  spm_hip_sample_encode_and_score_batch at num_samples 1, 4 and 16

For each: the HIP-event time of the fast-tier launch (its memsets included;
spm_hip_model_last_stats with timing on) and the host-clock time of the whole
blocking call (it ends in a device synchronise; scan, gather and the small
read-backs included), over 20 launches after warm-up: median, min and max,
and the sentences the exact tier took.

  python tools/lattice_score_bench.py [--sentences N] [--launches K] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sentencepiece-comments_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, default=10_000_000)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--theta", type=float, default=0.5)
    ap.add_argument("--samples", default="1,4,16")
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
    samples = [int(x) for x in args.samples.split(",")]
    kmax = max(samples)
    d_bytes = torch.from_numpy(buf).to(dev)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    d_ids = torch.empty(max(total * kmax, 1), dtype=torch.int32, device=dev)
    d_tok = torch.empty(n * kmax + 1, dtype=torch.int64, device=dev)
    d_sc = torch.empty(n * kmax, dtype=torch.float32, device=dev)
    d_h = torch.empty(n, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)

    def sample(k):
        dm.sample_encode_device(d_bytes.data_ptr(), d_off.data_ptr(), n, args.theta, 1234, d_ids.data_ptr(),
                                d_tok.data_ptr(), index_base=k * n)

    def entropy(_):
        dm.entropy_device(d_bytes.data_ptr(), d_off.data_ptr(), n, args.theta, d_h.data_ptr())

    def score(ns):
        def fn(k):
            dm.sample_encode_and_score_device(d_bytes.data_ptr(), d_off.data_ptr(), n, ns, args.theta, 1234,
                                              d_ids.data_ptr(), total * ns, d_tok.data_ptr(), d_sc.data_ptr(),
                                              index_base=k * n)
        return fn

    cases = [("sample_encode", sample), ("entropy", entropy)] + [("sample_and_score k=%d" % k, score(k)) for k in samples]
    rows = {}
    for name, fn in cases:
        for k in range(args.warmup):
            fn(k)
        kern, call, general = [], [], 0
        for k in range(args.launches):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn(args.warmup + k)
            call.append((time.perf_counter() - t0) * 1e3)
            st = dm.stats()
            kern.append(float(st.fast_kernel_ms))
            general = int(st.general_path)
        rows[name] = (kern, call, general)
    lines = ["c2 workload: %d sentences, %d bytes, model %s, theta %.2f, %d launches after %d warm-up"
             % (n, total, os.path.basename(args.model), args.theta, args.launches, args.warmup)]
    for name, (kern, call, general) in rows.items():
        lines.append("%-22s fast tier median %.3f ms (min %.3f, max %.3f); whole call median %.3f ms (min %.3f, "
                     "max %.3f); exact tier %d of %d sentences"
                     % (name, statistics.median(kern), min(kern), max(kern), statistics.median(call), min(call),
                        max(call), general, n))
    base_k, base_c = statistics.median(rows["sample_encode"][0]), statistics.median(rows["sample_encode"][1])
    for name, (kern, call, _) in rows.items():
        if name != "sample_encode":
            lines.append("ratio %s / sample_encode: fast tier %.2f, whole call %.2f"
                         % (name, statistics.median(kern) / base_k, statistics.median(call) / base_c))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
