#!/usr/bin/env python3
"""Kernel time of the unigram sampler next to the plain encode, on bench.py's
c2 workload (10 M synthetic sentences of tools/synth.py seed 1234, the 32k
unigram model): HIP-event time of the fast kernel of spm_hip_encode_batch and
of spm_hip_sample_encode_batch (theta 0.5; the sampler's figure includes the
memset of its node masks) over the same resident batch, after warm-up, 20
launches each; median and spread, their ratio, sentences/s and the share of
sentences the exact tier took.

  python tools/sample_bench.py [--sentences N] [--launches K] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sentencepiece-comments_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, default=10_000_000)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--theta", type=float, default=0.5)
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
    d_ids = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    d_tok = torch.empty(n + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)

    def plain(_):
        dm.encode_device(d_bytes.data_ptr(), d_off.data_ptr(), n, d_ids.data_ptr(), d_tok.data_ptr())

    def sample(k):
        dm.sample_encode_device(d_bytes.data_ptr(), d_off.data_ptr(), n, args.theta, 1234, d_ids.data_ptr(),
                                d_tok.data_ptr(), index_base=k * n)

    rows = {}
    for name, fn in (("encode", plain), ("sample_encode", sample)):
        for k in range(args.warmup):
            fn(k)
        ms, general, tokens = [], 0, 0
        for k in range(args.launches):
            fn(args.warmup + k)
            st = dm.stats()
            ms.append(float(st.fast_kernel_ms))
            general = int(st.general_path)
            tokens = int(d_tok[-1].item())
        med = statistics.median(ms)
        rows[name] = dict(median_ms=med, min_ms=min(ms), max_ms=max(ms), general_path=general, tokens=tokens,
                          sentences_per_s=n / (med * 1e-3))
    lines = ["c2 workload: %d sentences, %d bytes, model %s, theta %.2f, %d launches after %d warm-up"
             % (n, total, os.path.basename(args.model), args.theta, args.launches, args.warmup)]
    for name, r in rows.items():
        lines.append("%-14s fast kernel median %.3f ms (min %.3f, max %.3f), %.3e sentences/s, tokens %d, "
                     "exact/general tier %d of %d sentences (%.4f %%)"
                     % (name, r["median_ms"], r["min_ms"], r["max_ms"], r["sentences_per_s"], r["tokens"],
                        r["general_path"], n, 100.0 * r["general_path"] / n))
    lines.append("ratio sample_encode / encode: %.2f" % (rows["sample_encode"]["median_ms"] / rows["encode"]["median_ms"]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
