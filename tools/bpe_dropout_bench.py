#!/usr/bin/env python3
"""Device time of BPE-dropout next to the plain BPE encode, over a resident
batch: the timed span of spm_hip_encode_batch and of
spm_hip_bpe_dropout_encode_batch (first kernels, the general kernels over
what they flag, scan and compaction; HIP events), after warm-up, a number of
launches each; median and spread, sentences/s, and the share of sentences the
general tier took.

Workloads: c3 (bench.py's BPE leg: synthetic sentences of tools/synth.py seed
1234, the 32k BPE model) and botchan (the normalized lines of
tests/golden/botchan.txt under botchan_bpe1k.model, repeated to --sentences).

The kernels' A/B knobs are read once per process, so one process measures one
configuration: SPM_HIP_BPE_DROPOUT_SHORT=0 turns the short-slab pass off,
SPM_HIP_BPE_FAST_ONLY=1 runs bpe_fast_kernel alone for the plain encode (one
sentence per wave, the like-for-like yardstick).  --package DIR imports
spm_amd from another build (a parent commit's); --no-dropout measures the
plain encode only (a build without the entry).

  python tools/bpe_dropout_bench.py --workload c3|botchan [--sentences N] [--launches K] [--label TEXT] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("c3", "botchan"), default="c3")
    ap.add_argument("--sentences", type=int, default=None, help="default: 10 M (c3), 1 M (botchan)")
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--alphas", default="0,0.1,0.5")
    ap.add_argument("--package", default=os.path.join(ROOT, "sentencepiece-comments_amd"))
    ap.add_argument("--no-dropout", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None, help="append the report to this file")
    args = ap.parse_args()
    sys.path.insert(0, args.package)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import numpy as np
    import torch
    import spm_amd
    dev = torch.device("cuda", 0)
    if args.workload == "c3":
        import synth
        model = os.path.join(ROOT, "data", "synth32k_bpe.model")
        dm = spm_amd.DeviceModel(open(model, "rb").read())
        buf, off = synth.normalized(args.sentences or 10_000_000, seed=1234)
    else:
        model = os.path.join(ROOT, "tests", "golden", "botchan_bpe1k.model")
        dm = spm_amd.DeviceModel(open(model, "rb").read())
        with open(os.path.join(ROOT, "tests", "golden", "botchan.txt"), "rb") as f:
            lines = f.read().split(b"\n")[:-1]
        norm = dm.normalize(lines)
        want = args.sentences or 1_000_000
        norm = (norm * (want // len(norm) + 1))[:want]
        buf, off = spm_amd.to_csr(norm)
    dm.set_timing(True)
    n, total = len(off) - 1, int(off[-1])
    lens = np.diff(off.astype(np.int64))
    d_bytes = torch.from_numpy(buf).to(dev)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    d_ids = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    d_tok = torch.empty(n + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)

    def plain(_):
        dm.encode_device(d_bytes.data_ptr(), d_off.data_ptr(), n, d_ids.data_ptr(), d_tok.data_ptr())

    def dropout(alpha):
        def fn(k):
            dm.bpe_dropout_encode_device(d_bytes.data_ptr(), d_off.data_ptr(), n, alpha, 1234, d_ids.data_ptr(),
                                         d_tok.data_ptr(), index_base=k * n)
        return fn

    runs = [("encode", plain)]
    if not args.no_dropout:
        runs += [("dropout alpha %s" % a, dropout(float(a))) for a in args.alphas.split(",")]
    knobs = " ".join("%s=%s" % (k, os.environ[k]) for k in ("SPM_HIP_BPE_DROPOUT_SHORT", "SPM_HIP_BPE_FAST_ONLY")
                     if k in os.environ)
    out = ["%s%s: %d sentences, %d bytes (mean %.1f, max %d, over 128 bytes: %.2f %%), model %s, %d launches after "
           "%d warm-up%s" % (args.label + ": " if args.label else "", args.workload, n, total, lens.mean(), lens.max(),
                             100.0 * float((lens > 128).mean()), os.path.basename(model), args.launches, args.warmup,
                             ", " + knobs if knobs else "")]
    base = None
    for name, fn in runs:
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
        base = base or med
        out.append("  %-18s median %9.3f ms (min %9.3f, max %9.3f)  %.3e sentences/s  x%.2f of encode  tokens %d  "
                   "general tier %d of %d (%.4f %%)" % (name, med, min(ms), max(ms), n / (med * 1e-3), med / base,
                                                        tokens, general, n, 100.0 * general / n))
    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
