#!/usr/bin/env python3
"""Device time of the plain BPE encode over real text, next to BPE-dropout at
alpha 0 (the same ids through bpe_dropout_kernel), over a resident batch: the
timed span of spm_hip_encode_batch (first kernels, the word and wave tiers and
the literal kernel over what they flag, scan and compaction; HIP events),
after warm-up, a number of launches each; median and spread, sentences/s, and
the flagged sentences by the tier that finished them.

Workloads: c3 (bench.py's BPE leg: synthetic sentences of tools/synth.py seed
1234, the 32k BPE model), botchan (the normalized lines of botchan.txt under
botchan_bpe1k.model), wagahaiwa (the normalized lines of
wagahaiwa_nekodearu.txt under botchan_bf_bpe1k.model: giant words) and docs
(botchan lines joined to documents of about 8 KB) and frozen (the botchan
lines with "<tag>" / "<mask>" spliced in after every seventh space, under
botchan_bpe1k's pieces plus those two as USER_DEFINED pieces: the
frozen-symbol tier; --symbols-normal makes them NORMAL pieces, the text tiers'
yardstick for it); the corpora are repeated to --sentences.  A call that ran
host-sized (the literal kernel over every sentence) has no fast span: its
general-kernel span is reported.

The kernels' A/B knobs are read once per process, so one process measures one
configuration: SPM_HIP_BPE_TEXT=0 hands every flagged sentence to the literal
kernel, SPM_HIP_BPE_TEXT=2 runs the wave tier without the word tier,
SPM_HIP_BPE_FROZEN=0 restores the host-sized pass of user-defined models.
--package DIR imports spm_amd from another build (a parent commit's).

  python tools/bpe_text_bench.py --workload c3|botchan|wagahaiwa|docs|frozen [--sentences N] [--launches K] [--label TEXT] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DEFAULT_N = {"c3": 10_000_000, "botchan": 1_000_000, "wagahaiwa": 100_000, "docs": 20_000, "frozen": 1_000_000}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=tuple(DEFAULT_N), default="botchan")
    ap.add_argument("--sentences", type=int, default=None)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--package", default=os.path.join(ROOT, "sentencepiece-comments_amd"))
    ap.add_argument("--no-dropout", action="store_true")
    ap.add_argument("--symbols-normal", action="store_true", help="frozen: the two symbols as NORMAL pieces")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None, help="append the report to this file")
    args = ap.parse_args()
    sys.path.insert(0, args.package)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import spm_amd
    dev = torch.device("cuda", 0)
    want = args.sentences or DEFAULT_N[args.workload]
    if args.workload == "c3":
        import synth
        model = os.path.join(ROOT, "data", "synth32k_bpe.model")
        dm = spm_amd.DeviceModel(open(model, "rb").read())
        buf, off = synth.normalized(want, seed=1234)
    else:
        model = os.path.join(GOLD, "botchan_bf_bpe1k.model" if args.workload == "wagahaiwa" else "botchan_bpe1k.model")
        blob = open(model, "rb").read()
        if args.workload == "frozen":
            import model_builder as mb
            import model_reader
            kind = mb.NORMAL if args.symbols_normal else mb.USER_DEFINED
            pieces = model_reader.read_pieces(blob) + [("<tag>", -2000.0, kind), ("<mask>", -2001.0, kind)]
            blob = mb.model(pieces, mb.BPE, charsmap=model_reader.charsmap(blob))
            args.no_dropout = True  # (dropout of a user-defined model is the literal kernel over every sentence)
        dm = spm_amd.DeviceModel(blob)
        corpus = "wagahaiwa_nekodearu.txt" if args.workload == "wagahaiwa" else "botchan.txt"
        with open(os.path.join(GOLD, corpus), "rb") as f:
            norm = dm.normalize(f.read().split(b"\n")[:-1])
        if args.workload == "docs":  # consecutive lines joined up to about 8 KB
            docs, cur = [], b""
            for s in norm:
                cur += s
                if len(cur) >= 8192:
                    docs.append(cur)
                    cur = b""
            norm = docs
        if args.workload == "frozen":
            ws, spliced = "\u2581".encode(), []
            for line in norm:
                words = line.split(ws)
                for k in range(7, len(words), 7):
                    words[k] = (b"<mask>" if k % 2 else b"<tag>") + words[k]
                spliced.append(ws.join(words))
            norm = spliced
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

    def dropout0(k):
        dm.bpe_dropout_encode_device(d_bytes.data_ptr(), d_off.data_ptr(), n, 0.0, 1234, d_ids.data_ptr(),
                                     d_tok.data_ptr(), index_base=k * n)

    runs = [("encode", plain)] + ([] if args.no_dropout else [("dropout alpha 0", dropout0)])
    knobs = " ".join("%s=%s" % (k, os.environ[k]) for k in ("SPM_HIP_BPE_TEXT", "SPM_HIP_BPE_FROZEN") if k in os.environ)
    if args.symbols_normal:
        knobs = (knobs + " symbols NORMAL").strip()
    out = ["%s%s: %d sentences, %d bytes (mean %.1f, max %d, over 64 bytes: %.2f %%), model %s, %d launches after "
           "%d warm-up%s" % (args.label + ": " if args.label else "", args.workload, n, total, lens.mean(), lens.max(),
                             100.0 * float((lens > 64).mean()), os.path.basename(model), args.launches, args.warmup,
                             ", " + knobs if knobs else "")]
    first_ids = None
    for name, fn in runs:
        for k in range(args.warmup):
            fn(k)
        ms = []
        for k in range(args.launches):
            fn(args.warmup + k)
            ms.append(float(dm.stats().fast_kernel_ms) or float(dm.stats().general_kernel_ms))
        st = dm.stats()
        tokens = int(d_tok[-1].item())
        ids = d_ids[:tokens].clone()
        same = "" if first_ids is None else "  ids %s encode's" % ("=" if torch.equal(ids, first_ids) else "DIFFER FROM")
        first_ids = ids if first_ids is None else first_ids
        tiers = ""
        if name == "encode" and hasattr(dm, "bpe_tier_stats"):
            tiers = "  word / wave / literal tier %d / %d / %d" % dm.bpe_tier_stats()
        if name == "encode" and hasattr(dm, "bpe_frozen_stats"):
            tiers += "  frozen tier taken / handed on %d / %d" % dm.bpe_frozen_stats()
        med = statistics.median(ms)
        out.append("  %-16s median %9.3f ms (min %9.3f, max %9.3f)  %.3e sentences/s  tokens %d  flagged %d of %d%s%s"
                   % (name, med, min(ms), max(ms), n / (med * 1e-3), tokens, int(st.general_path), n, tiers, same))
    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
