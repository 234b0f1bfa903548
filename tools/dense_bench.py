#!/usr/bin/env python3
"""Speed of the dense id batches (spm_hip_pad_ids / spm_hip_pack_ids) on a
final id CSR resident in HBM.

Id batches, each encoded on the device first:
  c2        bench.py's c2 workload (synthetic sentences of tools/synth.py seed
            1234, the 32k unigram model), 4.4 tokens per sentence
  botchan   tests/golden/botchan.txt under test_model.model with "bos:eos",
            its id CSR repeated to --lines lines
  wagahaiwa tests/golden/wagahaiwa_nekodearu.txt under test_ja_model.model,
            likewise
Workloads: pad of c2 at L = 16, pad of botchan and wagahaiwa at L = 64 and
L = 512 (all outputs: ids, lengths, mask, stats), pack of c2 and botchan at
L = 2048 (ids, seq, pos, stats).  Per workload, in one run:

  * the kernel's time (HIP events around the stream call) and a restatement of
    the same result with torch ops on the same CSR on the device, warmed up and
    then timed alternately, one pair after the other; per side the median, and
    the spread (min, max) of these repeated identical runs next to the
    difference;
  * the bytes the operation needs (offsets and kept ids in; ids, lengths / seq,
    mask / pos out) and that over the kernel's time;
  * a device-to-device copy of a buffer of that size (it reads and writes it,
    so it moves twice that), and the share of the copy's bandwidth the kernel
    reaches;
  * whether the torch restatement's tensors equal the kernel's.

  python tools/dense_bench.py [--sentences N] [--lines N] [--pairs K] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sentencepiece-comments_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, default=10_000_000)
    ap.add_argument("--lines", type=int, default=500_000)
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import oracle_lib
    import spm_amd
    import synth
    if not torch.cuda.is_available():
        sys.exit("dense_bench: no GPU; nothing measured")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    lines = []

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1), out

    def pairs(a, b):
        """Warm up, then a and b alternately; per side (median, min, max) ms and the last result."""
        ta, tb, ra, rb = [], [], None, None
        for k in range(args.warmup + args.pairs):
            x, ra = timed(a)
            y, rb = timed(b)
            if k >= args.warmup:
                ta.append(x)
                tb.append(y)
        return [(statistics.median(t), min(t), max(t)) for t in (ta, tb)], ra, rb

    def report(name, moved, times, same):
        (k, t) = times
        src = torch.empty(moved, dtype=torch.uint8, device=dev)
        dst = torch.empty(moved, dtype=torch.uint8, device=dev)
        c = []
        for r in range(args.warmup + args.pairs):
            ms, _ = timed(lambda: dst.copy_(src))
            if r >= args.warmup:
                c.append(ms)
        cm = statistics.median(c)
        kernel_bw, copy_bw = moved / (k[0] * 1e-3) / 1e9, 2 * moved / (cm * 1e-3) / 1e9
        lines.append("%s  kernel (stream call, HIP events) median %.3f ms (min %.3f, max %.3f): %d bytes needed, "
                     "%.1f GB/s" % (name, k[0], k[1], k[2], moved, kernel_bw))
        lines.append("%s  device-to-device copy of %d bytes median %.3f ms (min %.3f, max %.3f): %.1f GB/s read + "
                     "written; the kernel reaches %.2f of the copy's bandwidth"
                     % (name, moved, cm, min(c), max(c), copy_bw, kernel_bw / copy_bw))
        lines.append("%s  torch restatement median %.3f ms (min %.3f, max %.3f); equal tensors: %s; restatement - "
                     "kernel = %.3f ms (%.1f x), spread of identical runs: kernel %.3f ms, restatement %.3f ms"
                     % (name, t[0], t[1], t[2], same, t[0] - k[0], t[0] / k[0], k[2] - k[1], t[2] - t[1]))

    def pad(name, d_ids, d_off, L, pad_id=-1):
        n = d_off.numel() - 1
        out = torch.empty((n, L), dtype=torch.int32, device=dev)
        lengths = torch.empty(n, dtype=torch.int32, device=dev)
        mask = torch.empty((n, L), dtype=torch.uint8, device=dev)
        stats = torch.empty(2, dtype=torch.int64, device=dev)

        def kernel():
            spm_amd.pad_ids_device(d_ids.data_ptr(), d_off.data_ptr(), n, L, pad_id, 0, out.data_ptr(),
                                   lengths.data_ptr(), mask.data_ptr(), stats.data_ptr(), stream=stream)

        def restated():
            lens = d_off[1:] - d_off[:-1]
            k = lens.clamp(max=L)
            cols = torch.arange(L, device=dev)
            m = cols[None, :] < k[:, None]
            src = (d_off[:-1, None] + cols[None, :]).clamp(max=d_ids.numel() - 1)
            o = torch.where(m, d_ids[src], torch.tensor(pad_id, dtype=torch.int32, device=dev))
            cut = lens > L
            return o, k.to(torch.int32), m.to(torch.uint8), torch.stack([cut.sum(), (lens - k).sum()])

        times, _, r = pairs(kernel, restated)
        same = all(bool(torch.equal(a, b)) for a, b in zip((out, lengths, mask, stats), r))
        kept = int(r[1].sum().item())
        moved = 8 * (n + 1) + 4 * kept + 4 * n * L + 4 * n + n * L + 16
        lines.append("%s: pad, %d sentences, L = %d, %d ids of %d kept, %d cut"
                     % (name, n, L, kept, int((d_off[-1] - d_off[0]).item()), int(stats[0].item())))
        del r
        report(name, moved, times, same)

    def pack(name, d_ids, d_off, L, pad_id=-1):
        n = d_off.numel() - 1
        T = int((d_off[-1] - d_off[0]).item())
        rows = (T + L - 1) // L
        out, seq, pos = (torch.empty((rows, L), dtype=torch.int32, device=dev) for _ in range(3))
        stats = torch.empty(2, dtype=torch.int64, device=dev)

        def kernel():
            spm_amd.pack_ids_device(d_ids.data_ptr(), d_off.data_ptr(), n, L, pad_id, rows, out.data_ptr(),
                                    seq.data_ptr(), pos.data_ptr(), stats.data_ptr(), stream=stream)

        def restated():
            base = d_off[0]
            t = torch.arange(rows * L, device=dev)
            valid = t < T
            ends = d_off[1:] - base
            s = torch.searchsorted(ends, t, right=True).clamp(max=n - 1)
            p = t - (d_off[s] - base)
            o = torch.where(valid, d_ids[(base + t).clamp(max=d_ids.numel() - 1)],
                            torch.tensor(pad_id, dtype=torch.int32, device=dev))
            s = torch.where(valid, s, -1).to(torch.int32)
            p = torch.where(valid, p, 0).to(torch.int32)
            return o.view(rows, L), s.view(rows, L), p.view(rows, L)

        times, _, r = pairs(kernel, restated)
        same = all(bool(torch.equal(a, b)) for a, b in zip((out, seq, pos), r))
        same = same and stats.tolist() == [rows, T]
        del r
        moved = 8 * (n + 1) + 4 * T + 3 * 4 * rows * L + 16
        lines.append("%s: pack, %d sentences, %d ids, L = %d, %d rows" % (name, n, T, L, rows))
        report(name, moved, times, same)

    # c2: the synthetic batch, encoded on the device (model-level ids are final ids here: no extra options).
    buf, off = synth.normalized(args.sentences, seed=1234)
    dm = spm_amd.DeviceModel(open(os.path.join(ROOT, "data", "synth32k_unigram.model"), "rb").read())
    n = len(off) - 1
    d_bytes = torch.from_numpy(buf).to(dev)
    d_boff = torch.from_numpy(off.view(np.int64)).to(dev)
    c2_ids = torch.empty(max(int(off[-1]), 1), dtype=torch.int32, device=dev)
    c2_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    dm.encode_device(d_bytes.data_ptr(), d_boff.data_ptr(), n, c2_ids.data_ptr(), c2_off.data_ptr())
    torch.cuda.synchronize(dev)
    c2_ids = c2_ids[:int(c2_off[-1].item())].clone()
    del d_bytes, d_boff, dm
    pad("c2 L=16", c2_ids, c2_off, 16)
    pack("c2 L=2048", c2_ids, c2_off, 2048)
    del c2_ids, c2_off

    gold = os.path.join(ROOT, "tests", "golden")
    for name, model, text in (("botchan", "test_model.model", "botchan.txt"),
                              ("wagahaiwa", "test_ja_model.model", "wagahaiwa_nekodearu.txt")):
        raw = oracle_lib.read_lines_binary(os.path.join(gold, text))
        dm = spm_amd.DeviceModel(open(os.path.join(gold, model), "rb").read())
        d_fin, d_foff, k = dm._lines_to_id_csr(raw, "bos:eos")
        torch.cuda.synchronize(dev)
        reps = (args.lines + len(raw) - 1) // len(raw)
        foff = d_foff.cpu().numpy()
        toff = np.zeros(reps * len(raw) + 1, dtype=np.int64)
        toff[1:] = np.cumsum(np.tile(foff[1:] - foff[:-1], reps))
        d_ids = d_fin[:k].repeat(reps)
        d_off = torch.from_numpy(toff).to(dev)
        del dm, d_fin, d_foff
        for L in (64, 512):
            pad("%s x%d L=%d" % (name, reps, L), d_ids, d_off, L)
        if name == "botchan":
            pack("%s x%d L=2048" % (name, reps), d_ids, d_off, 2048)
        del d_ids, d_off
        torch.cuda.empty_cache()

    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
