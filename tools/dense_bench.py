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
L = 2048 (ids, seq, pos, stats); fit (spm_hip_fit_ids, all outputs) of c2 at
L = 16 and L = 2048 and of botchan and wagahaiwa at L = 512, timed in pairs
with spm_hip_pack_ids on the same ids (--fit-only skips the rest); window
(spm_hip_window_ids, all outputs) of c2 at L = 16, S = 4, of botchan at
L = 64, S = 16 and of wagahaiwa at L = 128, S = 32, likewise beside pack
(--window-only skips the rest).  Per workload, in one run:

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
    ap.add_argument("--fit-only", action="store_true")
    ap.add_argument("--window-only", action="store_true")
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
    lines = ["python tools/dense_bench.py " + " ".join(sys.argv[1:])]

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

    def fit(name, d_ids, d_off, L, pad_id=-1):
        """spm_hip_fit_ids beside spm_hip_pack_ids on the same ids, and the one-thread host loop once."""
        import time
        n = d_off.numel() - 1
        T = int((d_off[-1] - d_off[0]).item())
        cap = spm_amd.fit_rows_bound(T, n, L)
        prow = (T + L - 1) // L
        out, seq, pos = (torch.empty((cap, L), dtype=torch.int32, device=dev) for _ in range(3))
        rl = torch.empty(cap, dtype=torch.int32, device=dev)
        place = torch.empty(n, dtype=torch.int64, device=dev)
        stats = torch.empty(4, dtype=torch.int64, device=dev)
        nbytes = spm_amd.fit_ids_scratch_bytes(n, L, cap)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)

        def kernel():
            spm_amd.fit_ids_device(d_ids.data_ptr(), d_off.data_ptr(), n, L, pad_id, 0, cap, out.data_ptr(),
                                   scratch.data_ptr(), nbytes, seq.data_ptr(), pos.data_ptr(), rl.data_ptr(),
                                   place.data_ptr(), stats.data_ptr(), stream=stream)

        def packed():
            spm_amd.pack_ids_device(d_ids.data_ptr(), d_off.data_ptr(), n, L, pad_id, prow, out.data_ptr(),
                                    seq.data_ptr(), pos.data_ptr(), stream=stream)

        times, _, _ = pairs(packed, kernel)
        kernel()
        torch.cuda.synchronize(dev)
        R, kept = int(stats[0].item()), int(stats[1].item())
        t0 = time.perf_counter()
        h = spm_amd.fit_ids_host(d_ids.cpu().numpy(), d_off.cpu().numpy().view(np.uint64), L, pad_id, 0,
                                 rows_capacity=R)
        host_ms = (time.perf_counter() - t0) * 1e3
        same = all(np.array_equal(a[:R].cpu().numpy(), b) for a, b in zip((out, seq, pos, rl), h[:4]))
        same = same and np.array_equal(place.cpu().numpy().view(np.uint64), h[4]) and stats.tolist() == h[5].tolist()
        moved = 8 * (n + 1) + 4 * kept + 3 * 4 * R * L + 4 * R + 8 * n + 32
        lines.append("%s: fit, %d sentences, %d ids, L = %d, %d rows (pack: %d), %d bytes of scratch; pack on the same "
                     "ids median %.3f ms (min %.3f, max %.3f); fit / pack = %.2f; one-thread host loop (with its "
                     "buffers) %.1f ms; equal to the host loop: %s"
                     % (name, n, T, L, R, prow, nbytes, times[0][0], times[0][1], times[0][2],
                        times[1][0] / times[0][0], host_ms, same))
        src, dst = (torch.empty(moved, dtype=torch.uint8, device=dev) for _ in range(2))
        c = [timed(lambda: dst.copy_(src))[0] for _ in range(args.warmup + args.pairs)][args.warmup:]
        k = times[1]
        lines.append("%s  kernels (stream call, HIP events) median %.3f ms (min %.3f, max %.3f): %d bytes needed, "
                     "%.1f GB/s; device-to-device copy of that many bytes median %.3f ms"
                     % (name, k[0], k[1], k[2], moved, moved / (k[0] * 1e-3) / 1e9, statistics.median(c)))

    def window(name, d_ids, d_off, L, S, pad_id=-1):
        """spm_hip_window_ids (all outputs, no kept tokens) beside spm_hip_pack_ids at the same L on the same
        ids, a device copy of the bytes it writes, and the one-thread host loop once."""
        import time
        n = d_off.numel() - 1
        T = int((d_off[-1] - d_off[0]).item())
        cap = spm_amd.window_rows_bound(T, n, L, S)
        prow = (T + L - 1) // L
        out, pos, seq = (torch.empty((max(cap, prow), L), dtype=torch.int32, device=dev) for _ in range(3))
        fresh = torch.empty((cap, L), dtype=torch.uint8, device=dev)
        lengths, rs = (torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(2))
        first_row = torch.empty(n + 1, dtype=torch.int64, device=dev)
        stats = torch.empty(2, dtype=torch.int64, device=dev)
        nbytes = spm_amd.window_ids_scratch_bytes(n)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)

        def kernel():
            spm_amd.window_ids_device(d_ids.data_ptr(), d_off.data_ptr(), n, L, S, pad_id, 0, cap, out.data_ptr(),
                                      scratch.data_ptr(), nbytes, pos.data_ptr(), fresh.data_ptr(),
                                      lengths.data_ptr(), rs.data_ptr(), first_row.data_ptr(), stats.data_ptr(),
                                      stream=stream)

        def packed():
            spm_amd.pack_ids_device(d_ids.data_ptr(), d_off.data_ptr(), n, L, pad_id, prow, out.data_ptr(),
                                    seq.data_ptr(), pos.data_ptr(), stream=stream)

        times, _, _ = pairs(packed, kernel)
        kernel()
        torch.cuda.synchronize(dev)
        R, multi = stats.tolist()
        t0 = time.perf_counter()
        h = spm_amd.window_ids_host(d_ids.cpu().numpy(), d_off.cpu().numpy().view(np.uint64), L, S, pad_id, 0,
                                    rows_capacity=R)
        host_ms = (time.perf_counter() - t0) * 1e3
        same = all(np.array_equal(a[:R].cpu().numpy(), b) for a, b in zip((out, pos, fresh, lengths, rs), h[:5]))
        same = same and np.array_equal(first_row.cpu().numpy().view(np.uint64), h[5]) and [R, multi] == h[6].tolist()
        written = 9 * R * L + 8 * R + 8 * (n + 1) + 16
        src, dst = (torch.empty(written, dtype=torch.uint8, device=dev) for _ in range(2))
        c = [timed(lambda: dst.copy_(src))[0] for _ in range(args.warmup + args.pairs)][args.warmup:]
        cm, (p, k) = statistics.median(c), times
        lines.append("%s: window, %d sentences, %d ids, L = %d, S = %d, %d rows (bound %d; pack: %d), %d sentences of "
                     "several rows, %d bytes of scratch; equal to the host loop: %s"
                     % (name, n, T, L, S, R, cap, prow, multi, nbytes, same))
        lines.append("%s  kernels (stream call, HIP events) median %.3f ms (min %.3f, max %.3f): %d bytes written, "
                     "%.1f GB/s; device-to-device copy of that many bytes median %.3f ms (min %.3f, max %.3f); "
                     "window / copy = %.2f" % (name, k[0], k[1], k[2], written, written / (k[0] * 1e-3) / 1e9, cm,
                                               min(c), max(c), k[0] / cm))
        lines.append("%s  pack at the same L on the same ids median %.3f ms (min %.3f, max %.3f); window / pack = "
                     "%.2f; one-thread host loop (with its buffers) %.1f ms"
                     % (name, p[0], p[1], p[2], k[0] / p[0], host_ms))

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
    only = args.fit_only or args.window_only
    if not only:
        pad("c2 L=16", c2_ids, c2_off, 16)
        pack("c2 L=2048", c2_ids, c2_off, 2048)
    if not args.window_only:
        fit("c2 L=16", c2_ids, c2_off, 16)
        fit("c2 L=2048", c2_ids, c2_off, 2048)
    if not args.fit_only:
        window("c2 L=16 S=4", c2_ids, c2_off, 16, 4)
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
        for L in () if only else (64, 512):
            pad("%s x%d L=%d" % (name, reps, L), d_ids, d_off, L)
        if name == "botchan" and not only:
            pack("%s x%d L=2048" % (name, reps), d_ids, d_off, 2048)
        if not args.window_only:
            fit("%s x%d L=512" % (name, reps), d_ids, d_off, 512)
        if not args.fit_only:
            L = 64 if name == "botchan" else 128
            window("%s x%d L=%d S=%d" % (name, reps, L, L // 4), d_ids, d_off, L, L // 4)
        del d_ids, d_off
        torch.cuda.empty_cache()

    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
