#!/usr/bin/env python3
"""Speed of the device decode (spm_hip_decode_batch) on ids resident in HBM.

Two batches are encoded on the device first: bench.py's c2 workload (synthetic
sentences of tools/synth.py seed 1234, the 32k unigram model) and its Japanese
leg (tests/golden/wagahaiwa_nekodearu.txt repeated to --ja-lines lines,
test_ja_model.model).  Per batch, in one run:

  * the blocking call spm_hip_decode_batch (host clock around it; it ends in
    a stream synchronization) and the kernels alone (HIP events around
    spm_hip_decode_batch_async): warm-up, then the median of --launches calls;
  * the bytes the call has to move (ids + offsets in, text + offsets out) and
    a device-to-device copy of a buffer of that size as the traffic bound
    (a copy reads and writes it, so it moves twice that);
  * the host loop (spm_hip_decode_batch_host on a host-only model, one
    thread) over the same ids: what a caller would otherwise run.

Then the crossover on the c2 ids: for growing batches, the host loop against
the host-buffer entry on the device model (upload, decode, download: what
SentencePieceProcessor::DecodeBatch does on its device path).  The first size
at which the device wins sets the processor's kDecodeDeviceMinTokens.

  python tools/decode_bench.py [--sentences N] [--ja-lines N] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sentencepiece-comments_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def median_ms(fn, warmup, launches):
    out = []
    for k in range(warmup + launches):
        t = fn()
        if k >= warmup:
            out.append(t)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, default=1_000_000)
    ap.add_argument("--ja-lines", type=int, default=1_000_000)
    ap.add_argument("--launches", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import oracle_lib
    import spm_amd
    import synth
    if not torch.cuda.is_available():
        sys.exit("decode_bench: no GPU; nothing measured")
    dev = torch.device("cuda", 0)
    lines = []

    def encode(model_path, buf, off):
        mbytes = open(model_path, "rb").read()
        dm = spm_amd.DeviceModel(mbytes)
        n, total = len(off) - 1, int(off[-1])
        d_bytes = torch.from_numpy(buf).to(dev)
        d_off = torch.from_numpy(off.view(np.int64)).to(dev)
        d_ids = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        d_tok = torch.empty(n + 1, dtype=torch.int64, device=dev)
        dm.encode_device(d_bytes.data_ptr(), d_off.data_ptr(), n, d_ids.data_ptr(), d_tok.data_ptr())
        torch.cuda.synchronize(dev)
        tokens = int(d_tok[-1].item())
        return mbytes, dm, n, d_ids[:tokens].clone(), d_tok, tokens

    def leg(name, model_path, buf, off):
        mbytes, dm, n, d_ids, d_tok, tokens = encode(model_path, buf, off)
        d_ooff = torch.empty(n + 1, dtype=torch.int64, device=dev)
        total = dm.decode_device("", d_ids.data_ptr(), d_tok.data_ptr(), n, None, 0, d_ooff.data_ptr())
        d_out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        d_st = torch.zeros(1, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream

        def blocking():
            t0 = time.perf_counter()
            dm.decode_device("", d_ids.data_ptr(), d_tok.data_ptr(), n, d_out.data_ptr(), total, d_ooff.data_ptr())
            return (time.perf_counter() - t0) * 1e3

        def kernels():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dm.decode_device_async("", d_ids.data_ptr(), d_tok.data_ptr(), n, d_out.data_ptr(), total,
                                   d_ooff.data_ptr(), d_st.data_ptr(), stream=stream)
            e1.record()
            torch.cuda.synchronize(dev)
            return e0.elapsed_time(e1)

        moved = 4 * tokens + 8 * (n + 1) + total + 8 * (n + 1)
        src = torch.empty(moved, dtype=torch.uint8, device=dev)
        dst = torch.empty(moved, dtype=torch.uint8, device=dev)

        def copy():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1.record()
            torch.cuda.synchronize(dev)
            return e0.elapsed_time(e1)

        b = median_ms(blocking, args.warmup, args.launches)
        k = median_ms(kernels, args.warmup, args.launches)
        c = median_ms(copy, args.warmup, args.launches)
        assert int(d_st.item()) == 0
        ids = d_ids.cpu().numpy()
        tok = d_tok.cpu().numpy().view(np.uint64)
        hm = spm_amd.DeviceModel(mbytes, host_only=True)
        t0 = time.perf_counter()
        text, ooff = hm.decode_csr_host(ids, tok, capacity=total)
        host_ms = (time.perf_counter() - t0) * 1e3
        same = bool(np.array_equal(text, d_out.cpu().numpy()[:total])) and \
            bool(np.array_equal(ooff, d_ooff.cpu().numpy().view(np.uint64)))
        kernel_bw, copy_bw = moved / (k[0] * 1e-3) / 1e9, 2 * moved / (c[0] * 1e-3) / 1e9
        lines.append("%s: %d sentences, %d tokens, %d text bytes, %d bytes moved per call (ids + offsets in, text + "
                     "offsets out); device output == host loop: %s" % (name, n, tokens, total, moved, same))
        lines.append("%s  spm_hip_decode_batch (blocking) median %.3f ms (min %.3f, max %.3f), %.3e tokens/s"
                     % (name, b[0], b[1], b[2], tokens / (b[0] * 1e-3)))
        lines.append("%s  kernels alone (async call, HIP events) median %.3f ms (min %.3f, max %.3f): %.1f GB/s of "
                     "needed traffic" % (name, k[0], k[1], k[2], kernel_bw))
        lines.append("%s  device-to-device copy of %d bytes median %.3f ms: %.1f GB/s read + written; decode reaches "
                     "%.2f of the copy's bandwidth" % (name, moved, c[0], copy_bw, kernel_bw / copy_bw))
        lines.append("%s  host loop, one thread: %.1f ms, %.3e tokens/s; the blocking device call is %.1f x faster"
                     % (name, host_ms, tokens / (host_ms * 1e-3), host_ms / b[0]))
        return dm, hm, ids, tok

    buf, off = synth.normalized(args.sentences, seed=1234)
    dm, hm, ids, tok = leg("c2", os.path.join(ROOT, "data", "synth32k_unigram.model"), buf, off)

    # Crossover on the c2 ids: host loop against upload + device decode + download.
    bound = dm.decode_bound()
    cross = None
    for n in (1, 4, 16, 64, 256, 1024, 4096, 16384, 65536, 262144):
        if n > len(tok) - 1:
            break
        sub_tok = tok[:n + 1].copy()
        sub_ids = ids[:int(sub_tok[-1])]
        cap = int(sub_tok[-1]) * bound

        def host():
            t0 = time.perf_counter()
            hm.decode_csr_host(sub_ids, sub_tok, capacity=cap)
            return (time.perf_counter() - t0) * 1e3

        def device():
            t0 = time.perf_counter()
            dm.decode_csr_host(sub_ids, sub_tok, capacity=cap)
            return (time.perf_counter() - t0) * 1e3

        h = median_ms(host, 2, 9)[0]
        d = median_ms(device, 2, 9)[0]
        if cross is None and d < h:
            cross = int(sub_tok[-1])
        lines.append("crossover  %7d sentences, %8d tokens: host loop %.4f ms, host-buffer device call %.4f ms"
                     % (n, int(sub_tok[-1]), h, d))
    lines.append("crossover  the device call first wins at %s tokens"
                 % (cross if cross is not None else "no measured size: more than %d" % int(tok[-1])))
    del dm, hm, ids, tok

    if args.ja_lines > 0:
        gold = os.path.join(ROOT, "tests", "golden")
        mpath = os.path.join(gold, "test_ja_model.model")
        raw = oracle_lib.read_lines_binary(os.path.join(gold, "wagahaiwa_nekodearu.txt"))
        reps = (args.ja_lines + len(raw) - 1) // len(raw)
        hn = spm_amd.DeviceModel(open(mpath, "rb").read(), host_only=True)
        rb, ro = spm_amd.to_csr(raw)
        nb, no = hn.normalize_csr(rb, ro, threads=16)
        lens = np.tile((no[1:] - no[:-1]).astype(np.uint64), reps)
        joff = np.zeros(len(lens) + 1, dtype=np.uint64)
        joff[1:] = np.cumsum(lens, dtype=np.uint64)
        leg("ja", mpath, np.tile(nb[:int(no[-1])], reps), joff)

    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
