#!/usr/bin/env python3
"""Speed of the byte-fallback epilogue and decode on buffers resident in HBM.

Model: tests/golden/botchan_bf_unigram1k.model (byte_fallback, English).  The
"plain" model of the comparisons is the same model with its BYTE rows typed
CONTROL and the byte_fallback flag cleared: it gives the same model-level tokens and
runs the code a model without byte fallback has always run.

  busy    spm_hip_finalize_ids_bytes on wagahaiwa_nekodearu.txt x --copies
          (Japanese text: all but ~0.3 % of the output ids are bytes): output
          ids/s, and the needed traffic (ids + lengths + offsets + text in, ids
          + offsets out) against a device-to-device copy of that many bytes.
  idle    the same call over text without unknown chars (botchan lines that
          encode without a byte id, x --idle-copies) against
          spm_hip_finalize_ids of the plain model on the same token stream;
          the spread is the plain call against itself (two runs).
  decode  spm_hip_decode_batch_async on the busy leg's output ids (byte runs)
          against the plain model's decode of an id stream of the same length
          without byte ids (the idle leg's ids, tiled).

Kernel times are HIP events around the pure stream entries: warm-up, then the
median of --launches calls.

  python tools/byte_fallback_bench.py [--copies N] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sentencepiece-comments_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=90)        # x 1 111 622 ids: about 100 M
    ap.add_argument("--idle-copies", type=int, default=400)  # x ~42 k tokens
    ap.add_argument("--launches", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import byte_fallback_ref as R
    import spm_amd
    if not torch.cuda.is_available():
        sys.exit("byte_fallback_bench: no GPU; nothing measured")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    out_lines = []

    def median_ms(fn):
        ts = []
        for k in range(args.warmup + args.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize(dev)
            if k >= args.warmup:
                ts.append(e0.elapsed_time(e1))
        return statistics.median(ts), min(ts), max(ts)

    def copy_gbs(nbytes):
        src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        dst = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ms = median_ms(lambda: dst.copy_(src))[0]
        return 2 * nbytes / (ms * 1e-3) / 1e9, ms

    mbytes = R.fixture_model(R.FIXTURES[0])
    bf = spm_amd.DeviceModel(mbytes)
    plain = spm_amd.DeviceModel(R.plain_view(mbytes))
    host = spm_amd.DeviceModel(mbytes, host_only=True)

    class Batch:
        """Raw lines x copies, normalized on the host, tiled, encoded on the device."""

        def __init__(self, lines, copies):
            rb, ro = spm_amd.to_csr(lines)
            nb, no = host.normalize_csr(rb, ro, threads=16)
            lens = np.tile((no[1:] - no[:-1]).astype(np.uint64), copies)
            off = np.zeros(len(lens) + 1, dtype=np.uint64)
            off[1:] = np.cumsum(lens, dtype=np.uint64)
            self.n, self.bytes = len(lens), int(off[-1])
            self.d_norm = torch.from_numpy(np.tile(nb[:int(no[-1])], copies)).to(dev)
            self.d_noff = torch.from_numpy(off.view(np.int64)).to(dev)
            self.d_ids = torch.empty(max(self.bytes, 1), dtype=torch.int32, device=dev)
            self.d_len = torch.empty(max(self.bytes, 1), dtype=torch.int32, device=dev)
            self.d_tok = torch.empty(self.n + 1, dtype=torch.int64, device=dev)
            bf.encode_device(self.d_norm.data_ptr(), self.d_noff.data_ptr(), self.n, self.d_ids.data_ptr(),
                             self.d_tok.data_ptr(), d_len=self.d_len.data_ptr())
            torch.cuda.synchronize(dev)
            self.tokens = int(self.d_tok[-1].item())
            self.d_out = torch.empty(max(self.bytes, 1), dtype=torch.int32, device=dev)
            self.d_ooff = torch.empty(self.n + 1, dtype=torch.int64, device=dev)
            self.d_st = torch.zeros(1, dtype=torch.int32, device=dev)

        def finalize_bytes(self):
            bf.finalize_ids_bytes_device_async("", self.d_ids.data_ptr(), self.d_len.data_ptr(), self.d_tok.data_ptr(),
                                               self.n, self.d_norm.data_ptr(), self.d_noff.data_ptr(),
                                               self.d_out.data_ptr(), self.bytes, self.d_ooff.data_ptr(),
                                               self.d_st.data_ptr(), stream=stream)

        def finalize_plain(self):
            plain.finalize_ids_device_async("", self.d_ids.data_ptr(), self.d_tok.data_ptr(), self.n,
                                            self.d_out.data_ptr(), self.bytes, self.d_ooff.data_ptr(),
                                            self.d_st.data_ptr(), stream=stream)

    # ---- busy ----
    busy = Batch(R.corpus_lines("wagahaiwa_nekodearu.txt"), args.copies)
    k = median_ms(busy.finalize_bytes)
    assert int(busy.d_st.item()) == 0
    outs = int(busy.d_ooff[-1].item())
    want_off, want_ids, _, _ = R.recorded_spt("wagahaiwa", R.FIXTURES[0])
    same = bool(np.array_equal(busy.d_out[:len(want_ids)].cpu().numpy(), want_ids)) and outs == args.copies * len(want_ids)
    moved = 8 * busy.tokens + 16 * (busy.n + 1) + busy.bytes + 4 * outs + 8 * (busy.n + 1)
    cbw, cms = copy_gbs(moved)
    bw = moved / (k[0] * 1e-3) / 1e9
    out_lines.append("busy   wagahaiwa x %d: %d lines, %d model tokens, %d output ids (first copy == the package's: %s)"
                     % (args.copies, busy.n, busy.tokens, outs, same))
    out_lines.append("busy   spm_hip_finalize_ids_bytes kernels median %.3f ms (min %.3f, max %.3f): %.3e output ids/s"
                     % (k[0], k[1], k[2], outs / (k[0] * 1e-3)))
    out_lines.append("busy   needed traffic %d bytes: %.1f GB/s; a device copy of that size takes %.3f ms (%.1f GB/s "
                     "read + written): the epilogue reaches %.2f of the copy's bandwidth" % (moved, bw, cms, cbw, bw / cbw))

    # ---- decode of the byte ids against ids without bytes ----
    def decode_leg(name, dm, d_ids, d_tok, n):
        d_ooff = torch.empty(n + 1, dtype=torch.int64, device=dev)
        total = dm.decode_device("", d_ids.data_ptr(), d_tok.data_ptr(), n, None, 0, d_ooff.data_ptr())
        d_text = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        d_st = torch.zeros(1, dtype=torch.int32, device=dev)
        t = median_ms(lambda: dm.decode_device_async("", d_ids.data_ptr(), d_tok.data_ptr(), n, d_text.data_ptr(),
                                                     total, d_ooff.data_ptr(), d_st.data_ptr(), stream=stream))
        assert int(d_st.item()) == 0
        tokens = int(d_tok[-1].item())
        out_lines.append("decode %s: %d ids -> %d text bytes, kernels median %.3f ms (min %.3f, max %.3f): %.3e ids/s"
                         % (name, tokens, total, t[0], t[1], t[2], tokens / (t[0] * 1e-3)))
        return t[0], tokens

    byte_ms, byte_tokens = decode_leg("byte runs (byte-fallback model)", bf, busy.d_out, busy.d_ooff, busy.n)
    del busy

    # ---- idle ----
    off, ids, _, _ = R.recorded_spt("botchan", R.FIXTURES[0])
    is_byte = np.isin(ids, np.array(R.byte_ids(mbytes)))
    has = np.add.reduceat(is_byte, off[:-1].astype(np.int64)) * (np.diff(off.astype(np.int64)) > 0)
    lines = [l for l, h in zip(R.corpus_lines("botchan.txt"), has) if h == 0 and l]
    idle = Batch(lines, args.idle_copies)
    a = median_ms(idle.finalize_plain)
    b = median_ms(idle.finalize_plain)
    plain_out = idle.d_out[:idle.tokens].clone()
    c = median_ms(idle.finalize_bytes)
    assert int(idle.d_st.item()) == 0 and int(idle.d_ooff[-1].item()) == idle.tokens
    assert bool(torch.equal(plain_out, idle.d_out[:idle.tokens]))
    out_lines.append("idle   botchan lines without unknown chars x %d: %d lines, %d tokens, no byte id"
                     % (args.idle_copies, idle.n, idle.tokens))
    out_lines.append("idle   spm_hip_finalize_ids (plain model) median %.3f ms, again %.3f ms (spread %.1f %%)"
                     % (a[0], b[0], 100 * abs(a[0] - b[0]) / min(a[0], b[0])))
    out_lines.append("idle   spm_hip_finalize_ids_bytes (byte-fallback model, same tokens, same output) median %.3f ms: "
                     "%.2f x the plain call" % (c[0], c[0] / min(a[0], b[0])))

    reps = max(1, byte_tokens // idle.tokens)
    per = idle.d_tok.cpu().numpy()
    lens = np.tile(np.diff(per), reps)
    tok = np.zeros(len(lens) + 1, dtype=np.int64)
    tok[1:] = np.cumsum(lens)
    d_ids = idle.d_out[:idle.tokens].repeat(reps)
    plain_ms, plain_tokens = decode_leg("no byte ids (plain model)", plain, d_ids, torch.from_numpy(tok).to(dev),
                                        len(lens))
    out_lines.append("decode per id: byte runs %.3f ns, no byte ids %.3f ns (%.2f x)"
                     % (byte_ms * 1e6 / byte_tokens, plain_ms * 1e6 / plain_tokens,
                        (byte_ms / byte_tokens) / (plain_ms / plain_tokens)))

    text = "\n".join(out_lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
