#!/usr/bin/env python3
"""Speed of the piece count (spm_hip_count_ids) and of the in-place type
change (spm_hip_model_set_piece_types) on ids resident in HBM.

Two id streams are made on the device first: bench.py's c2 workload (synthetic
sentences of tools/synth.py seed 1234, the 32k unigram model) and c3 (the same
text, the 32k BPE model).  Per stream, in one run:

  * the count kernel alone (HIP events around spm_hip_count_ids): warm-up,
    then the median of --launches calls, and its result against
    numpy.bincount;
  * a device-to-device copy of the ids' bytes as the traffic bound (the count
    only reads them, the copy reads and writes them);
  * the host loop a caller would otherwise run: numpy.bincount over the same
    ids, one thread;
  * the count of a stream of the same length that holds one id only: the
    worst case for contention on a counter;
  * spm_hip_model_set_piece_types (blocking, host clock): every second
    multi-character NORMAL piece to UNUSED and back.

  python tools/vocab_bench.py [--sentences N] [--out FILE]
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
    ap.add_argument("--sentences", type=int, default=10_000_000)
    ap.add_argument("--launches", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import spm_amd
    import synth
    if not torch.cuda.is_available():
        sys.exit("vocab_bench: no GPU; nothing measured")
    dev = torch.device("cuda", 0)
    lines = []
    buf, off = synth.normalized(args.sentences, seed=1234)
    d_bytes = torch.from_numpy(buf).to(dev)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    n, total = len(off) - 1, int(off[-1])

    def leg(name, model_path):
        dm = spm_amd.DeviceModel(open(model_path, "rb").read())
        v = dm.info().piece_size
        d_all = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        d_tok = torch.empty(n + 1, dtype=torch.int64, device=dev)
        dm.encode_device(d_bytes.data_ptr(), d_off.data_ptr(), n, d_all.data_ptr(), d_tok.data_ptr())
        torch.cuda.synchronize(dev)
        tokens = int(d_tok[-1].item())
        d_ids = d_all[:tokens].clone()
        del d_all
        d_one = torch.full((tokens,), 7, dtype=torch.int32, device=dev)
        d_counts = torch.zeros(v, dtype=torch.int64, device=dev)
        d_st = torch.zeros(1, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream

        def count(d_src):
            def run():
                d_counts.zero_()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                dm.count_ids_device(d_src.data_ptr(), tokens, d_counts.data_ptr(), d_st.data_ptr(), stream=stream)
                e1.record()
                torch.cuda.synchronize(dev)
                return e0.elapsed_time(e1)
            return run

        dst = torch.empty_like(d_ids)

        def copy():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(d_ids)
            e1.record()
            torch.cuda.synchronize(dev)
            return e0.elapsed_time(e1)

        k = median_ms(count(d_ids), args.warmup, args.launches)
        got = d_counts.cpu().numpy()
        one = median_ms(count(d_one), args.warmup, args.launches)
        one_ok = int(d_counts[7].item()) == tokens and int(d_counts.sum().item()) == tokens
        c = median_ms(copy, args.warmup, args.launches)
        assert int(d_st.item()) == 0
        ids = d_ids.cpu().numpy()
        t0 = time.perf_counter()
        want = np.bincount(ids, minlength=v)
        host_ms = (time.perf_counter() - t0) * 1e3
        same = bool(np.array_equal(got, want))
        top = float(want.max()) / max(tokens, 1)
        nbytes = 4 * tokens
        lines.append("%s: %d sentences, %d tokens (%d id bytes), %d pieces, commonest id %.2f %% of the tokens; "
                     "device counts == numpy.bincount: %s" % (name, n, tokens, nbytes, v, 100 * top, same))
        lines.append("%s  spm_hip_count_ids (kernel, HIP events) median %.3f ms (min %.3f, max %.3f): %.3e tokens/s, "
                     "%.1f GB/s of ids read" % (name, k[0], k[1], k[2], tokens / (k[0] * 1e-3),
                                               nbytes / (k[0] * 1e-3) / 1e9))
        lines.append("%s  the same length of one id median %.3f ms (min %.3f, max %.3f), counts right: %s; %.2f x the "
                     "real stream's time" % (name, one[0], one[1], one[2], one_ok, one[0] / k[0]))
        lines.append("%s  device-to-device copy of the ids median %.3f ms: %.1f GB/s read + written; the count reads "
                     "at %.2f of the copy's read rate" % (name, c[0], 2 * nbytes / (c[0] * 1e-3) / 1e9, c[0] / k[0]))
        lines.append("%s  host loop (numpy.bincount, one thread): %.1f ms, %.3e tokens/s; the device kernel is %.0f x "
                     "faster" % (name, host_ms, tokens / (host_ms * 1e-3), host_ms / k[0]))
        del d_one, dst
        # Type change: every second multi-character NORMAL piece, there and back.
        t_all = dm.piece_types()
        multi = np.nonzero(t_all == 1)[0]
        from model_reader import read_pieces
        pieces = read_pieces(open(model_path, "rb").read())
        multi = np.array([i for i in multi if len(pieces[i][0].decode(errors="replace")) > 1])
        t_half = t_all.copy()
        t_half[multi[::2]] = 5
        flip = [t_half, t_all]
        state = [0]

        def retag():
            t0 = time.perf_counter()
            dm.set_piece_types(flip[state[0] % 2])
            state[0] += 1
            return (time.perf_counter() - t0) * 1e3

        r = median_ms(retag, 2, 2 * (args.launches // 2) + 2)
        inf = dm.info()
        lines.append("%s  spm_hip_model_set_piece_types (blocking, %d of %d pieces change, %d trie units) median "
                     "%.3f ms (min %.3f, max %.3f)" % (name, len(multi[::2]), v, inf.trie_units, r[0], r[1], r[2]))

    leg("c2", os.path.join(ROOT, "data", "synth32k_unigram.model"))
    leg("c3", os.path.join(ROOT, "data", "synth32k_bpe.model"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
