#!/usr/bin/env python3
"""spm_hip_fit_ids on bench.py's c2 id batch (10 M synthetic sentences, 4.4 ids
each), for finding where its time goes.

  python tools/fit_passes.py --geometry 16,128 --geometry 16,256 ...
      per "branch,top_walk" (the SPM_HIP_FIT_GEOMETRY test knob): the call's
      time by HIP events (median, min, max of --reps runs), its scratch and
      its table levels, at every --row-len.
  rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/fit_passes.py --geometry 16,128 --reps 5
      then python tools/rocprof_summary.py DIR/.../run_results.db gives the
      time per kernel, which is the split between the passes.
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
    ap.add_argument("--geometry", action="append", default=None)
    ap.add_argument("--row-len", type=int, action="append", default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import spm_amd
    import synth
    if not torch.cuda.is_available():
        sys.exit("fit_passes: no GPU; nothing measured")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    buf, off = synth.normalized(args.sentences, seed=1234)
    dm = spm_amd.DeviceModel(open(os.path.join(ROOT, "data", "synth32k_unigram.model"), "rb").read())
    n = len(off) - 1
    d_bytes = torch.from_numpy(buf).to(dev)
    d_boff = torch.from_numpy(off.view(np.int64)).to(dev)
    ids = torch.empty(max(int(off[-1]), 1), dtype=torch.int32, device=dev)
    ioff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    dm.encode_device(d_bytes.data_ptr(), d_boff.data_ptr(), n, ids.data_ptr(), ioff.data_ptr())
    torch.cuda.synchronize(dev)
    T = int(ioff[-1].item())
    del d_bytes, d_boff, dm
    lines = ["fit_passes: %s; %d sentences, %d ids, tile %d sentences" % (" ".join(sys.argv[1:]), n, T,
                                                                          spm_amd.FIT_TILE)]
    for L in args.row_len or [16, 2048]:
        cap = spm_amd.fit_rows_bound(T, n, L)
        out, seq, pos = (torch.empty((cap, L), dtype=torch.int32, device=dev) for _ in range(3))
        rl = torch.empty(cap, dtype=torch.int32, device=dev)
        place = torch.empty(n, dtype=torch.int64, device=dev)
        stats = torch.empty(4, dtype=torch.int64, device=dev)
        for geo in args.geometry or ["%d,%d" % (spm_amd.FIT_BRANCH, spm_amd.FIT_TOP_WALK)]:
            os.environ["SPM_HIP_FIT_GEOMETRY"] = geo
            nbytes = spm_amd.fit_ids_scratch_bytes(n, L, cap)
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            branch, walk = (int(x) for x in geo.split(","))
            tiles, levels = -(-n // spm_amd.FIT_TILE), 1
            while tiles > walk:
                tiles, levels = -(-tiles // branch), levels + 1
            ms = []
            for r in range(2 + args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                spm_amd.fit_ids_device(ids.data_ptr(), ioff.data_ptr(), n, L, -1, 0, cap, out.data_ptr(),
                                       scratch.data_ptr(), nbytes, seq.data_ptr(), pos.data_ptr(), rl.data_ptr(),
                                       place.data_ptr(), stats.data_ptr(), stream=stream)
                e1.record()
                torch.cuda.synchronize(dev)
                if r >= 2:
                    ms.append(e0.elapsed_time(e1))
            lines.append("L = %d, branch %d, top_walk %d: %d table levels, %d tiles walked at the top, %d bytes of "
                         "scratch, %d rows; median %.3f ms (min %.3f, max %.3f)"
                         % (L, branch, walk, levels, tiles, nbytes, int(stats[0].item()), statistics.median(ms),
                            min(ms), max(ms)))
            del scratch
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
