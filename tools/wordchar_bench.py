#!/usr/bin/env python3
"""Speed of the WORD / CHAR device encode (wordchar_kernels.hip).

Models for the synthetic batch of tools/synth.py (seed 1234):
  CHAR  the single-char pieces of data/synth32k_unigram.model
  WORD  the 32000 most frequent words of the first million synth lines
and tests/golden/wagahaiwa_char2000.model for the Japanese lines
(tests/golden/wagahaiwa_nekodearu.txt, normalized, repeated to --ja-lines).

Per leg (model x batch), in one run:
  * spm_hip_encode_batch (blocking; host clock around it, it ends in a
    stream synchronization): warm-up, then the median of --launches calls;
    the tile-tier and general-tier kernel times the call's stats report;
  * the whole chain of kernels (HIP events around
    spm_hip_encode_batch_async), the bytes the call has to move (text and
    offsets in, ids and token offsets out) over that time, against a
    device-to-device copy of a buffer of that size (which reads and writes it);
  * the `sentencepiece` package's encode of the same normalized lines on one
    thread (a model with identity normalization and no dummy prefix, so the
    package tokenizes what the device call tokenizes); beyond --package-lines
    lines only the first --package-lines are timed and the line says so;
  * the unigram encode of the same batch (the fast kernel's time from the
    call's stats), for scale.

  python tools/wordchar_bench.py [--sentences 1000000,10000000] [--ja-lines N] [--out FILE]
"""
import argparse
import collections
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sentencepiece-comments_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
WS = "▁".encode()


def median3(fn, warmup, launches):
    out = [fn() for _ in range(warmup + launches)][warmup:]
    return statistics.median(out), min(out), max(out)


def char_model(builder, reader):
    """The single-char pieces of the synthetic unigram model."""
    src = reader.read_pieces(open(os.path.join(ROOT, "data", "synth32k_unigram.model"), "rb").read())
    singles = [(p, s, builder.NORMAL) for p, s, t in src if t == builder.NORMAL and len(p.decode("utf-8")) == 1]
    return builder.base_pieces() + singles


def word_model(builder, buf, off, lines, size=32000):
    """The most frequent words of the first `lines` sentences."""
    data = buf.tobytes()
    count = collections.Counter()
    for i in range(min(lines, len(off) - 1)):
        parts = data[int(off[i]):int(off[i + 1])].split(WS)
        if parts[0]:
            count[parts[0]] += 1
        count.update(WS + w for w in parts[1:])
    words = sorted(count.items(), key=lambda kv: (-kv[1], kv[0]))[:size]
    return builder.base_pieces() + [(w, 0.0, builder.NORMAL) for w, _ in words]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", default="1000000,10000000")
    ap.add_argument("--ja-lines", type=int, default=1_000_000)
    ap.add_argument("--package-lines", type=int, default=1_000_000)
    ap.add_argument("--launches", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import model_builder
    import model_reader
    import oracle_lib
    import sentencepiece
    import spm_amd
    import synth
    if not torch.cuda.is_available():
        sys.exit("wordchar_bench: no GPU; nothing measured")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = []

    def say(s):
        out.append(s)
        print(s, flush=True)

    def leg(name, mbytes, pkg_bytes, uni_bytes, buf, off):
        n, total = len(off) - 1, int(off[-1])
        dm = spm_amd.DeviceModel(mbytes)
        dm.set_timing(True)
        d_bytes = torch.from_numpy(buf[:max(total, 1)]).to(dev)
        d_off = torch.from_numpy(off.view(np.int64)).to(dev)
        d_ids = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        d_tok = torch.empty(n + 1, dtype=torch.int64, device=dev)
        d_st = torch.zeros(1, dtype=torch.int32, device=dev)
        tiers = []

        def blocking():
            t0 = time.perf_counter()
            dm.encode_device(d_bytes.data_ptr(), d_off.data_ptr(), n, d_ids.data_ptr(), d_tok.data_ptr(), stream=stream)
            t = (time.perf_counter() - t0) * 1e3
            st = dm.stats()
            tiers.append((st.fast_kernel_ms, st.general_kernel_ms, st.general_path))
            return t

        def chain():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dm.encode_device_async(d_bytes.data_ptr(), d_off.data_ptr(), n, total, d_ids.data_ptr(), d_tok.data_ptr(),
                                   d_st.data_ptr(), stream=stream)
            e1.record()
            torch.cuda.synchronize(dev)
            return e0.elapsed_time(e1)

        b = median3(blocking, args.warmup, args.launches)
        tokens = int(d_tok[-1].item())
        tile_ms = statistics.median(t[0] for t in tiers[args.warmup:])
        gen_ms = statistics.median(t[1] for t in tiers[args.warmup:])
        k = median3(chain, args.warmup, args.launches)
        assert int(d_st.item()) == 0
        moved = total + 8 * (n + 1) + 4 * tokens + 8 * (n + 1)
        src = torch.empty(moved, dtype=torch.uint8, device=dev)
        dst = torch.empty(moved, dtype=torch.uint8, device=dev)

        def copy():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1.record()
            torch.cuda.synchronize(dev)
            return e0.elapsed_time(e1)

        c = median3(copy, args.warmup, args.launches)
        del src, dst
        need_bw, copy_bw = moved / (k[0] * 1e-3) / 1e9, 2 * moved / (c[0] * 1e-3) / 1e9
        say("%s: %d sentences, %d bytes, %d tokens, %d bytes moved per call (text + offsets in, ids + token offsets "
            "out); general tier ran %d sentences" % (name, n, total, tokens, moved, tiers[-1][2]))
        say("%s  spm_hip_encode_batch (blocking) median %.3f ms (min %.3f, max %.3f), %.3e tokens/s"
            % (name, b[0], b[1], b[2], tokens / (b[0] * 1e-3)))
        say("%s  kernel times of the call's stats: tile tier (wc_mark_kernel) %.3f ms, general tier "
            "(wc_general_kernel) %.3f ms" % (name, tile_ms, gen_ms))
        say("%s  all kernels (async call, HIP events) median %.3f ms (min %.3f, max %.3f): %.1f GB/s of needed "
            "traffic; a device-to-device copy of %d bytes takes %.3f ms (%.1f GB/s read + written): the encode "
            "reaches %.3f of the copy's bandwidth" % (name, k[0], k[1], k[2], need_bw, moved, c[0], copy_bw,
                                                      need_bw / copy_bw))
        # The package, one thread, on the same normalized lines.
        m = min(n, args.package_lines)
        data = buf.tobytes()
        text = [data[int(off[i]):int(off[i + 1])].decode("utf-8") for i in range(m)]
        sp = sentencepiece.SentencePieceProcessor(model_proto=pkg_bytes, num_threads=1)
        sp.encode(text[:1000], out_type=int)
        t0 = time.perf_counter()
        rows = sp.encode(text, out_type=int, num_threads=1)
        pkg_ms = (time.perf_counter() - t0) * 1e3
        pkg_tokens = sum(len(r) for r in rows)
        ids = d_ids[:int(d_tok[m].item())].cpu().numpy()
        same = pkg_tokens <= len(ids)  # the package merges unknown runs; equal when there is no unknown run
        say("%s  sentencepiece %s encode, one thread, %s%d lines: %.1f ms (%d tokens after its unknown-run merge, the "
            "device call's %d before it: %s); per line the blocking device call is %.1f x faster"
            % (name, sentencepiece.__version__, "the first " if m < n else "", m, pkg_ms, pkg_tokens, len(ids),
               "consistent" if same else "INCONSISTENT", (pkg_ms / m) / (b[0] / n)))
        del text, rows, data
        um = spm_amd.DeviceModel(uni_bytes)
        um.set_timing(True)
        uni = []

        def unigram():
            t0 = time.perf_counter()
            um.encode_device(d_bytes.data_ptr(), d_off.data_ptr(), n, d_ids.data_ptr(), d_tok.data_ptr(), stream=stream)
            t = (time.perf_counter() - t0) * 1e3
            uni.append(um.stats().fast_kernel_ms)
            return t

        u = median3(unigram, args.warmup, args.launches)
        say("%s  unigram encode of the same batch: blocking call median %.3f ms (min %.3f, max %.3f), its fast kernel "
            "%.3f ms" % (name, u[0], u[1], u[2], statistics.median(uni[args.warmup:])))

    def package_model(pieces, kind):
        return model_builder.model(pieces, model_type=kind, add_dummy_prefix=False, remove_extra_whitespaces=False)

    uni_bytes = open(os.path.join(ROOT, "data", "synth32k_unigram.model"), "rb").read()
    sizes = [int(x) for x in args.sentences.split(",") if x]
    cpieces = wpieces = None
    for size in sizes:
        buf, off = synth.normalized(size, seed=1234)
        if cpieces is None:
            cpieces = char_model(model_builder, model_reader)
            wpieces = word_model(model_builder, buf, off, 1_000_000)
            say("models: CHAR %d pieces, WORD %d pieces" % (len(cpieces), len(wpieces)))
        tag = "%dM" % (size // 1_000_000) if size % 1_000_000 == 0 else str(size)
        leg("char %s" % tag, model_builder.model(cpieces, model_type=4), package_model(cpieces, 4), uni_bytes, buf, off)
        leg("word %s" % tag, model_builder.model(wpieces, model_type=3), package_model(wpieces, 3), uni_bytes, buf, off)
        del buf, off
    if args.ja_lines > 0:
        gold = os.path.join(ROOT, "tests", "golden")
        mbytes = open(os.path.join(gold, "wagahaiwa_char2000.model"), "rb").read()
        raw = oracle_lib.read_lines_binary(os.path.join(gold, "wagahaiwa_nekodearu.txt"))
        reps = (args.ja_lines + len(raw) - 1) // len(raw)
        hn = spm_amd.DeviceModel(mbytes, host_only=True)
        rb, ro = spm_amd.to_csr(raw)
        nb, no = hn.normalize_csr(rb, ro, threads=16)
        lens = np.tile((no[1:] - no[:-1]).astype(np.uint64), reps)
        joff = np.zeros(len(lens) + 1, dtype=np.uint64)
        joff[1:] = np.cumsum(lens, dtype=np.uint64)
        pieces = model_reader.read_pieces(mbytes)
        leg("char ja", mbytes, package_model(pieces, 4),
            open(os.path.join(gold, "test_ja_model.model"), "rb").read(), np.tile(nb[:int(no[-1])], reps), joff)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
