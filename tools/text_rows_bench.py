"""Time the three text-row kernel groups against a device copy of the bytes
each must read and write (torch events, default stream).  Runs alternate:
call, copy, call, copy, ... `--reps` of each; prints every time and the median.

  python tools/text_rows_bench.py [--lines 1000000] [--reps 3]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sentencepiece-comments_amd"))
import spm_amd as S  # noqa: E402


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--c2", action="store_true", help="id rows only, over a synthetic id CSR of the c2 shape: "
                    "10 M sentences of 1..8 ids below 32000")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    gold = os.path.join(ROOT, "tests", "golden")
    text = open(os.path.join(gold, "botchan.txt"), "rb").read()
    per = text.count(b"\n")
    text *= max(1, a.lines // per)
    dm = S.DeviceModel(open(os.path.join(gold, "test_model.model"), "rb").read())
    scratch = torch.empty(S.TEXT_ROWS_SCRATCH_BYTES, dtype=torch.uint8, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def report(name, call, nbytes, env=None):
        for k in ("SPM_HIP_TEXT_ROWS_FORM", "SPM_HIP_TEXT_ROWS_PIECE_WAVE"):
            os.environ.pop(k, None)
        os.environ.update(env or {})
        name = "%s %s" % (name, " ".join(v for v in (env or {}).values()) or "default")
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        call()
        dst.copy_(src)
        t_call, t_copy = [], []
        for _ in range(a.reps):
            t_call.append(timed(call))
            t_copy.append(timed(lambda: dst.copy_(src)))
        assert int(status[0].item()) == 0
        print("%-22s moves %6.1f MB  call ms %s median %.3f | copy ms %s median %.3f | ratio %.2f" % (
            name, nbytes / 1e6, ["%.3f" % x for x in t_call], np.median(t_call),
            ["%.3f" % x for x in t_copy], np.median(t_copy), np.median(t_call) / np.median(t_copy)), flush=True)

    if a.c2:
        n = 10000000
        lens = torch.randint(1, 9, (n,), device=dev, dtype=torch.int64)
        d_ooff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_ooff[1:] = torch.cumsum(lens, 0)
        k = int(d_ooff[n].item())
        d_ids = torch.randint(0, 32000, (k,), device=dev, dtype=torch.int32)
        cap = 11 * k + n
        d_rows = torch.empty(cap, dtype=torch.uint8, device=dev)
        d_roff = torch.empty(n + 1, dtype=torch.int64, device=dev)
        call = lambda: S.format_id_rows_device(d_ids.data_ptr(), d_ooff.data_ptr(), n, d_rows.data_ptr(),  # noqa: E731
                                               cap, d_roff.data_ptr(), status.data_ptr(), scratch.data_ptr())
        call()
        for form in ("image", "direct"):
            report("id rows c2", call, 4 * k + 16 * n + int(d_roff[n].item()), {"SPM_HIP_TEXT_ROWS_FORM": form})
        print("sentences %d, ids %d" % (n, k))
        return
    d_lines, d_off, n, line_bytes = dm.split_text_device(text)
    d_text = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(dev)
    d_out = torch.empty(len(text), dtype=torch.uint8, device=dev)
    d_o = torch.empty(n + 1, dtype=torch.int64, device=dev)
    for form in ("image", "direct"):
        report("split", lambda: S.split_lines_device(d_text.data_ptr(), len(text), d_out.data_ptr(), d_o.data_ptr(),
                                                     n, status.data_ptr(), scratch.data_ptr()),
               len(text) + line_bytes + 8 * n, {"SPM_HIP_TEXT_ROWS_FORM": form})

    d_ids, d_ooff, k = dm._device_csr_to_id_csr(d_lines, d_off, n, line_bytes)
    cap = 11 * k + n
    d_rows = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_roff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    call = lambda: S.format_id_rows_device(d_ids.data_ptr(), d_ooff.data_ptr(), n, d_rows.data_ptr(), cap,  # noqa: E731
                                           d_roff.data_ptr(), status.data_ptr(), scratch.data_ptr())
    call()
    for form in ("image", "direct"):
        report("id rows", call, 4 * k + 16 * n + int(d_roff[n].item()), {"SPM_HIP_TEXT_ROWS_FORM": form})

    d_norm, d_noff, d_p, d_po, tn, tp = dm._spt_records_device(d_lines, d_off, n, line_bytes)
    cap = tn.value + 8 * tp.value + n
    d_rows = torch.empty(cap, dtype=torch.uint8, device=dev)
    call = lambda: dm.format_piece_rows_device(d_p.data_ptr(), d_po.data_ptr(), n, d_norm.data_ptr(),  # noqa: E731
                                               d_noff.data_ptr(), d_rows.data_ptr(), cap, d_roff.data_ptr(),
                                               status.data_ptr(), scratch.data_ptr())
    call()
    for wave in ("0", "4", "8", "16", "32", "64", "128"):  # 0: laid out over the output bytes
        report("piece rows wave>", call, 20 * tp.value + tn.value + 24 * n + int(d_roff[n].item()),
               {"SPM_HIP_TEXT_ROWS_PIECE_WAVE": wave})
    print("lines %d, text %.1f MB, ids %d, pieces %d" % (n, len(text) / 1e6, k, tp.value))


if __name__ == "__main__":
    main()
