#!/usr/bin/env python3
"""CLAHE, equalizeHist and EnhanceLocalContrastByCLAHE (clahe.hip) on device-resident pages: one JSON line per workload.

    python tools/bench_clahe.py [--steps 10] [--warmup 3] [--repeats 5] [--only G,C,K] [--out FILE] [--no-check]

G   256 x A4 gray (2480 x 3508)
C   64 x A4 x 3 channels
K   256 x 4096 x 4096 gray

Per workload, in the same run on the same pages, between two device events on the current stream:
    clahe_ms       prl_hip_clahe_batch_device, clip limit 2.0, the 8 x 8 grid: tile histograms, tile tables, interpolation
    luts_ms        prl_hip_clahe_luts_batch_device alone: the first two of those stages (the tables are a few microseconds)
    interp_ms      clahe_ms - luts_ms: the interpolation stage, by difference (no entry runs it alone)
    equalize_ms    prl_hip_equalize_hist_batch_device: histogram, table, look-up
    enhance_ms     prl_hip_enhance_local_contrast_batch_device(2.0, equalize): CLAHE whose interpolation counts its output, table,
                   look-up in place
    histogram_ms, lut_ms, copy_ms   the yardsticks: prl_hip_histogram_batch_device, prl_hip_lut_batch_device (one table per page and
                   channel), a device-to-device copy of the batch
ms: per repeat the median of `steps` calls after `warmup`; the line reports the median, the minimum and the maximum of the `repeats`
medians.  clahe_over_hist_plus_lut = clahe_ms / (histogram_ms + lut_ms): CLAHE is one histogram-like pass plus one look-up-like pass
with four gathers.  One page of each workload is checked against tests/clahe_ref.py, outside the timed window.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_focus import make_pages, timed  # noqa: E402  (the same pages and the same timing rule)

RUNS = {"G": (256, 3508, 2480, 1), "C": (64, 3508, 2480, 3), "K": (256, 4096, 4096, 1)}
CLIP = 2.0


def run(torch, prl, args, name, n, h, w, c):
    import clahe_ref

    pages = make_pages(torch, n, h, w, c)
    out = torch.empty_like(pages)
    hist = torch.empty((n, c, 256), dtype=torch.int32, device="cuda")
    tables = torch.empty((n, c, 8, 8, 256), dtype=torch.uint8, device="cuda")
    ident = torch.arange(256, dtype=torch.uint8, device="cuda").repeat(n, c, 1).contiguous()
    t = lambda call: timed(torch, call, args.steps, args.warmup, args.repeats)  # noqa: E731
    m = dict(clahe=t(lambda: prl.clahe(pages, CLIP, out=out)), luts=t(lambda: prl.claheLuts(pages, CLIP, out=tables)),
             equalize=t(lambda: prl.equalizeHist(pages, out=out)), enhance=t(lambda: prl.enhanceLocalContrast(pages, CLIP, True, out=out)),
             histogram=t(lambda: prl.histogram(pages, out=hist)), lut=t(lambda: prl.lut(pages, ident, out=out)),
             copy=t(lambda: out.copy_(pages)))
    nbytes = pages.numel()
    rec = dict(workload=name, pages=n, height=h, width=w, channels=c, clip_limit=CLIP, tiles=[8, 8], steps=args.steps, warmup=args.warmup,
               repeats=args.repeats, bytes=nbytes)
    for k, v in m.items():
        rec[k + "_ms"], rec[k + "_ms_min"], rec[k + "_ms_max"] = v
    rec["interp_ms"] = round(m["clahe"][0] - m["luts"][0], 4)
    base = m["histogram"][0] + m["lut"][0]
    rec.update(copy_GBps=round(2 * nbytes / m["copy"][0] / 1e6, 1), clahe_GBps=round(2 * nbytes / m["clahe"][0] / 1e6, 1),
               clahe_over_hist_plus_lut=round(m["clahe"][0] / base, 3), luts_over_histogram=round(m["luts"][0] / m["histogram"][0], 3),
               interp_over_lut=round(rec["interp_ms"] / m["lut"][0], 3), equalize_over_hist_plus_lut=round(m["equalize"][0] / base, 3),
               enhance_over_clahe_plus_equalize=round(m["enhance"][0] / (m["clahe"][0] + m["equalize"][0]), 3))
    if not args.no_check:
        j = n // 2 - 1
        prl.enhanceLocalContrast(pages, CLIP, True, out=out)
        rec["check"] = "ok" if np.array_equal(out[j].cpu().numpy(), clahe_ref.enhance(pages[j].cpu().numpy(), CLIP, True)) else "MISMATCH"
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--no-check", action="store_true")
    args = ap.parse_args()
    import torch

    import prlib_amd

    if not torch.cuda.is_available():
        sys.exit("bench_clahe.py needs a GPU")
    lines = []
    for name in [s for s in args.only.split(",") if s] or list(RUNS):
        rec = run(torch, prlib_amd, args, name, *RUNS[name])
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in lines) + "\n")


if __name__ == "__main__":
    main()
