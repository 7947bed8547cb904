#!/usr/bin/env python3
"""prl::basicDeblur (deblur.hip: a float32 73 x 73 Gaussian and the unsharp mask, fused) on device-resident pages: one JSON line per
workload.

    python tools/bench_deblur.py [--steps 10] [--warmup 3] [--repeats 5] [--only G,C] [--out FILE] [--no-check]

G   256 x A4 gray (2480 x 3508)
C   64 x A4 x 3 channels

Per workload, in the same run, between two device events on the current stream:
    deblur_ms      prl_hip_basic_deblur_batch_device with the header defaults (kernel size 0, sigma 9: 73 x 73; weight 0.75)
    blur_f32_ms    prl_hip_gaussian_blur_f32_batch_device, the same kernel writing the float32 plane (4 bytes a sample)
    adaptive_ms    (gray only) prl_hip_adaptive_threshold_batch_device(GAUSSIAN_C, block 73) on the same pages: the in-tree yardstick
                   for a float32 separable Gaussian of the same length
    copy_ms        a device-to-device copy of the batch (read + write)
ms: per repeat the median of `steps` calls after `warmup`; the line reports the median, the minimum and the maximum of the
`repeats` medians.  deblur_over_adaptive and deblur_over_copy are ratios of the medians; ns_per_sample = deblur_ms over the batch's
samples; gflops counts 2 (73 + 73) + 4 float operations a sample (no fused multiply-add: the order of roundings is pinned).
A window of one page of each workload is checked against tests/deblur_ref.py, outside the timed window.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

RUNS = {"G": (256, 3508, 2480, 1), "C": (64, 3508, 2480, 3)}


def run(torch, prl, args, name, n, h, w, c):
    import deblur_ref
    from bench_focus import make_pages, timed

    pages = make_pages(torch, n, h, w, c)
    out = torch.empty_like(pages)
    f = timed(torch, lambda: prl.basicDeblur(pages, out=out), args.steps, args.warmup, args.repeats)
    rec = dict(workload=name, pages=n, height=h, width=w, channels=c, kernel=73, sigma=9.0, image_weight=0.75,
               steps=args.steps, warmup=args.warmup, repeats=args.repeats, deblur_ms=f[0], deblur_ms_min=f[1], deblur_ms_max=f[2])
    if not args.no_check:   # rows 0 .. 99 of a page depend on its rows 0 .. 135 only (reflection at the top, 36 rows below)
        j = n // 2 - 1
        top = pages[j, :136].cpu().numpy()
        rec["check"] = "ok" if np.array_equal(out[j, :100].cpu().numpy(), deblur_ref.deblur(np.ascontiguousarray(top))[:100]) else "MISMATCH"
    if c == 1:
        mask = torch.empty_like(pages)
        a = timed(torch, lambda: prl.adaptiveThreshold(pages, 255.0, 1, 0, 73, 5.0, out=mask), args.steps, args.warmup, args.repeats)
        rec.update(adaptive_ms=a[0], adaptive_ms_min=a[1], adaptive_ms_max=a[2], deblur_over_adaptive=round(f[0] / a[0], 3))
        del mask
    cp = timed(torch, lambda: out.copy_(pages), args.steps, args.warmup, args.repeats)
    del out
    plane = torch.empty(pages.shape, dtype=torch.float32, device="cuda")
    b = timed(torch, lambda: prl.gaussianBlurF32(pages, out=plane), args.steps, args.warmup, args.repeats)
    samples = pages.numel()
    rec.update(blur_f32_ms=b[0], blur_f32_ms_min=b[1], blur_f32_ms_max=b[2], copy_ms=cp[0], copy_ms_min=cp[1], copy_ms_max=cp[2],
               deblur_over_copy=round(f[0] / cp[0], 2), samples=samples, ns_per_sample=round(f[0] * 1e6 / samples, 5),
               ms_per_page=round(f[0] / n, 4), gflops=round(samples * (2 * 146 + 4) / f[0] / 1e6, 1))
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
        sys.exit("bench_deblur.py needs a GPU")
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
