#!/usr/bin/env python3
"""The adaptive-threshold binarizers on device-resident pages: one JSON line per workload.

    python tools/bench_adaptive.py [--steps 10] [--warmup 3] [--only T1,N1] [--out FILE] [--no-check]

T1  256 x A4 gray (2480 x 3508), cv::adaptiveThreshold MEAN_C, block 19        T2  the same, GAUSSIAN_C, block 19
T3  the same, GAUSSIAN_C, block 101
N1  prl::binarizeNativeAdaptive, header defaults, 256 x A4 gray                 N2  the same on 64 x A4 colour
A1  prl::binarizeAT(5, 255, 19, 9) on 64 x A4 colour

ms per call: `steps` calls after `warmup`, host clock closed by a device synchronise.  T1-T3 also report the share of
8 TB/s at 2 B per pixel (read + write) and the share of a device copy (torch copy_ of 2 GiB) measured in the same run.
N1 and N2 time their stages separately in the same run - BGR -> gray, the median at k = 5, the bare threshold with
auto-invert - and report the sum next to the composed call (the composition adds no host round trip).  One page of each
workload is checked against the restatement of tests/adaptive_ref.py outside the timed window.
Kernel times: run this under `rocprofv3 --kernel-trace --stats` separately.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

A4 = dict(h=3508, w=2480)
WORKLOADS = {
    "T1": dict(kind="threshold", n=256, c=1, method=0, bs=19),
    "T2": dict(kind="threshold", n=256, c=1, method=1, bs=19),
    "T3": dict(kind="threshold", n=256, c=1, method=1, bs=101),
    "N1": dict(kind="native", n=256, c=1),
    "N2": dict(kind="native", n=64, c=3),
    "A1": dict(kind="at", n=64, c=3),
}


def timed(torch, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--no-check", action="store_true")
    args = ap.parse_args()
    import torch

    import adaptive_ref as ar
    import prlib_amd as prl
    from bench_median import copy_ceiling, make_pages

    if not torch.cuda.is_available():
        sys.exit("bench_adaptive.py needs a GPU")
    ceiling = copy_ceiling(torch)
    names = [s for s in args.only.split(",") if s] or list(WORKLOADS)
    lines = []
    h, w = A4["h"], A4["w"]
    for i, name in enumerate(names):
        p = WORKLOADS[name]
        n, c = p["n"], p["c"]
        pages = make_pages(torch, n, h, w, c, 11 + i)
        if c == 1:
            pages = pages[..., 0]
        out = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
        px = n * h * w
        rec = dict(workload=name, kind=p["kind"], pages=n, height=h, width=w, channels=c, steps=args.steps, warmup=args.warmup)
        if p["kind"] == "threshold":
            call = lambda: prl.adaptiveThreshold(pages, 255.0, p["method"], ar.BINARY_INV, p["bs"], 9.0, out=out)   # noqa: E731
            want = lambda src: ar.adaptive_threshold(src, 255.0, p["method"], ar.BINARY_INV, p["bs"], 9.0)            # noqa: E731
            rec.update(method="GAUSSIAN_C" if p["method"] else "MEAN_C", block=p["bs"])
        elif p["kind"] == "native":
            call = lambda: prl.binarizeNativeAdaptive(pages, out=out)   # noqa: E731
            want = ar.binarize_native_adaptive
        else:
            call = lambda: prl.binarizeAT(pages, 5, 255, 19, 9, out=out)   # noqa: E731
            want = lambda src: ar.binarize_at(src, 5, 255, 19, 9)          # noqa: E731
        ms = timed(torch, call, args.steps, args.warmup)
        rec.update(ms_per_call=round(ms, 4), mpix_per_s=round(px / ms / 1e3, 1))
        if p["kind"] == "threshold":
            alg = 2 * px
            rec.update(alg_bytes=alg, alg_TBps=round(alg / ms / 1e9, 3), frac_8TBps=round(alg / ms / 1e9 / 8.0, 3),
                       copy_ceiling_TBps=round(ceiling / 1e12, 3), frac_copy_ceiling=round(alg / (ms * 1e-3) / ceiling, 3))
        if not args.no_check:
            j = n // 2
            rec["check"] = "ok" if np.array_equal(out[j].cpu().numpy(), want(pages[j].cpu().numpy())) else "MISMATCH"
        if p["kind"] == "native":   # the stages, one by one, on the same pages
            stages = {}
            gray = pages
            if c > 1:
                gray = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
                stages["bgr2gray_ms"] = round(timed(torch, lambda: prl.cvtColorBGR2GRAY(pages, out=gray), args.steps, args.warmup), 4)
            med = torch.empty_like(gray)
            stages["median5_ms"] = round(timed(torch, lambda: prl.denoiseSaltPepper(gray, 5, 1, out=med), args.steps, args.warmup), 4)
            stages["threshold_auto_invert_ms"] = round(timed(
                torch, lambda: prl.adaptiveThreshold(med, 255.0, ar.GAUSSIAN_C, ar.BINARY_INV, 19, 9.0, autoInvert=True, out=out),
                args.steps, args.warmup), 4)
            rec["stages"] = stages
            rec["sum_of_stages_ms"] = round(sum(stages.values()), 4)
            rec["composed_over_sum"] = round(ms / sum(stages.values()), 4)
            del med, gray
        del pages, out
        torch.cuda.empty_cache()
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
