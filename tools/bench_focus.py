#!/usr/bin/env python3
"""The focus sums (focus.hip: LAPM, LAPV, TENG, GLVN of blur detection) on device-resident pages: one JSON line per workload.

    python tools/bench_focus.py [--steps 10] [--warmup 3] [--repeats 5] [--only G,C,K] [--out FILE] [--no-check]

G   256 x A4 gray (2480 x 3508)
C   64 x A4 x 3 channels
K   256 x 4096 x 4096 gray

Per workload, in the same run, between two device events on the current stream:
    focus_ms       prl_hip_focus_sums_batch_device (the memset of the result included), Sobel size 3
    histogram_ms   prl_hip_histogram_batch_device on the same pages: the library's other read-only reduction
    copy_ms        a device-to-device copy of the batch (read + write); read_ceiling_ms = copy_ms / 2, the time the batch's bytes
                   take at the copy's rate when they are only read
ms: per repeat the median of `steps` calls after `warmup`; the line reports the median, the minimum and the maximum of the
`repeats` medians.  focus_over_histogram and focus_over_read_ceiling are ratios of the medians; GBps = the batch's bytes over
focus_ms.
One page of each workload is checked against tests/focus_ref.py, outside the timed window.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RUNS = {"G": (256, 3508, 2480, 1), "C": (64, 3508, 2480, 3), "K": (256, 4096, 4096, 1)}


def make_pages(torch, n, h, w, c, bases=2):
    """`bases` distinct text pages, repeated over the batch with a gain per page and a tint per channel"""
    from prlib_amd import synth

    base = torch.from_numpy(np.stack([synth.text_page_numpy(h, w, i, skew_deg=0.0, shading=0.15) for i in range(bases)])).cuda()
    pages = torch.empty((n, h, w) + ((c,) if c > 1 else ()), dtype=torch.uint8, device="cuda")
    for i in range(n):
        g = (base[i % bases].to(torch.float32) * (0.75 + 0.25 * ((i * 7) % 11) / 10.0)).to(torch.uint8)
        if c > 1:
            for ch in range(c):
                pages[i, :, :, ch] = torch.clamp(g.to(torch.int16) + (ch - 1) * 9, 0, 255).to(torch.uint8)
        else:
            pages[i] = g
    return pages


def timed(torch, call, steps, warmup, repeats):
    meds = []
    for _ in range(repeats):
        for _ in range(warmup):
            call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        meds.append(float(np.median(ms)))
    return round(float(np.median(meds)), 4), round(min(meds), 4), round(max(meds), 4)


def run(torch, prl, args, name, n, h, w, c):
    import focus_ref

    pages = make_pages(torch, n, h, w, c)
    sums = torch.empty((n, c, 6) if c > 1 else (n, 6), dtype=torch.int64, device="cuda")
    hist = torch.empty((n, c, 256), dtype=torch.int32, device="cuda")
    other = torch.empty_like(pages)
    f = timed(torch, lambda: prl.focusSums(pages, 3, out=sums), args.steps, args.warmup, args.repeats)
    g = timed(torch, lambda: prl.histogram(pages, out=hist), args.steps, args.warmup, args.repeats)
    cp = timed(torch, lambda: other.copy_(pages), args.steps, args.warmup, args.repeats)
    nbytes = pages.numel()
    rec = dict(workload=name, pages=n, height=h, width=w, channels=c, teng_ksize=3,
               steps=args.steps, warmup=args.warmup, repeats=args.repeats, focus_ms=f[0], focus_ms_min=f[1], focus_ms_max=f[2],
               histogram_ms=g[0], histogram_ms_min=g[1], histogram_ms_max=g[2], copy_ms=cp[0], copy_ms_min=cp[1], copy_ms_max=cp[2],
               copy_GBps=round(2 * nbytes / cp[0] / 1e6, 1), read_ceiling_ms=round(cp[0] / 2, 4), bytes=nbytes,
               GBps=round(nbytes / f[0] / 1e6, 1), mpix_per_s=round(n * h * w / f[0] / 1e3, 1),
               focus_over_histogram=round(f[0] / g[0], 3), focus_over_read_ceiling=round(f[0] / (cp[0] / 2), 3))
    if not args.no_check:
        j = n // 2 - 1
        prl.focusSums(pages, 3, out=sums)
        rec["check"] = "ok" if np.array_equal(sums[j].cpu().numpy(), focus_ref.sums(pages[j].cpu().numpy(), 3)) else "MISMATCH"
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
        sys.exit("bench_focus.py needs a GPU")
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
