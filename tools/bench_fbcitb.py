#!/usr/bin/env python3
"""cv::bilateralFilter (bilateral.hip), the ordered paint and prl::binarizeFBCITB (fbcitb.hip) on device-resident pages: one JSON line
per workload.

    python tools/bench_fbcitb.py [--steps 10] [--warmup 3] [--repeats 5] [--call-steps 3] [--call-warmup 1] [--only G,C,P,F,K]
                                 [--pages 0] [--out FILE] [--no-check]

G   the bilateral filter on 256 x A4 gray (2480 x 3508), sigmas 150 / 150
C   the same on 64 x A4 x 3 channels
        bilateral_d5_ms, bilateral_d9_ms   prl_hip_bilateral_filter_batch_device at d = 5 (12 taps) and d = 9 (48 taps)
        median5_ms                         prl_hip_median_batch_device at k = 5 on the same pages (one pass)
        blur_u8_5_ms, blur_u8_9_ms         prl_hip_gaussian_blur_u8_batch_device at the same sides
        copy_ms                            a device-to-device copy of the batch (read + write)
P   the ordered paint on 256 x A4 gray with every page's rectangles from the whole call's own contour stage:
        paint_ms       prl_hip_rect_paint_batch_device
        rect_otsu_ms   prl_hip_rect_otsu_batch_device on the same rectangles (its paint stores 0 only and needs no order)
F   prl_hip_binarize_fbcitb_batch_device on 256 x A4 gray text pages, variance mask + Canny on it (useCanny = false: the mode that
    keeps contours on text), and its stages one by one on the same pages:
K   the same on 64 x A4 colour pages
        call_ms        the whole call (it waits for its stream: the host clock around it)
        clahe_ms, bilateral_ms, variance_ms, canny_ms, gray_ms (colour), paint_ms, morph_ms    the stage entries
        host_ms        the read-back, the contours on the host pool and the upload BY DIFFERENCE: call_ms minus the stages above
Device times: between two device events on the current stream.  ms: per repeat the median of `steps` calls after `warmup` (the whole
call: --call-steps after --call-warmup); the line reports the median, the minimum and the maximum of the `repeats` medians.  A window
of one page of G and C and a reduced page of F are checked against tests/fbcitb_ref.py outside the timed window.
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

RUNS = {"G": (256, 3508, 2480, 1), "C": (64, 3508, 2480, 3), "P": (256, 3508, 2480, 1), "F": (256, 3508, 2480, 1), "K": (64, 3508, 2480, 3)}


def triple(rec, key, t):
    rec[key], rec[key + "_min"], rec[key + "_max"] = t


def run_filter(torch, prl, args, name, n, h, w, c):
    import fbcitb_ref
    from bench_focus import make_pages, timed

    n = args.pages or n
    pages = make_pages(torch, n, h, w, c)
    out = torch.empty_like(pages)
    rec = dict(workload=name, pages=n, height=h, width=w, channels=c, steps=args.steps, warmup=args.warmup, repeats=args.repeats)
    t = lambda call: timed(torch, call, args.steps, args.warmup, args.repeats)   # noqa: E731
    triple(rec, "bilateral_d9_ms", t(lambda: prl.bilateralFilter(pages, 9, 150.0, 150.0, out=out)))
    triple(rec, "bilateral_d5_ms", t(lambda: prl.bilateralFilter(pages, 5, 150.0, 150.0, out=out)))
    if not args.no_check:   # rows 0 .. 39 of a page depend on its rows 0 .. 41 only
        j = n // 2 - 1
        top = np.ascontiguousarray(pages[j, :42, :300].cpu().numpy())
        want = fbcitb_ref.bilateral(top, 5, 150.0, 150.0)[:40, :298]
        rec["check"] = "ok" if np.array_equal(out[j, :40, :298].cpu().numpy(), want) else "MISMATCH"
    triple(rec, "median5_ms", t(lambda: prl.denoiseSaltPepper(pages, 5, 1, out=out)))
    triple(rec, "blur_u8_5_ms", t(lambda: prl.gaussianBlurU8(pages, (5, 5), out=out)))
    triple(rec, "blur_u8_9_ms", t(lambda: prl.gaussianBlurU8(pages, (9, 9), out=out)))
    triple(rec, "copy_ms", t(lambda: out.copy_(pages)))
    px = pages.numel()
    rec.update(d5_over_median5=round(rec["bilateral_d5_ms"] / rec["median5_ms"], 3), d5_over_blur5=round(rec["bilateral_d5_ms"] / rec["blur_u8_5_ms"], 3),
               d9_over_blur9=round(rec["bilateral_d9_ms"] / rec["blur_u8_9_ms"], 3), d5_over_copy=round(rec["bilateral_d5_ms"] / rec["copy_ms"], 2),
               samples=px, d5_ns_per_tap_sample=round(rec["bilateral_d5_ms"] * 1e6 / (px * 12), 6),
               d9_ns_per_tap_sample=round(rec["bilateral_d9_ms"] * 1e6 / (px * 48), 6))
    return rec


def page_rects(torch, prl, pages):
    """every page's kept contours as the whole call's host stage finds them (variance mask + Canny on it)"""
    from concurrent.futures import ThreadPoolExecutor

    cmap = prl.canny(prl.varianceMask(pages, 200.0), 64.0, 128.0).cpu().numpy()
    proc = prl.bilateralFilter(prl.enhanceLocalContrast(pages, 2.0, False), 5, 150.0, 150.0)
    gray = (prl.cvtColorBGR2GRAY(proc) if proc.dim() == 4 else proc).cpu().numpy()
    with ThreadPoolExecutor(16) as pool:
        return list(pool.map(lambda i: prl.fbcitbContours(cmap[i], gray[i])[0], range(len(gray))))


def run_paint(torch, prl, args, name, n, h, w, c):
    from bench_focus import make_pages, timed

    n = args.pages or n
    pages = make_pages(torch, n, h, w, c)
    out = torch.empty_like(pages)
    rects = page_rects(torch, prl, pages)
    counts = [len(r) for r in rects]
    rec = dict(workload=name, pages=n, height=h, width=w, steps=args.steps, warmup=args.warmup, repeats=args.repeats,
               rects_per_page=[int(np.median(counts)), min(counts), max(counts)])
    triple(rec, "paint_ms", timed(torch, lambda: prl.rectPaint(pages, rects, out=out), args.steps, args.warmup, args.repeats))
    four = [r[:, :4] for r in rects]
    triple(rec, "rect_otsu_ms", timed(torch, lambda: prl.rectOtsu(pages, four, 255.0, out=out), args.steps, args.warmup, args.repeats))
    rec["paint_over_rect_otsu"] = round(rec["paint_ms"] / rec["rect_otsu_ms"], 3)
    return rec


def run_call(torch, prl, args, name, n, h, w, c):
    import fbcitb_ref
    from bench_focus import make_pages, timed
    from bench_localotsu import host_timed
    from prlib_amd import morphology, synth

    n = args.pages or n
    pages = make_pages(torch, n, h, w, c)
    out = torch.empty(pages.shape[:3], dtype=torch.uint8, device="cuda")
    rec = dict(workload=name, pages=n, height=h, width=w, channels=c, steps=args.steps, warmup=args.warmup, repeats=args.repeats,
               call_steps=args.call_steps, call_warmup=args.call_warmup, mode="variance mask + Canny on it")
    counts = {}

    def call():
        counts["c"] = prl.binarizeFBCITB(pages, False, True, out=out, with_counts=True)[1]

    triple(rec, "call_ms", host_timed(torch, call, args.call_steps, args.call_warmup, args.repeats))
    t = lambda f: timed(torch, f, args.steps, args.warmup, args.repeats)   # noqa: E731
    proc, filt = torch.empty_like(pages), torch.empty_like(pages)
    triple(rec, "clahe_ms", t(lambda: prl.enhanceLocalContrast(pages, 2.0, False, out=proc)))
    triple(rec, "bilateral_ms", t(lambda: prl.bilateralFilter(proc, 5, 150.0, 150.0, out=filt)))
    del proc
    mask, edges = torch.empty_like(out), torch.empty_like(out)
    triple(rec, "variance_ms", t(lambda: prl.varianceMask(pages, 200.0, out=mask)))
    triple(rec, "canny_ms", host_timed(torch, lambda: prl.canny(mask, 64.0, 128.0, out=edges), args.call_steps, args.call_warmup, args.repeats))
    stages = ["clahe_ms", "bilateral_ms", "variance_ms", "canny_ms", "paint_ms", "morph_ms"]
    gray = filt
    if c > 1:
        gray = torch.empty_like(out)
        triple(rec, "gray_ms", t(lambda: prl.cvtColorBGR2GRAY(filt, out=gray)))
        stages.append("gray_ms")
    del mask, edges
    rects = page_rects(torch, prl, pages)
    painted = torch.empty_like(out)
    triple(rec, "paint_ms", t(lambda: prl.rectPaint(gray, rects, out=painted)))
    triple(rec, "morph_ms", t(lambda: prl.morphologyEx(painted, morphology.MORPH_CLOSE, morphology.MORPH_RECT, (5, 5), out=out)))
    device = sum(rec[k] for k in stages)
    kept = np.asarray(counts["c"])[:, 2]
    rec.update(device_stages_ms=round(device, 3), host_ms=round(rec["call_ms"] - device, 3), ms_per_page=round(rec["call_ms"] / n, 4),
               kept_per_page=[int(np.median(kept)), int(kept.min()), int(kept.max())])
    if not args.no_check:
        small = synth.text_page_numpy(300, 400, 5)
        got = prl.binarizeFBCITB(torch.from_numpy(small).cuda(), False, True).cpu().numpy()
        rec["check"] = "ok" if np.array_equal(got, fbcitb_ref.binarize_fbcitb(small, False, True)[0]) else "MISMATCH"
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--call-steps", type=int, default=3)
    ap.add_argument("--call-warmup", type=int, default=1)
    ap.add_argument("--pages", type=int, default=0)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--no-check", action="store_true")
    args = ap.parse_args()
    import torch

    import prlib_amd

    if not torch.cuda.is_available():
        sys.exit("bench_fbcitb.py needs a GPU")
    lines = []
    for name in [s for s in args.only.split(",") if s] or list(RUNS):
        fn = run_filter if name in "GC" else run_paint if name == "P" else run_call
        rec = fn(torch, prlib_amd, args, name, *RUNS[name])
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        torch.cuda.empty_cache()
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(json.dumps(r) for r in lines) + "\n")


if __name__ == "__main__":
    main()
