#!/usr/bin/env python3
"""The 8-bit cv::GaussianBlur (blur8.hip) and prl::binarizeLocalOtsu (localotsu.hip, edgedet.hip) on device-resident pages: one JSON
line per workload.

    python tools/bench_localotsu.py [--steps 10] [--warmup 3] [--repeats 5] [--call-steps 3] [--call-warmup 1] [--only G,C,L]
                                    [--pages-l 256] [--out FILE] [--no-check]

G   the blur at 19 x 19, sigma 0, on 256 x A4 gray (2480 x 3508)
C   the same on 64 x A4 x 3 channels
        blur_u8_ms     prl_hip_gaussian_blur_u8_batch_device
        blur_f32_ms    prl_hip_gaussian_blur_f32_batch_device at the same size on the same pages (4 bytes a sample out)
        copy_ms        a device-to-device copy of the batch (read + write)
L   prl_hip_binarize_local_otsu_batch_device with the header defaults on 256 x A4 synthetic text pages, and its stages one by one
    on the same pages:
        call_ms        the whole call (it waits for its stream: the host clock around it)
        clahe_ms       gray / CLAHE: EnhanceLocalContrastByCLAHE(2.0, equalize) - NOT part of the default call (clip limit 0), whose
                       gray page is the input itself; timed because a positive limit adds it
        edges_ms       CannyEdgeDetection(19, 0.15, 0.01, 1)
        dilate_ms      the 7 x 7 dilation (three iterations of 3 x 3)
        host_ms        the call's read-back and host stage BY DIFFERENCE: call_ms - edges_ms - dilate_ms - rects_ms (the call runs the
                       rectangles on the library's own thread pool from pinned memory; no entry runs that stage alone)
        host_py_ms     the same stage as this script can make it: a pageable read-back of the dilated maps and
                       prl_hip_external_rects of every page on 16 Python threads (the host clock); an upper bound, not the call's
        rects_ms       the upload of the rectangles and prl_hip_rect_otsu_batch_device
        rects_per_page the median, the smallest and the largest number of rectangles of a page
Device times: between two device events on the current stream.  ms: per repeat the median of `steps` calls after `warmup` (the
whole call and the host stage: --call-steps after --call-warmup); the line reports the median, the minimum and the maximum of the
`repeats` medians.  A window of one page of G and C, and one whole page of L at a reduced size, is checked against
tests/localotsu_ref.py outside the timed window.
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

RUNS = {"G": (256, 3508, 2480, 1), "C": (64, 3508, 2480, 3), "L": (256, 3508, 2480, 1)}
SIDE = 19


def host_timed(torch, call, steps, warmup, repeats):
    meds = []
    for _ in range(repeats):
        for _ in range(warmup):
            call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(steps):
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        meds.append(float(np.median(ms)))
    return round(float(np.median(meds)), 3), round(min(meds), 3), round(max(meds), 3)


def triple(rec, key, t):
    rec[key], rec[key + "_min"], rec[key + "_max"] = t


def run_blur(torch, prl, args, name, n, h, w, c):
    import localotsu_ref
    from bench_focus import make_pages, timed

    pages = make_pages(torch, n, h, w, c)
    out = torch.empty_like(pages)
    rec = dict(workload=name, pages=n, height=h, width=w, channels=c, kernel=SIDE, sigma=0.0, steps=args.steps, warmup=args.warmup,
               repeats=args.repeats)
    triple(rec, "blur_u8_ms", timed(torch, lambda: prl.gaussianBlurU8(pages, (SIDE, SIDE), out=out), args.steps, args.warmup, args.repeats))
    if not args.no_check:   # rows 0 .. 99 of a page depend on its rows 0 .. 108 only
        j = n // 2 - 1
        top = np.ascontiguousarray(pages[j, :100 + SIDE // 2].cpu().numpy())
        rec["check"] = "ok" if np.array_equal(out[j, :100].cpu().numpy(), localotsu_ref.blur_u8(top, (SIDE, SIDE))[:100]) else "MISMATCH"
    triple(rec, "copy_ms", timed(torch, lambda: out.copy_(pages), args.steps, args.warmup, args.repeats))
    del out
    plane = torch.empty(pages.shape, dtype=torch.float32, device="cuda")
    triple(rec, "blur_f32_ms", timed(torch, lambda: prl.gaussianBlurF32(pages, (SIDE, SIDE), 0.0, 0.0, out=plane), args.steps, args.warmup, args.repeats))
    samples = pages.numel()
    rec.update(u8_over_f32=round(rec["blur_u8_ms"] / rec["blur_f32_ms"], 3), u8_over_copy=round(rec["blur_u8_ms"] / rec["copy_ms"], 2),
               samples=samples, ns_per_sample=round(rec["blur_u8_ms"] * 1e6 / samples, 5), ms_per_page=round(rec["blur_u8_ms"] / n, 4))
    return rec


def run_call(torch, prl, args, name, n, h, w, c):
    import localotsu_ref
    from bench_focus import make_pages, timed
    from prlib_amd import morphology, synth

    n = args.pages_l or n
    pages = make_pages(torch, n, h, w, c)
    out = torch.empty_like(pages)
    rec = dict(workload=name, pages=n, height=h, width=w, channels=c, steps=args.steps, warmup=args.warmup, repeats=args.repeats,
               call_steps=args.call_steps, call_warmup=args.call_warmup)
    triple(rec, "call_ms", host_timed(torch, lambda: prl.binarizeLocalOtsu(pages, out=out), args.call_steps, args.call_warmup, args.repeats))
    # the stages, each on the result of the one before
    gray = torch.empty_like(pages)
    triple(rec, "clahe_ms", timed(torch, lambda: prl.enhanceLocalContrast(pages, 2.0, True, out=gray), args.steps, args.warmup, args.repeats))
    del gray
    edges = torch.empty_like(pages)
    triple(rec, "edges_ms", host_timed(torch, lambda: prl.cannyEdgeDetection(pages, out=edges), args.call_steps, args.call_warmup, args.repeats))
    dil = torch.empty_like(pages)
    triple(rec, "dilate_ms", timed(torch, lambda: prl.morphologyEx(edges, morphology.MORPH_DILATE, morphology.MORPH_RECT, (7, 7), out=dil),
                                    args.steps, args.warmup, args.repeats))
    del edges
    pool = ThreadPoolExecutor(16)
    found = {}

    def host_stage():
        maps = dil.cpu().numpy()
        found["rects"] = list(pool.map(lambda m: prl.externalRects(m)[0], maps))

    triple(rec, "host_py_ms", host_timed(torch, host_stage, args.call_steps, args.call_warmup, args.repeats))
    del dil
    rects = found["rects"]
    counts = [len(r) for r in rects]
    triple(rec, "rects_ms", timed(torch, lambda: prl.rectOtsu(pages, rects, 255.0, out=out), args.steps, args.warmup, args.repeats))
    device = rec["edges_ms"] + rec["dilate_ms"] + rec["rects_ms"]
    rec.update(rects_per_page=[int(np.median(counts)), min(counts), max(counts)], device_stages_ms=round(device, 3),
               host_ms=round(rec["call_ms"] - device, 3), ms_per_page=round(rec["call_ms"] / n, 4))
    if not args.no_check:
        small = synth.text_page_numpy(300, 400, 5)
        got = prl.binarizeLocalOtsu(torch.from_numpy(small).cuda()).cpu().numpy()
        ok = np.array_equal(got, localotsu_ref.binarize_local_otsu(small)[0])
        whole = prl.binarizeLocalOtsu(pages[:2]).cpu().numpy()
        ok = ok and np.array_equal(whole, prl.rectOtsu(pages[:2], rects[:2]).cpu().numpy())   # the stages give the call's masks
        rec["check"] = "ok" if ok else "MISMATCH"
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--call-steps", type=int, default=3)
    ap.add_argument("--call-warmup", type=int, default=1)
    ap.add_argument("--pages-l", type=int, default=0)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--no-check", action="store_true")
    args = ap.parse_args()
    import torch

    import prlib_amd

    if not torch.cuda.is_available():
        sys.exit("bench_localotsu.py needs a GPU")
    lines = []
    for name in [s for s in args.only.split(",") if s] or list(RUNS):
        rec = (run_call if name == "L" else run_blur)(torch, prlib_amd, args, name, *RUNS[name])
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in lines) + "\n")


if __name__ == "__main__":
    main()
