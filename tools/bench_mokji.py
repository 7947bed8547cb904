#!/usr/bin/env python3
"""prl::binarizeMokji (mokji.hip) on device-resident pages: one JSON line per workload and stage.

    python tools/bench_mokji.py [--steps 10] [--warmup 3] [--repeats 5] [--only G,C] [--out FILE] [--no-check]

G   256 x A4 gray (2480 x 3508) at the defaults (maxEdgeWidth 3, minEdgeMagnitude 20)
C   64 x A4 x 3 channels at the defaults

Per workload one line for the whole call (`binarizeMokji`) and one per stage, each stage timed on its own through the entry that
runs it alone, between two device events on the current stream:
    dilate            the (2E + 1)^2 dilation of the gray pages (prl_hip_morphology_batch_device, the launch path the binarizer uses)
    cooc_M            k_mokji_cooc with min_diff = M on the gray and dilated pages (prl_hip_cooccurrence_batch_device; the memset of
                      the matrices included) - the kernel as the binarizer launches it
    cooc_0            the same with min_diff = 0: every pixel reaches an LDS atomic (the full matrix)
    thresholds        gray, dilation, matrix and threshold (prl_hip_mokji_thresholds_batch_device): everything but the compare
    binarizeMokji     the whole call; compare_by_difference_ms = this minus `thresholds`
ms: per repeat the median of `steps` calls after `warmup`; the line reports the median, the minimum and the maximum of the
`repeats` medians and their spread (max - min).  alg_bytes = 3 B per pixel for the whole call (the page is read for the statistics,
read again for the compare, and the mask is written: like Wolf-Jolion); the stage lines carry their own (dilate 2 B/px, cooc 2 B/px
read, thresholds 1 B/px).  frac_8TBps: those bytes over 8 TB/s; frac_copy: the same bytes at the rate of a device-to-device copy
of the gray batch measured in the same run (copy_ms, copy_GBps).
One page of each workload is checked against tests/mokji_ref.py, outside the timed window.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

A4 = dict(h=3508, w=2480)
E, M = 3, 20


def make_pages(torch, n, c, bases=4):
    """`bases` distinct text pages, repeated over the batch with a gain per page and a tint per channel"""
    from prlib_amd import synth

    base = torch.from_numpy(np.stack([synth.text_page_numpy(A4["h"], A4["w"], i, skew_deg=0.0, shading=0.15) for i in range(bases)])).cuda()
    pages = torch.empty((n, A4["h"], A4["w"]) + ((c,) if c > 1 else ()), dtype=torch.uint8, device="cuda")
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
    return dict(ms_median=round(float(np.median(meds)), 4), ms_min=round(min(meds), 4), ms_max=round(max(meds), 4),
                spread_ms=round(max(meds) - min(meds), 4))


def record(name, op, n, c, t, bytes_per_px, copy_gbps, copy_ms, args, **extra):
    px = n * A4["h"] * A4["w"]
    alg = bytes_per_px * px
    return dict(workload=name, op=op, pages=n, height=A4["h"], width=A4["w"], channels=c, max_edge_width=E, min_edge_magnitude=M,
                steps=args.steps, warmup=args.warmup, repeats=args.repeats, **t, bytes_per_px=bytes_per_px, alg_bytes=alg,
                mpix_per_s=round(px / t["ms_median"] / 1e3, 1), frac_8TBps=round(alg / t["ms_median"] / 1e9 / 8.0, 4),
                copy_ms=round(copy_ms, 4), copy_GBps=round(copy_gbps, 1), frac_copy=round(alg / t["ms_median"] / 1e6 / copy_gbps, 4), **extra)


def run(torch, prl, args, name, n, c):
    import mokji_ref
    from prlib_amd import morphology

    pages = make_pages(torch, n, c)
    gray = pages if c == 1 else prl.cvtColorBGR2GRAY(pages)
    out = torch.empty_like(gray)
    dil = torch.empty_like(gray)
    cooc = torch.empty((n, 256, 256), dtype=torch.int32, device="cuda")
    thr = torch.empty((n,), dtype=torch.int32, device="cuda")
    cp = timed(torch, lambda: dil.copy_(gray), args.steps, args.warmup, 1)
    gbps, cms = 2 * gray.numel() / cp["ms_median"] / 1e6, cp["ms_median"]
    k = 2 * E + 1
    prl.morphologyEx(gray, morphology.MORPH_DILATE, morphology.MORPH_RECT, (k, k), out=dil)
    stages = [("dilate", lambda: prl.morphologyEx(gray, morphology.MORPH_DILATE, morphology.MORPH_RECT, (k, k), out=dil), 2),
              ("cooc_M", lambda: prl.cooccurrence(gray, dil, E, M, out=cooc), 2),
              ("cooc_0", lambda: prl.cooccurrence(gray, dil, E, 0, out=cooc), 2),
              ("thresholds", lambda: prl.mokjiThresholds(pages, E, M, out=thr), 1),
              ("binarizeMokji", lambda: prl.binarizeMokji(pages, E, M, out=out), 3)]
    recs = []
    for op, call, bpp in stages:
        recs.append(record(name, op, n, c, timed(torch, call, args.steps, args.warmup, args.repeats), bpp, gbps, cms, args))
    recs[-1]["compare_by_difference_ms"] = round(recs[-1]["ms_median"] - recs[-2]["ms_median"], 4)
    if not args.no_check:
        j = n // 2 - 1
        prl.binarizeMokji(pages, E, M, out=out)
        prl.mokjiThresholds(pages, E, M, out=thr)
        want, t = mokji_ref.mokji(pages[j].cpu().numpy(), E, M)
        ok = np.array_equal(out[j].cpu().numpy(), want) and int(thr[j].cpu()) == t
        recs[-1]["check"] = "ok" if ok else "MISMATCH"
        recs[-1]["thresholds_seen"] = sorted(set(thr.cpu().tolist()))
    return recs


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
        sys.exit("bench_mokji.py needs a GPU")
    runs = {"G": (256, 1), "C": (64, 3)}
    lines = []
    for name in [s for s in args.only.split(",") if s] or list(runs):
        for rec in run(torch, prlib_amd, args, name, *runs[name]):
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in lines) + "\n")


if __name__ == "__main__":
    main()
