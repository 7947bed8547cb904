#!/usr/bin/env python3
"""cv::pyrDown, cv::Canny, the edge map of prl::documentContour and prl::resize (pyr.hip, canny.hip, border.hip) on device-resident pages:
one JSON line per case.

    python tools/bench_edges.py [--steps 5] [--warmup 2] [--repeats 5] [--only P1,P2,C1,C2,D1,R1] [--out FILE] [--no-check]

P1  256 x A4 gray (2480 x 3508)           one pyramid level
P2  64 x A4 x 3 channels                  one pyramid level
C1  256 x A4 gray synthetic text          canny(25, 50)
C2  the same pages                        the two stage entries on their own: canny_classes (byte class map) and edge_link (pack,
                                          linking passes, expand) with the largest pass count of the batch
D1  256 x A4 x 3 channels                 document_edges
R1  64 x A4 x 3 channels                  resize with maxSize = 1024 (two pyramid levels)

Every case is timed in the same run, between two device events on the current stream, beside a device-to-device copy of its
own source buffer.  ms: per repeat the median of `steps` calls after `warmup`; the line reports the median, the minimum and the
maximum of the `repeats` medians and their spread (max - min).  alg_bytes: 1 1/4 B per source pixel and channel for a pyramid
level (1 read, 1/4 written), 2 B per pixel for Canny (1 read, 1 written); frac_8TBps: alg_bytes over the time at 8 TB/s;
frac_copy: alg_bytes at the copy's measured rate over the time.  One page of each case is checked against tests/edges_ref.py
outside the timed window.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W = 3508, 2480


def make_pages(torch, n, c, bases=4):
    """`bases` distinct text pages, repeated over the batch with a gain per page and a tint per channel"""
    from prlib_amd import synth

    base = torch.from_numpy(np.stack([synth.text_page_numpy(H, W, i, skew_deg=0.0, shading=0.15) for i in range(bases)])).cuda()
    pages = torch.empty((n, H, W) + ((c,) if c > 1 else ()), dtype=torch.uint8, device="cuda")
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default="P1,P2,C1,C2,D1,R1")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-check", action="store_true")
    args = ap.parse_args()
    import torch

    import edges_ref as er
    import prlib_amd as prl

    only = args.only.split(",")
    lines = []
    cache = {}

    def pages_of(n, c):
        if (n, c) not in cache:
            cache.clear()
            torch.cuda.empty_cache()
            cache[(n, c)] = make_pages(torch, n, c)
        return cache[(n, c)]

    def report(case, op, pages, t, alg, extra=None):
        cdst = torch.empty_like(pages)
        t_copy = timed(torch, lambda: cdst.copy_(pages), args.steps, args.warmup, args.repeats)
        del cdst
        copy_gbps = 2 * pages.numel() / t_copy["ms_median"] / 1e6
        gbps = alg / t["ms_median"] / 1e6
        lines.append(dict(case=case, op=op, pages=pages.shape[0], height=H, width=W, channels=pages.shape[3] if pages.dim() == 4 else 1,
                          steps=args.steps, warmup=args.warmup, repeats=args.repeats, **t, alg_bytes=int(alg), GBps=round(gbps, 1),
                          frac_8TBps=round(gbps / 8000.0, 4), copy_ms=t_copy["ms_median"], copy_GBps=round(copy_gbps, 1),
                          frac_copy=round(gbps / copy_gbps, 4), **(extra or {})))
        print(json.dumps(lines[-1]), flush=True)

    def check(got, want, what):
        assert args.no_check or np.array_equal(got.cpu().numpy(), want), what + " differs from tests/edges_ref.py"

    for case, n, c in (("P1", 256, 1), ("P2", 64, 3)):
        if case in only:
            pages = pages_of(n, c)
            out = prl.pyr_down(pages)
            if not args.no_check:
                check(out[n - 1], er.pyr_down(pages[n - 1].cpu().numpy()), "pyr_down")
            t = timed(torch, lambda: prl.pyr_down(pages, 1, out=out), args.steps, args.warmup, args.repeats)
            report(case, "pyr_down", pages, t, 1.25 * pages.numel())
            del out
    if "C1" in only or "C2" in only:
        pages = pages_of(256, 1)
        out = torch.empty_like(pages)
        if not args.no_check:
            prl.canny(pages[:2], 25, 50, out=out[:2])
            check(out[1], er.canny(pages[1].cpu().numpy(), 25, 50), "canny")
        if "C1" in only:
            t = timed(torch, lambda: prl.canny(pages, 25, 50, out=out), args.steps, args.warmup, args.repeats)
            report("C1", "canny", pages, t, 2.0 * pages.numel())
        if "C2" in only:
            cls = torch.empty_like(pages)
            t = timed(torch, lambda: prl.canny_classes(pages, 25, 50, out=cls), args.steps, args.warmup, args.repeats)
            report("C2", "canny_classes", pages, t, 2.0 * pages.numel())
            passes = prl.edge_link(cls, out=out, return_passes=True)[1]
            t = timed(torch, lambda: prl.edge_link(cls, out=out), args.steps, args.warmup, args.repeats)
            report("C2", "edge_link", pages, t, 2.0 * pages.numel(), dict(link_passes_max=int(passes.max()), link_passes_min=int(passes.min())))
            del cls
        del out
    if "D1" in only:
        pages = pages_of(256, 3)
        maps, chosen = prl.document_edges(pages)
        if not args.no_check:
            want, ch = er.document_edges(pages[255].cpu().numpy())
            assert int(chosen[255]) == ch
            check(maps[255], want, "document_edges")
        t = timed(torch, lambda: prl.document_edges(pages, out=maps), args.steps, args.warmup, args.repeats)
        levels, ow, oh = prl.document_edges_geometry(W, H)
        alg = sum(1.25 * pages.numel() / 4 ** k for k in range(levels)) + 256 * ow * oh * (3 + 3 + 1 + 2)   # levels, bins, channel, Canny
        report("D1", "document_edges", pages, t, alg, dict(levels=levels, out_w=ow, out_h=oh))
        del maps
    if "R1" in only:
        pages = pages_of(64, 3)
        out = prl.resize(pages, 0, 0, 1024)
        if not args.no_check:
            check(out[63], er.resize(pages[63].cpu().numpy(), 0, 0, 1024), "resize")
        t = timed(torch, lambda: prl.resize(pages, 0, 0, 1024, out=out), args.steps, args.warmup, args.repeats)
        levels = prl.resize_pyramid_levels(W, H, 1024)[0]
        report("R1", "resize_max1024", pages, t, sum(1.25 * pages.numel() / 4 ** k for k in range(levels)), dict(levels=levels))
    if args.out:
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
