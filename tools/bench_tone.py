#!/usr/bin/env python3
"""The tone functions (tone.hip) on device-resident pages: one JSON line per workload.

    python tools/bench_tone.py [--steps 10] [--warmup 3] [--repeats 5] [--only G,C,H] [--out FILE] [--no-check]

G   256 x A4 gray (2480 x 3508) through cleanBackgroundToWhite
C   64 x A4 x 3 channels through gammaCorrection, simpleWhiteBalance, grayWorldWhiteBalance (pNorm 1 on the device, and 2.5
    through the host tables: that call synchronises the stream) and cleanBackgroundToWhite: one line each
H   the histogram kernel alone on 64 x A4 x 3 channels: a page of one value (every wavefront takes the uniform shortcut, and every
    workgroup adds to the same three bins) against a uniform-noise page; flat_to_noise is the ratio of the two medians

ms: per repeat the median of `steps` calls after `warmup`, each between two device events on the current stream; the line
reports the median, the minimum and the maximum of the `repeats` medians and their spread (max - min).  passes: how often the
call walks the page (histogram, normalisation's two reads, look-up ...); alg_bytes = 2 B per pixel byte and pass (read + write
of the page; a histogram pass only reads, so this is an upper estimate of its traffic); frac_8TBps: those bytes over 8 TB/s;
frac_copy: the same bytes at the rate of a device-to-device copy of the batch measured in the same run.
One page of each workload is checked against tests/tone_ref.py, outside the timed window.
Kernel times and counters: run this under rocprofv3 separately (--kernel-trace --stats; --pmc in a run of its own).
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


def copy_rate(torch, pages, args):
    dup = torch.empty_like(pages)
    cp = timed(torch, lambda: dup.copy_(pages), args.steps, args.warmup, 1)
    del dup
    return 2 * pages.numel() / cp["ms_median"] / 1e6, cp["ms_median"]   # GB/s


def record(name, op, pages, t, passes, copy_gbps, copy_ms, args, **extra):
    alg = 2 * pages.numel() * passes
    return dict(workload=name, op=op, pages=pages.shape[0], height=A4["h"], width=A4["w"], channels=pages.shape[3] if pages.dim() == 4 else 1,
                steps=args.steps, warmup=args.warmup, repeats=args.repeats, **t, passes=passes, alg_bytes=alg,
                mpix_per_s=round(pages.shape[0] * A4["h"] * A4["w"] / t["ms_median"] / 1e3, 1),
                frac_8TBps=round(alg / t["ms_median"] / 1e9 / 8.0, 4), copy_ms=round(copy_ms, 4), copy_GBps=round(copy_gbps, 1),
                frac_copy=round(alg / t["ms_median"] / 1e6 / copy_gbps, 4), **extra)


def run_g(torch, prl, args):
    import tone_ref
    from oracle import capi as oracle

    pages = make_pages(torch, 256, 1)
    out = torch.empty_like(pages)
    gbps, cms = copy_rate(torch, pages, args)
    t = timed(torch, lambda: prl.cleanBackgroundToWhite(pages, out=out), args.steps, args.warmup, args.repeats)
    rec = record("G", "cleanBackgroundToWhite", pages, t, 3, gbps, cms, args)   # tiles read, apply read + write, look-up read + write
    if not args.no_check:
        j = 127
        rec["check"] = "ok" if np.array_equal(out[j].cpu().numpy(), tone_ref.clean_background(oracle, pages[j].cpu().numpy())) else "MISMATCH"
    return [rec]


def run_c(torch, prl, args):
    import tone_ref
    from oracle import capi as oracle

    pages = make_pages(torch, 64, 3)
    out = torch.empty_like(pages)
    gbps, cms = copy_rate(torch, pages, args)
    j = 31
    ops = [("gammaCorrection", lambda: prl.gammaCorrection(pages, 0.9, 2.2, out=out), 1, lambda p: tone_ref.gamma_model(p, 0.9, 2.2)),
           ("simpleWhiteBalance", lambda: prl.simpleWhiteBalance(pages, 0.01, out=out), 1.5, lambda p: tone_ref.swb_model(p, 0.01)),
           ("grayWorldWhiteBalance_p1", lambda: prl.grayWorldWhiteBalance(pages, 1.0, False, out=out), 1.5,
            lambda p: tone_ref.gw_model(p, 1.0, False)),
           ("grayWorldWhiteBalance_p2.5_host_tables", lambda: prl.grayWorldWhiteBalance(pages, 2.5, False, out=out), 1.5,
            lambda p: tone_ref.gw_model(p, 2.5, False)),
           ("cleanBackgroundToWhite", lambda: prl.cleanBackgroundToWhite(pages, out=out), 3, lambda p: tone_ref.clean_background(oracle, p))]
    recs = []
    for op, call, passes, want in ops:   # passes: a histogram pass reads only: half a pass of 2 B per byte
        t = timed(torch, call, args.steps, args.warmup, args.repeats)
        rec = record("C", op, pages, t, passes, gbps, cms, args)
        if not args.no_check:
            call()
            rec["check"] = "ok" if np.array_equal(out[j].cpu().numpy(), want(pages[j].cpu().numpy())) else "MISMATCH"
        recs.append(rec)
    return recs


def run_h(torch, prl, args):
    n = 64
    flat = torch.full((n, A4["h"], A4["w"], 3), 233, dtype=torch.uint8, device="cuda")
    noise = torch.randint(0, 256, (n, A4["h"], A4["w"], 3), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    hist = torch.empty((n, 3, 256), dtype=torch.int32, device="cuda")
    gbps, cms = copy_rate(torch, noise, args)
    recs = []
    for op, pages in (("histogram_flat", flat), ("histogram_noise", noise)):
        t = timed(torch, lambda: prl.histogram(pages, out=hist), args.steps, args.warmup, args.repeats)
        rec = record("H", op, pages, t, 0.5, gbps, cms, args)
        if not args.no_check:
            got = hist[5].cpu().numpy()
            want = np.stack([np.bincount(pages[5, :, :, c].cpu().numpy().ravel(), minlength=256) for c in range(3)])
            rec["check"] = "ok" if np.array_equal(got, want) else "MISMATCH"
        recs.append(rec)
    ratio = round(recs[0]["ms_median"] / recs[1]["ms_median"], 3)
    for r in recs:
        r["flat_to_noise"] = ratio
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
        sys.exit("bench_tone.py needs a GPU")
    runs = {"G": run_g, "C": run_c, "H": run_h}
    lines = []
    for name in [s for s in args.only.split(",") if s] or list(runs):
        for rec in runs[name](torch, prlib_amd, args):
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in lines) + "\n")


if __name__ == "__main__":
    main()
