#!/usr/bin/env python3
"""prl::removeLines on device-resident pages: one JSON line per workload.

    python tools/bench_lines.py [--steps 10] [--warmup 3] [--repeats 5] [--only G,C,W] [--out FILE] [--no-check]

G   256 x A4 gray (2480 x 3508: L = 49, Lv = 70), synth.text_page_numpy pages with ruled lines added
C   64 x A4 x 3 channels
W   16 pages of 13000 x 4000 (L = 260: a size the byte path cannot do)

ms: per repeat the median of `steps` calls after `warmup`, each between two device events on the current stream; the line
reports the median, the minimum and the maximum of the `repeats` medians and their spread (max - min).  Algorithmic bytes: gray
2 B per pixel (read + write once), colour 3 B read + 1 B write; frac_8TBps: those bytes over 8 TB/s; frac_copy: the same bytes
at the rate of a device-to-device copy of the batch measured in the same run.
G also times, in the same run, the morphological part composed from the byte path's public entries on a fixed-threshold byte
mask (pages < 128; the span kernel's time does not depend on the data): two prl_hip_morphology_batch_device(OPEN, RECT, ...)
calls (49 x 1 and 1 x 70).  `beats_byte_openings` is true when the whole
removeLines call (histogram, threshold, mask, both openings, expand) takes less than those two calls alone by more than the
larger of the two spreads.
One page of each workload is checked against the restatement of tests/lines_ref.py, outside the timed window.
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

WORKLOADS = {
    "G": dict(n=256, c=1, h=3508, w=2480, bases=4),
    "C": dict(n=64, c=3, h=3508, w=2480, bases=4),
    "W": dict(n=16, c=1, h=4000, w=13000, bases=2),
}


def ruled_page(h, w, index):
    """a text page with a table grid and a form box drawn over it"""
    from prlib_amd import synth

    page = synth.text_page_numpy(h, w, index, skew_deg=0.0, shading=0.15)
    for y in range(h // 8, h - h // 10, h // 9):
        page[y:y + 3, w // 12:w - w // 12] = 40
    for x in range(w // 12, w - w // 12 + 1, (w - w // 6) // 5):
        page[h // 8:h - h // 10, x:x + 3] = 40
    return page


def make_pages(torch, p):
    """`bases` distinct pages, repeated over the batch with a gain per page (so that the Otsu thresholds differ)"""
    base = torch.from_numpy(np.stack([ruled_page(p["h"], p["w"], i) for i in range(p["bases"])])).cuda()
    n = p["n"]
    shape = (n, p["h"], p["w"]) + ((3,) if p["c"] == 3 else ())
    pages = torch.empty(shape, dtype=torch.uint8, device="cuda")
    for i in range(n):
        g = (base[i % p["bases"]].to(torch.float32) * (0.75 + 0.25 * ((i * 7) % 11) / 10.0)).to(torch.uint8)
        if p["c"] == 3:
            for ch in range(3):
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


def run_workload(torch, prl, name, p, args):
    import lines_ref

    pages = make_pages(torch, p)
    out = torch.empty(pages.shape[:3], dtype=torch.uint8, device="cuda")
    t = timed(torch, lambda: prl.removeLines(pages, out=out), args.steps, args.warmup, args.repeats)
    px = p["n"] * p["h"] * p["w"]
    alg = px * (4 if p["c"] == 3 else 2)
    dup = torch.empty_like(pages)
    cp = timed(torch, lambda: dup.copy_(pages), args.steps, args.warmup, 1)
    copy_gbps = 2 * pages.numel() / cp["ms_median"] / 1e6
    del dup
    rec = dict(workload=name, op="removeLines", pages=p["n"], height=p["h"], width=p["w"], channels=p["c"], L=p["w"] // 50,
               Lv=p["h"] // 50, steps=args.steps, warmup=args.warmup, repeats=args.repeats, **t,
               mpix_per_s=round(px / t["ms_median"] / 1e3, 1), alg_bytes=alg, frac_8TBps=round(alg / t["ms_median"] / 1e9 / 8.0, 4),
               copy_GBps=round(copy_gbps, 1), frac_copy=round(alg / t["ms_median"] / 1e6 / copy_gbps, 4))
    if name == "G":   # the morphological part alone, from the byte path's public entries, on a fixed-threshold byte mask
        M = prl.morphology
        mask = torch.where(pages < 128, 255, 0).to(torch.uint8)
        hb, vb = torch.empty_like(mask), torch.empty_like(mask)

        def byte_openings():
            prl.morphologyEx(mask, M.MORPH_OPEN, M.MORPH_RECT, (p["w"] // 50, 1), out=hb)
            prl.morphologyEx(mask, M.MORPH_OPEN, M.MORPH_RECT, (1, p["h"] // 50), out=vb)

        b = timed(torch, byte_openings, args.steps, args.warmup, args.repeats)
        rec["byte_openings"] = b
        margin = b["ms_median"] - t["ms_median"]
        rec["margin_ms"] = round(margin, 4)
        rec["beats_byte_openings"] = bool(margin > max(b["spread_ms"], t["spread_ms"]))
        del mask, hb, vb
    if not args.no_check:
        j = p["n"] // 2 - 1
        rec["check"] = "ok" if np.array_equal(out[j].cpu().numpy(), lines_ref.remove_lines(pages[j].cpu().numpy())) else "MISMATCH"
    del pages, out
    torch.cuda.empty_cache()
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
        sys.exit("bench_lines.py needs a GPU")
    lines = []
    for name in [s for s in args.only.split(",") if s] or list(WORKLOADS):
        rec = run_workload(torch, prlib_amd, name, WORKLOADS[name], args)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in lines) + "\n")


if __name__ == "__main__":
    main()
