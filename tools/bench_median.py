#!/usr/bin/env python3
"""prl::denoiseSaltPepper on device-resident pages: one JSON line per workload.

    python tools/bench_median.py [--steps 10] [--warmup 3] [--only W1,W2] [--out FILE]

W1  256 x A4 gray (2480 x 3508), k = 3, times = 1      W2  the same at k = 5
W3  64 x 4096^2 x 3, k = 3                              W4  64 x A4 gray at k = 7 and k = 15 (the histogram kernel)
W5  W1 with times = 3

ms per call: `steps` calls after `warmup`, host clock closed by a device synchronise.  Algorithmic bytes: 2 B per
channel-pixel per pass (read + write).  frac_8TBps: those bytes over 8 TB/s; frac_copy_ceiling: over a device copy
(torch copy_ of 2 GiB, read + write) measured in the same run.  One page of each workload is checked against the
restatement of tests/median_ref.py outside the timed window (rows bands for the multi-pass and 4096^2 workloads).
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

WORKLOADS = {
    "W1": dict(n=256, h=3508, w=2480, c=1, k=3, times=1),
    "W2": dict(n=256, h=3508, w=2480, c=1, k=5, times=1),
    "W3": dict(n=64, h=4096, w=4096, c=3, k=3, times=1),
    "W4a": dict(n=64, h=3508, w=2480, c=1, k=7, times=1),
    "W4b": dict(n=64, h=3508, w=2480, c=1, k=15, times=1),
    "W5": dict(n=256, h=3508, w=2480, c=1, k=3, times=3),
}


def copy_ceiling(torch):
    a = torch.empty(1 << 31, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    b.copy_(a)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        b.copy_(a)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 5
    del a, b
    return 2 * (1 << 31) / dt


def make_pages(torch, n, h, w, c, seed):
    from prlib_amd import synth

    g = torch.Generator(device="cuda").manual_seed(seed)
    base = torch.from_numpy(synth.page_numpy(h, w, index=seed % 7)).cuda()
    pages = base[None, :, :, None].expand(n, h, w, c).contiguous()
    imp = torch.rand((n, h, w, c), device="cuda", generator=g) < 0.05
    val = (torch.rand((n, h, w, c), device="cuda", generator=g) < 0.5).to(torch.uint8) * 255
    pages = torch.where(imp, val, pages)
    del imp, val
    return pages.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--no-check", action="store_true")
    args = ap.parse_args()
    import torch

    import median_ref
    import prlib_amd

    if not torch.cuda.is_available():
        sys.exit("bench_median.py needs a GPU")
    ceiling = copy_ceiling(torch)
    names = [s for s in args.only.split(",") if s] or list(WORKLOADS)
    lines = []
    for i, name in enumerate(names):
        p = WORKLOADS[name]
        pages = make_pages(torch, p["n"], p["h"], p["w"], p["c"], 11 + i)
        out = torch.empty_like(pages)
        for _ in range(args.warmup):
            prlib_amd.denoiseSaltPepper(pages, p["k"], p["times"], out=out)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            prlib_amd.denoiseSaltPepper(pages, p["k"], p["times"], out=out)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / args.steps * 1e3
        cpx = p["n"] * p["h"] * p["w"] * p["c"]
        alg = 2 * cpx * p["times"]
        rec = dict(workload=name, pages=p["n"], height=p["h"], width=p["w"], channels=p["c"], ksize=p["k"], times=p["times"],
                   steps=args.steps, warmup=args.warmup, ms_per_call=round(ms, 4), mpix_per_s=round(cpx / ms / 1e3, 1),
                   alg_bytes=alg, alg_TBps=round(alg / ms / 1e9, 3), frac_8TBps=round(alg / ms / 1e9 / 8.0, 3),
                   copy_ceiling_TBps=round(ceiling / 1e12, 3), frac_copy_ceiling=round(alg / (ms * 1e-3) / ceiling, 3))
        if not args.no_check:
            j = p["n"] // 2
            src = pages[j].cpu().numpy()
            got = out[j].cpu().numpy()
            y0, y1 = p["h"] // 2, p["h"] // 2 + 48
            rows = [(0, 48), (y0, y1), (p["h"] - 48, p["h"])]
            rec["check"] = "ok" if all(np.array_equal(got[a:b], median_ref.denoise_salt_pepper_rows(src, p["k"], p["times"], a, b))
                                       for a, b in rows) else "MISMATCH"
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
