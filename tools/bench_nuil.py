#!/usr/bin/env python3
"""prl::correctNUIL and the morphology under it on device-resident pages: one JSON line per workload.

    python tools/bench_nuil.py [--steps 10] [--warmup 3] [--only G31,C31] [--out FILE] [--no-check] [--no-literal]

G15 / G31 / G101   256 x A4 gray (2480 x 3508), correctNUIL at size 15 / 31 / 101
C15 / C31 / C101   64 x A4 x 3 channels, the same sizes
R31                256 x A4 gray, cv::morphologyEx(MORPH_CLOSE, 31 x 31 rectangle): the separable yardstick
P31 / L31          32 x A4 gray, correctNUIL at size 31: the span kernel (P31) and, in a child process that loads the hooks
                   build with PRL_HIP_GMORPH_LITERAL=1, the by-the-definition kernel (L31) on the same pages in the same run;
                   speedup_vs_literal on the P31 line is L31 / P31

ms: the median of `steps` calls after `warmup`, each between two device events on the current stream.  Algorithmic bytes: 2 B
per pixel and channel (read + write once); frac_8TBps: those bytes over 8 TB/s.  One page of each workload is checked against
the restatement of tests/nuil_ref.py on three bands of rows, outside the timed window.
Kernel times: run this under `rocprofv3 --kernel-trace --stats` separately.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

A4 = dict(h=3508, w=2480)
WORKLOADS = {
    "G15": dict(n=256, c=1, size=15, **A4), "G31": dict(n=256, c=1, size=31, **A4), "G101": dict(n=256, c=1, size=101, **A4),
    "C15": dict(n=64, c=3, size=15, **A4), "C31": dict(n=64, c=3, size=31, **A4), "C101": dict(n=64, c=3, size=101, **A4),
    "R31": dict(n=256, c=1, size=31, rect_close=True, **A4),
    "P31": dict(n=32, c=1, size=31, **A4),
    "L31": dict(n=32, c=1, size=31, literal=True, **A4),
}


def make_pages(torch, n, h, w, c, seed):
    """synthetic text pages under a shadow that differs per page; every fifth page is a negative"""
    from prlib_amd import synth

    g = torch.Generator(device="cuda").manual_seed(seed)
    base = torch.from_numpy(synth.page_numpy(h, w, index=seed % 7)).cuda().to(torch.float32)
    lo = 0.45 + 0.5 * torch.rand((n, 1, 1, 1), device="cuda", generator=g)
    ramp = torch.linspace(0.0, 1.0, w, device="cuda")[None, None, :, None]
    pages = (base[None, :, :, None] * (1.0 - ramp * (1.0 - lo))).to(torch.uint8).expand(n, h, w, c).contiguous()
    pages[4::5] = 255 - pages[4::5]
    return pages


def run_workload(torch, prl, name, p, steps, warmup, check):
    import nuil_ref

    pages = make_pages(torch, p["n"], p["h"], p["w"], p["c"], 11)
    out = torch.empty_like(pages)
    if p.get("rect_close"):
        call = lambda: prl.morphologyEx(pages, prl.morphology.MORPH_CLOSE, prl.morphology.MORPH_RECT, p["size"], out=out)   # noqa: E731
    else:
        call = lambda: prl.correctNUIL(pages, p["size"], out=out)   # noqa: E731
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
    med = float(np.median(ms))
    cpx = p["n"] * p["h"] * p["w"] * p["c"]
    rec = dict(workload=name, op="close_rect" if p.get("rect_close") else "correctNUIL", kernel="literal" if p.get("literal") else "span",
               pages=p["n"], height=p["h"], width=p["w"], channels=p["c"], size=p["size"], steps=steps, warmup=warmup,
               ms_median=round(med, 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4), mpix_per_s=round(cpx / med / 1e3, 1),
               alg_bytes=2 * cpx, frac_8TBps=round(2 * cpx / med / 1e9 / 8.0, 4))
    if check:
        j = p["n"] // 2 - 1 if p["n"] > 1 else 0   # (a negative page when n >= 10)
        src, got = pages[j].cpu().numpy(), out[j].cpu().numpy()
        bands = [(0, 40), (p["h"] // 2, p["h"] // 2 + 40), (p["h"] - 40, p["h"])]
        if p.get("rect_close"):
            def want(a, b):
                r = p["size"] - 1
                b0, b1 = max(0, a - 2 * r), min(p["h"], b + 2 * r)
                return nuil_ref.morphology_ex(src[b0:b1], nuil_ref.CLOSE, nuil_ref.RECT, p["size"], p["size"])[a - b0:b - b0]
        else:
            def want(a, b):
                return nuil_ref.correct_nuil_rows(src, p["size"], a, b)
        rec["check"] = "ok" if all(np.array_equal(got[a:b], want(a, b)) for a, b in bands) else "MISMATCH"
    del pages, out
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--no-literal", action="store_true")
    ap.add_argument("--child-literal", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()

    if args.child_literal:   # the hooks build reads the knob; a fresh process because a library is loaded once
        from prlib_amd import _capi

        _capi.use_library(_capi.HOOKS_LIB_PATH)
    import torch

    import prlib_amd

    if not torch.cuda.is_available():
        sys.exit("bench_nuil.py needs a GPU")
    names = [s for s in args.only.split(",") if s] or list(WORKLOADS)
    if args.child_literal:
        names = ["L31"]
    lines, recs = [], {}
    for name in names:
        p = WORKLOADS[name]
        if p.get("literal") and not args.child_literal:
            if args.no_literal:
                continue
            env = dict(os.environ, PRL_HIP_GMORPH_LITERAL="1")
            cmd = [sys.executable, os.path.abspath(__file__), "--child-literal", "--steps", str(args.steps), "--warmup", str(args.warmup)]
            r = subprocess.run(cmd + (["--no-check"] if args.no_check else []), capture_output=True, text=True, env=env)
            if r.returncode != 0:
                sys.exit("the literal leg failed: " + r.stderr[-2000:])
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            if "P31" in recs:
                recs["P31"]["speedup_vs_literal"] = round(rec["ms_median"] / recs["P31"]["ms_median"], 2)
        else:
            rec = run_workload(torch, prlib_amd, name, p, args.steps, args.warmup, not args.no_check)
        recs[name] = rec
        if name != "P31" or args.no_literal or "L31" not in names:
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        if name == "L31" and "P31" in recs:
            print(json.dumps(recs["P31"]), flush=True)
            lines.append(recs["P31"])
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in lines) + "\n")


if __name__ == "__main__":
    main()
