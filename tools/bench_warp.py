#!/usr/bin/env python3
"""prl::warpCrop (warp.hip) on device-resident pages: one JSON line per workload and operation.

    python tools/bench_warp.py [--steps 10] [--warmup 3] [--repeats 5] [--only G,C] [--out FILE] [--no-check]

G   256 x A4 gray (2480 x 3508), one mild keystone quad for every page
C   64 x A4 x 3 channels, the same quad

Per workload, timed in the same run between two device events on the current stream:
    warp_crop   prl_hip_warp_crop_batch_device (sizes, matrices, the record upload and k_warp_persp)
    rotate      prl_hip_rotate_batch_device by 3.7 degrees on the same pages (k_warp of rotate.hip: the affine yardstick; its result
                is the max(W, H) square, so it makes more pixels - compare ns_per_out_px)
    copy        a device-to-device copy of the batch (the streaming yardstick)
ms: per repeat the median of `steps` calls after `warmup`; the line reports the median, the minimum and the maximum of the
`repeats` medians and their spread (max - min).  alg_bytes = source bytes + result bytes; frac_copy: those bytes at the copy's
measured rate over the time taken.  One page of each workload is checked against tests/warp_ref.py outside the timed window.
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
QUAD = [60, 45, 2410, 20, 2455, 3470, 25, 3440]   # a page photographed slightly from the lower left
ANGLE = 3.7


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default="G,C")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-check", action="store_true")
    args = ap.parse_args()
    import torch

    import prlib_amd as prl
    from prlib_amd import _capi
    from prlib_amd.deskew import rotate_out_size

    L = _capi.lib()
    lines = []
    for name, n, c in (("G", 256, 1), ("C", 64, 3)):
        if name not in args.only.split(","):
            continue
        pages = make_pages(torch, n, c)
        t4 = pages if pages.dim() == 4 else pages[:, :, :, None]
        h, w = A4["h"], A4["w"]
        stream = torch.cuda.current_stream().cuda_stream
        ow, oh = prl.warp_crop_size(QUAD)
        out = torch.empty((n, oh, ow, c), dtype=torch.uint8, device="cuda")
        quads = np.ascontiguousarray(np.broadcast_to(np.asarray(QUAD, np.int32), (n, 8)))
        wh = np.zeros((n, 2), np.int32)
        val = np.zeros(4)

        def warp():
            _capi.check(L.prl_hip_warp_crop_batch_device(n, c, quads.ctypes.data, -1.0, t4.data_ptr(), t4.stride(0), t4.stride(1), w, h,
                                                         out.data_ptr(), out.stride(0), out.stride(1), wh.ctypes.data, 0, val.ctypes.data, stream))

        rw, rh = rotate_out_size(w, h, ANGLE)
        rout = torch.empty((n, rh, rw, c), dtype=torch.uint8, device="cuda")
        angles = np.full(n, ANGLE)

        def rotate():
            _capi.check(L.prl_hip_rotate_batch_device(n, c, angles.ctypes.data, t4.data_ptr(), t4.stride(0), t4.stride(1), w, h,
                                                      rout.data_ptr(), rout.stride(0), rout.stride(1), stream))

        cdst = torch.empty_like(pages)
        t_copy = timed(torch, lambda: cdst.copy_(pages), args.steps, args.warmup, args.repeats)
        copy_gbps = 2 * pages.numel() / t_copy["ms_median"] / 1e6
        if not args.no_check:
            import warp_ref as wr

            warp()
            torch.cuda.synchronize()
            want = wr.warp_crop(t4[n - 1].cpu().numpy(), QUAD)
            assert (wh == (ow, oh)).all() and np.array_equal(out[n - 1].cpu().numpy(), want), "warp_crop differs from tests/warp_ref.py"
        for op, call, opx in (("warp_crop", warp, n * ow * oh), ("rotate", rotate, n * rw * rh), ("copy", None, pages.numel() // c)):
            t = t_copy if call is None else timed(torch, call, args.steps, args.warmup, args.repeats)
            alg = pages.numel() + opx * c
            lines.append(dict(workload=name, op=op, pages=n, height=h, width=w, channels=c, out_px=opx, steps=args.steps, warmup=args.warmup,
                              repeats=args.repeats, **t, alg_bytes=alg, ns_per_out_px=round(t["ms_median"] * 1e6 / opx, 4),
                              GBps=round(alg / t["ms_median"] / 1e6, 1), copy_GBps=round(copy_gbps, 1),
                              frac_copy=round(alg / t["ms_median"] / 1e6 / copy_gbps, 4)))
            print(json.dumps(lines[-1]), flush=True)
        del pages, out, rout, cdst
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
