#!/usr/bin/env python3
"""The component labeller and rule R's rectangles (components.hip) on device-resident edge maps, and prl::binarizeLocalOtsu with its
rectangles from the device and from the host scan: one JSON line per workload.

    python tools/bench_components.py [--steps 5] [--warmup 1] [--repeats 5] [--only G,C] [--pages 0] [--out FILE] [--no-check]

G   256 x A4 gray synthetic text pages (2480 x 3508);  C   64 x A4 x 3 channels
    The maps are what binarizeLocalOtsu labels: CannyEdgeDetection(19, 0.15, 0.01, 1) of the pages, dilated 7 x 7.
        labels_ms      prl_hip_connected_components_batch_device at connectivity 8, counts only (no label plane written out)
        rects_ms       prl_hip_external_rects_batch_device with room for every rectangle (a batch of more than one chunk of pages is
                       labelled twice: once for the counts, once to write)
        labels_one_chunk_ms, rects_one_chunk_ms   the same two on the first 64 pages: one chunk, one statistics pass, labelled once
        after_labels_ms  rects_one_chunk_ms - labels_one_chunk_ms: the outer flags, the statistics and the second compaction of 64
                       pages BY DIFFERENCE (the numbering of the external roots instead of all roots is on both sides)
        copy_ms        a device-to-device copy of the maps (read + write): the floor of one pass over them
        call_device_ms the whole prl_hip_binarize_local_otsu_batch_device call, header defaults, with PRL_HIP_LO_HOST_RECTS=0: the
                       rectangles from components.hip
        call_host_ms   the same call with PRL_HIP_LO_HOST_RECTS=1: the read-back and the host scan (the library's path)
    Both entries and the call wait for their stream: the host clock around them.  ms: per repeat the median of `steps` calls after
    `warmup`; the line reports the median, the minimum and the maximum of the `repeats` medians.  The two whole calls run in child
    processes of this one, one after the other in the same session, on the hooks build (the knob is read once per process); their
    masks and counts on the first two pages are compared.  The rectangles of two pages are checked against the host scan.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

RUNS = {"G": (256, 3508, 2480, 1), "C": (64, 3508, 2480, 3)}


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


def child(args):
    """one whole-call measurement on whichever path the environment selects: a JSON line with the times and a digest"""
    from prlib_amd import _capi

    _capi.use_library(_capi.HOOKS_LIB_PATH)
    import torch

    import prlib_amd as prl
    from bench_focus import make_pages

    n, h, w, c = RUNS[args.child]
    n = args.pages or n
    pages = make_pages(torch, n, h, w, c)
    out = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
    rec = {}
    triple(rec, "call_ms", host_timed(torch, lambda: prl.binarizeLocalOtsu(pages, out=out), args.steps, args.warmup, args.repeats))
    mask, found, kept = prl.binarizeLocalOtsu(pages[:2], with_counts=True)
    rec.update(found=found.tolist(), kept=kept.tolist(), black=int((mask == 0).sum()), digest=int(mask.to(torch.int64).mul_(torch.arange(mask.numel(), device="cuda").view(mask.shape) % 8191).sum()))
    print(json.dumps(rec), flush=True)


def whole_call(args, name, host):
    env = dict(os.environ)
    env.pop("PRL_HIP_LO_HOST_RECTS", None)
    env["PRL_HIP_LO_HOST_RECTS"] = "1" if host else "0"
    cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--repeats", str(args.repeats), "--pages", str(args.pages)]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        raise RuntimeError("the whole-call child failed: " + r.stdout[-1000:] + r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def run(torch, prl, args, name, n, h, w, c):
    from bench_focus import make_pages, timed
    from prlib_amd import _capi, morphology

    n = args.pages or n
    rec = dict(workload=name, pages=n, height=h, width=w, channels=c, steps=args.steps, warmup=args.warmup, repeats=args.repeats)
    pages = make_pages(torch, n, h, w, c)
    maps = prl.morphologyEx(prl.cannyEdgeDetection(pages), morphology.MORPH_DILATE, morphology.MORPH_RECT, (7, 7))
    del pages
    torch.cuda.empty_cache()
    L, stream = _capi.lib(), _capi.stream_on(maps)
    counts, found, kept, offsets = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n + 1, np.int32)
    src = (maps.data_ptr(), maps.stride(0), maps.stride(1), w, h)

    def labels(k=n):
        _capi.check(L.prl_hip_connected_components_batch_device(k, 8, *src, None, 0, 0, counts.ctypes.data, None, 0, stream))

    def rects_into(room, cap, k=n):
        _capi.check(L.prl_hip_external_rects_batch_device(k, *src, room.data_ptr() if room is not None else None, cap, offsets.ctypes.data,
                                                          found.ctypes.data, kept.ctypes.data, stream))

    triple(rec, "labels_ms", host_timed(torch, labels, args.steps, args.warmup, args.repeats))
    rects_into(None, 0)
    total = int(offsets[n])
    room = torch.empty((max(total, 1), 4), dtype=torch.int32, device="cuda")
    triple(rec, "rects_ms", host_timed(torch, lambda: rects_into(room, total), args.steps, args.warmup, args.repeats))
    # one chunk, one statistics pass: the entry labels once, so the difference to the labeller is what comes after the labels
    one = min(n, 64)
    triple(rec, "labels_one_chunk_ms", host_timed(torch, lambda: labels(one), args.steps, args.warmup, args.repeats))
    triple(rec, "rects_one_chunk_ms", host_timed(torch, lambda: rects_into(room, total, one), args.steps, args.warmup, args.repeats))
    rects_into(room, total)
    other = torch.empty_like(maps)
    triple(rec, "copy_ms", timed(torch, lambda: other.copy_(maps), args.steps, args.warmup, args.repeats))
    del other
    rec.update(one_chunk_pages=one, after_labels_ms=round(rec["rects_one_chunk_ms"] - rec["labels_one_chunk_ms"], 3), foreground=round(float((maps[:4] != 0).float().mean()), 4),
               components_per_page=[int(np.median(counts)), int(counts.min()), int(counts.max())],
               found_per_page=[int(np.median(found)), int(found.min()), int(found.max())],
               kept_per_page=[int(np.median(kept)), int(kept.min()), int(kept.max())],
               labels_over_copy=round(rec["labels_ms"] / rec["copy_ms"], 2), rects_over_copy=round(rec["rects_ms"] / rec["copy_ms"], 2),
               ns_per_pixel=round(rec["rects_ms"] * 1e6 / maps.numel(), 5))
    ok = True
    if not args.no_check:
        got = room.cpu().numpy()
        for i in (0, n - 1):
            want, want_found = prl.externalRects(maps[i].cpu().numpy())
            ok = ok and want_found == found[i] and np.array_equal(got[offsets[i]:offsets[i + 1]], want)
    del maps, room
    torch.cuda.empty_cache()
    dev, host = whole_call(args, name, False), whole_call(args, name, True)
    for key in ("call_ms", "call_ms_min", "call_ms_max"):
        rec[key.replace("call_", "call_device_")], rec[key.replace("call_", "call_host_")] = dev[key], host[key]
    rec["host_over_device"] = round(host["call_ms"] / dev["call_ms"], 3)
    if not args.no_check:
        ok = ok and all(dev[k] == host[k] for k in ("found", "kept", "black", "digest"))
        rec["check"] = "ok" if ok else "MISMATCH"
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pages", type=int, default=0)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--child", default="")
    args = ap.parse_args()
    if args.child:
        return child(args)
    import torch

    import prlib_amd

    if not torch.cuda.is_available():
        sys.exit("bench_components.py needs a GPU")
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
