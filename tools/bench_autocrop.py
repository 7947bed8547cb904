#!/usr/bin/env python3
"""prl::autoCrop on device-resident pages: where the time of the call goes.  One JSON line.

    python tools/bench_autocrop.py [--pages 256] [--steps 5] [--warmup 2] [--out FILE] [--no-check]

256 A4 colour pages (2480 x 3508 x 3), each a light quadrilateral on a dark table (tests/autocrop_cases.py; eight distinct pages,
repeated).  A call waits for the device by itself (the search needs the maps on the host), so every part is wall time around a
synchronised call, the median of `steps` calls after `warmup`:
    edges_ms     prl_hip_document_edges_batch_device alone: pyramid, channel choice, Canny
    contour_ms   prl_hip_document_contour_batch_device: the same plus the maps' copy to the host, the quad search per page on the
                 library's host thread pool, the closing and second search of the pages without a quad
    search_ms    contour_ms - edges_ms: the host half of the call at `pool_threads` threads (the library's rule for its pool:
                 PRL_HIP_HOST_COPY_THREADS, else half of the cores, at most 32)
    search_1t_ms the same searches one after the other on one thread (prl_hip_document_quad on the maps), for the scaling
    warp_ms      prl_hip_warp_crop_batch_device on the truncated corners (device events)
    auto_crop_ms prlib_amd.auto_crop end to end
One page is checked against the restatement outside the timed window.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

A4 = dict(h=3508, w=2480)


def pool_threads():
    env = int(os.environ.get("PRL_HIP_HOST_COPY_THREADS", "0") or 0)
    hc = max(1, os.cpu_count() or 1)
    n = min(64, env) if env > 0 else min(32, max(2, hc // 2))
    return max(1, min(n, hc))


def wall(torch, call, steps, warmup):
    for _ in range(warmup):
        call()
    ms = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-check", action="store_true")
    a = ap.parse_args()
    import torch

    import autocrop_cases as ac
    import prlib_amd as prl

    bases = np.stack([ac.page(A4["w"], A4["h"], "found", 3, seed=i, lean=0.01 * i) for i in range(8)])
    dev = torch.from_numpy(bases).cuda()
    pages = dev[torch.arange(a.pages, device="cuda") % 8].contiguous()
    n = a.pages
    res = {"bench": "auto_crop", "pages": n, "width": A4["w"], "height": A4["h"], "channels": 3, "steps": a.steps,
           "pool_threads": pool_threads(), "cpus": os.cpu_count()}
    quads, found, tries = prl.document_contour(pages)
    res["found"], res["after_closing"] = int(found.sum()), int(tries[found].sum())
    if not a.no_check:
        import contour_ref as cr

        want, want_try = cr.document_contour(bases[3])
        assert want is not None and np.array_equal(quads[3].reshape(8), want) and int(tries[3]) == want_try, "page 3 differs from the restatement"
        res["checked"] = True
    res["edges_ms"], res["edges_min"], res["edges_max"] = wall(torch, lambda: prl.document_edges(pages), a.steps, a.warmup)
    res["contour_ms"], res["contour_min"], res["contour_max"] = wall(torch, lambda: prl.document_contour(pages), a.steps, a.warmup)
    res["search_ms"] = res["contour_ms"] - res["edges_ms"]
    maps = prl.document_edges(pages)[0].cpu().numpy()
    t = time.perf_counter()
    for m in maps:
        prl.document_quad(m)
    res["search_1t_ms"] = (time.perf_counter() - t) * 1e3
    res["map"] = [int(maps.shape[2]), int(maps.shape[1])]
    q = quads[found].astype(np.int32).reshape(-1, 8)
    src = pages[torch.as_tensor(np.flatnonzero(found), device="cuda")]
    out = torch.empty((len(q), max(prl.warp_crop_size(r)[1] for r in q), max(prl.warp_crop_size(r)[0] for r in q), 3), dtype=torch.uint8,
                      device="cuda")
    ms = []
    for i in range(a.warmup + a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        prl.warp_crop(src, q, out=out)
        e1.record()
        torch.cuda.synchronize()
        if i >= a.warmup:
            ms.append(e0.elapsed_time(e1))
    res["warp_ms"] = statistics.median(ms)
    del out, src
    res["auto_crop_ms"] = wall(torch, lambda: prl.auto_crop(pages), a.steps, a.warmup)[0]
    res = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
