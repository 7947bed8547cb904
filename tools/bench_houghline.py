#!/usr/bin/env python3
"""prl::findHoughLineContour on device-resident pages: where the time of the call goes.  One JSON line per workload.

    python tools/bench_houghline.py [--gray-pages 256] [--colour-pages 64] [--steps 5] [--warmup 1] [--out FILE] [--no-check]

A4 pages (2480 x 3508), each a light quadrilateral on a dark table (tests/houghline_cases.py, 'found' and 'broken', eight distinct
pages, repeated), gray and 3-channel.  Every figure is the median of `steps` synchronised calls after `warmup`, with the smallest and
the largest beside it:
    edges_ms       prl_hip_hough_edges_batch_device: six median passes, Canny
    vote_ms        prl_hip_hough_accumulator_batch_device on the edge maps: point lists and votes (device events; it only enqueues)
    lines_ms       prl_hip_hough_lines_batch_device(threshold 50) on the edge maps: the same votes, then the peaks, the read-back of
                   the counts and of the peak lists and the sort on the host
    peaks_sort_readback_ms   lines_ms - vote_ms: the three are one synchronised stretch of the entry and are not timed apart
    readback_copy_ms         a pinned device-to-host copy of as many bytes as the peak lists and counts hold, for scale
    search_ms      contour_ms - edges_ms - lines_ms: the line filter and the quad search on the library's host thread pool
    search_1t_ms   the same searches one after the other on one thread (prl_hip_hough_line_quad on the lines)
    contour_ms     prl_hip_hough_line_contour_batch_device end to end
Then one A4 page that is a single long horizontal line plus noise, the same-address case of the LDS atomics (every point of the line
votes for one cell at its angle), beside a page with as many points scattered: vote_ms of each alone.
For scale, the plain C++ voting loop of houghline.h (tests/cpp/test_houghline.cpp, g++ -O2, one thread) on one of the edge maps.
One gray page is checked against the restatement outside the timed window.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 2480, 3508


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
    return [round(statistics.median(ms), 3), round(min(ms), 3), round(max(ms), 3)]


def events(torch, call, steps, warmup):
    ms = []
    for i in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    return [round(statistics.median(ms), 3), round(min(ms), 3), round(max(ms), 3)]


def cpu_vote_ms(edge_map, reps):
    with tempfile.TemporaryDirectory() as d:
        exe, raw = os.path.join(d, "test_houghline"), os.path.join(d, "map.raw")
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "test_houghline.cpp"), "-o", exe],
                       check=True)
        with open(raw, "wb") as f:
            f.write(np.ascontiguousarray(edge_map).tobytes())
        out = subprocess.run([exe, "time", str(edge_map.shape[1]), str(edge_map.shape[0]), str(reps), raw], capture_output=True, text=True,
                             check=True).stdout
    ms = [float(ln.split()[1]) for ln in out.splitlines() if ln.startswith("vote_ms")]
    return [round(statistics.median(ms), 3), round(min(ms), 3), round(max(ms), 3)]


def workload(torch, prl, hc, n, channels, a):
    import houghline_ref as ref

    bases = np.stack([hc.photo(W, H, "found" if i % 2 == 0 else "broken", channels, seed=i) for i in range(8)])
    dev = torch.from_numpy(bases).cuda()
    pages = dev[torch.arange(n, device="cuda") % 8].contiguous()
    res = {"bench": "hough_line_contour", "pages": n, "width": W, "height": H, "channels": channels, "steps": a.steps, "cpus": os.cpu_count()}
    quads, found, n_lines = prl.hough_line_contour(pages)
    res["found"], res["lines_per_page"] = int(found.sum()), [int(n_lines.min()), int(n_lines.max())]
    if not a.no_check and channels == 1:
        want, want_lines = ref.hough_line_contour(bases[1])
        assert want is not None and np.array_equal(quads[1], want) and int(n_lines[1]) == want_lines, "page 1 differs from the restatement"
        res["checked"] = True
    res["edges_ms"] = wall(torch, lambda: prl.hough_edges(pages), a.steps, a.warmup)
    maps = prl.hough_edges(pages)
    res["edge_points_per_page"] = int((maps != 0).sum().item()) // n
    acc = torch.empty((n,) + tuple(x + 2 for x in prl.hough_lines_geometry(W, H)), dtype=torch.int32, device="cuda")
    res["vote_ms"] = events(torch, lambda: prl.hough_accumulator(maps, out=acc), a.steps, a.warmup)
    del acc
    res["lines_ms"] = wall(torch, lambda: prl.hough_lines(maps, 50, max_lines=512), a.steps, a.warmup)
    res["peaks_sort_readback_ms"] = round(res["lines_ms"][0] - res["vote_ms"][0], 3)
    lines = prl.hough_lines(maps, 50)
    nbytes = sum(len(ln) for ln in lines) * 8 + 4 * n
    src, dst = torch.zeros(nbytes, dtype=torch.uint8, device="cuda"), torch.zeros(nbytes, dtype=torch.uint8).pin_memory()
    res["readback_bytes"] = nbytes
    res["readback_copy_ms"] = wall(torch, lambda: dst.copy_(src, non_blocking=True), a.steps, a.warmup)
    res["contour_ms"] = wall(torch, lambda: prl.hough_line_contour(pages), a.steps, a.warmup)
    res["search_ms"] = round(res["contour_ms"][0] - res["edges_ms"][0] - res["lines_ms"][0], 3)
    t = time.perf_counter()
    for ln in lines:
        prl.hough_line_quad(ln, W, H)
    res["search_1t_ms"] = round((time.perf_counter() - t) * 1e3, 3)
    res["ms_per_page"] = round(res["contour_ms"][0] / n, 4)
    if channels == 1:
        res["cpu_vote_one_page_ms"] = cpu_vote_ms(maps[1].cpu().numpy(), a.steps)
        res["vote_one_page_ms"] = round(res["vote_ms"][0] / n, 4)
    return res


def same_address(torch, prl, a):
    rng = np.random.default_rng(1)
    noise = np.zeros((H, W), np.uint8)
    noise[rng.integers(0, H, 20000), rng.integers(0, W, 20000)] = 255
    line = noise.copy()
    line[H // 2, :] = 255
    scattered = noise.copy()
    extra = int((line != 0).sum() - (noise != 0).sum())
    ys, xs = rng.integers(0, H, 4 * extra), rng.integers(0, W, 4 * extra)
    free = np.flatnonzero(scattered[ys, xs] == 0)
    keep = np.unique(ys[free].astype(np.int64) * W + xs[free], return_index=True)[1][:extra]
    scattered[ys[free][keep], xs[free][keep]] = 255
    res = {"bench": "hough_same_address", "width": W, "height": H, "points_line": int((line != 0).sum()),
           "points_scattered": int((scattered != 0).sum()), "steps": a.steps}
    acc = torch.empty(tuple(x + 2 for x in prl.hough_lines_geometry(W, H)), dtype=torch.int32, device="cuda")
    for name, m in (("line", line), ("scattered", scattered)):
        t = torch.from_numpy(m).cuda()
        res[f"vote_{name}_ms"] = events(torch, lambda: prl.hough_accumulator(t, out=acc), a.steps, a.warmup + 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gray-pages", type=int, default=256)
    ap.add_argument("--colour-pages", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-check", action="store_true")
    a = ap.parse_args()
    import torch

    import houghline_cases as hc
    import prlib_amd as prl

    lines = []
    for n, channels in ((a.gray_pages, 1), (a.colour_pages, 3)):
        if n > 0:
            lines.append(json.dumps(workload(torch, prl, hc, n, channels, a)))
            print(lines[-1], flush=True)
            torch.cuda.empty_cache()
    lines.append(json.dumps(same_address(torch, prl, a)))
    print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
