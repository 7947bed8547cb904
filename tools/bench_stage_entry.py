"""Host time per call of four stage entries on one 64 x 64 gray page, where the kernels are a few microseconds and what is
measured is the entry's own code: prl_hip_lut_batch_device (checks and a launch: no workspace, no lock),
prl_hip_median_batch_device(k = 3, times = 1) (checks, the shared workspace's lock and acquire, a launch),
prl_hip_nlm_planes_device(1 channel, h = 10) (checks, the workspace, the weight table cached from the call before, a launch: a
table rebuilt and uploaded per call would show here) and prl_hip_morph_batch_device(9 iterations) (checks, the workspace with a
scratch plane, the large-radius launches).

    python tools/bench_stage_entry.py [--lib PATH] [--calls 4000] [--repeats 5]

One JSON line per repeat and entry: wall time of `calls` calls with the stream drained at the end, over `calls`.  Two builds are
compared by running this program for each of them in turn, alternating, on the same machine (--lib picks the library)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--calls", type=int, default=4000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    from prlib_amd import _capi

    if a.lib:
        _capi.use_library(a.lib)
    import torch

    L = _capi.lib()
    n, w, h = 1, 64, 64
    src = torch.randint(0, 256, (n, h, w), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    table = torch.arange(255, -1, -1, dtype=torch.uint8, device="cuda")
    stream = _capi.stream_on(src)
    s, d, t = src.data_ptr(), dst.data_ptr(), table.data_ptr()
    entries = {
        "lut": lambda: L.prl_hip_lut_batch_device(n, 1, t, 0, s, w * h, w, w, h, d, w * h, w, stream),
        "median3": lambda: L.prl_hip_median_batch_device(n, 1, 3, 1, s, w * h, w, w, h, d, w * h, w, stream),
        "nlm_planes": lambda: L.prl_hip_nlm_planes_device(n, 1, 10.0, s, w * h, w, w, h, d, w * h, w, stream),
        "morph9": lambda: L.prl_hip_morph_batch_device(9, n, s, w * h, w, w, h, d, w * h, w, stream),
    }
    for name, call in entries.items():
        for _ in range(200):   # warm-up: code objects, the workspace
            _capi.check(call())
        torch.cuda.synchronize()
        for r in range(a.repeats):
            t0 = time.perf_counter()
            for _ in range(a.calls):
                st = call()
            torch.cuda.synchronize()
            us = (time.perf_counter() - t0) / a.calls * 1e6
            _capi.check(st)
            print(json.dumps({"tag": a.tag, "entry": name, "repeat": r, "calls": a.calls, "us_per_call": round(us, 3)}), flush=True)


if __name__ == "__main__":
    main()
