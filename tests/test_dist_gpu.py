"""The multi-GPU plumbing of bench.py on the ONE GPU a test box has (VERDICT r3 "next" 4), so that the driver's
first 8-GPU run measures throughput instead of finding a plumbing bug:

* an RCCL world of one rank (PRL_FORCE_DIST=1): init_process_group("nccl"), barrier(device_ids=...), the device all_reduce
  of the max-over-ranks, destroy_process_group - the exact calls an N-rank run makes, with real kernels in between;
* two ranks on one GPU over gloo (PRL_DIST_BACKEND=gloo; RCCL refuses two ranks on one device) through the real kernels
  with the weak line carrying the strong-scaling measurement: the masks of the two ranks' blocks, in page-list order, equal
  the single-process run of the same page list (CRC-32 per page).
"""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = ["--full", "--steps", "2", "--warmup", "1", "--size", "1024", "--traffic", "0", "--ceilings", "0", "--cpu-seconds", "0",
          "--worst-case", "0", "--end-to-end", "0", "--digest", "1"]   # (--full: the parity check against the oracle)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _line(r):
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def _env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.update(extra)
    return env


def test_rccl_world_of_one_runs_the_bench_protocol(cuda_device):
    env = _env(PRL_FORCE_DIST="1", WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--pages", "8"] + COMMON,
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    d = _line(r)
    assert d["n_gpus"] == 1 and d["config"]["pages_total"] == 8 and d["value"] > 0
    assert d["parity"]["mismatching_pixels"] == 0 and len(d["page_digests"]) == 8
    assert d["config"]["dist_backend"] == "nccl"   # (RCCL; a single rank only joins a process group under PRL_FORCE_DIST)


def test_two_gloo_ranks_on_one_gpu_equal_the_single_process(cuda_device):
    single = _line(subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--pages", "6"] + COMMON,
                                  capture_output=True, text=True, timeout=600, env=_env(), cwd=ROOT))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--pages", "3", "--scaling", "both"] + COMMON
    two = _line(subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=_env(PRL_DIST_BACKEND="gloo"), cwd=ROOT))
    assert two["n_gpus"] == 2 and two["scaling"] == "weak" and two["config"]["pages_total"] == 6 and two["config"]["pages_per_gpu"] == 3
    assert two["strong"]["pages_total"] == 3 and two["strong"]["value"] > 0        # the strong-scaling measurement rode along
    assert two["parity"]["mismatching_pixels"] == 0 and two["config"]["dist_backend"] == "gloo" and single["config"]["dist_backend"] is None
    assert two["page_digests"] == single["page_digests"] and len(single["page_digests"]) == 6
