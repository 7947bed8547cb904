"""prl::autoCrop / prl::documentContour as a drop-in, without a device: the program that keeps the reference's #include line builds
with only -I include/prl, and the contract that needs no device holds (exceptions, the scale path, the gray input that becomes
BGR); the photograph fixtures are what their maker writes."""
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_dropin(out_dir):
    """g++ of tests/cpp/test_autocrop_dropin.cpp + prl_host.cpp, with only -I include/prl for the drop-in header."""
    exe = os.path.join(out_dir, "test_autocrop_dropin")
    flags = []
    for pc in ("opencv4", "opencv"):
        r = subprocess.run(["pkg-config", "--cflags", "--libs", pc], capture_output=True, text=True) if shutil.which("pkg-config") else None
        if r is not None and r.returncode == 0:
            flags = r.stdout.split()
            break
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include", "prl"),
           os.path.join(ROOT, "tests", "cpp", "test_autocrop_dropin.cpp"), os.path.join(ROOT, "prlib_amd", "csrc", "prl", "prl_host.cpp"),
           ] + flags + ["-L", os.path.join(ROOT, "prlib_amd"), "-lprlib_hip", "-Wl,-rpath," + os.path.join(ROOT, "prlib_amd"),
                        "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_cpp_dropin_without_a_device(prl, tmp_path):
    import torch

    exe = build_dropin(str(tmp_path))
    if torch.cuda.is_available():
        pytest.skip("a device is present; the no-device behaviour is checked on the CPU box")
    r = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "autocrop dropin cpu: OK" in r.stdout, r.stdout + r.stderr


def test_photograph_fixtures():
    paths = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "autocrop", "*.npz")))
    assert len(paths) >= 3
    for p in paths:
        assert os.path.getsize(p) <= 1 << 20, p
        z = np.load(p)
        bgr = z["bgr"]
        assert bgr.dtype == np.uint8 and bgr.ndim == 3 and bgr.shape[2] == 3
        assert z["quad"].dtype == np.float32 and z["quad"].shape == (8,) and int(z["tries"]) in (0, 1) and int(z["found"]) in (0, 1)
        assert int(z["found"]) or not z["quad"].any()
