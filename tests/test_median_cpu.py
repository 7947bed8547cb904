"""prl::denoiseSaltPepper without a device: the restatement (tests/median_ref.py) against scipy and the definition,
hand-derived answers that pin the border, the C ABI's statuses and exports, and the drop-in header's C++ contract."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import median_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (1, 9), (9, 1), (2, 2), (33, 41)]


def _img(shape, c, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, size=shape + (c,), dtype=np.uint8)
    return a[:, :, 0] if c == 1 and seed % 2 else a


@pytest.mark.parametrize("k", [1, 3, 5, 7, 9, 101])
@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_restatement_equals_scipy(k, c):
    nd = pytest.importorskip("scipy.ndimage")
    for i, shape in enumerate(SHAPES):
        img = _img(shape, c, 7 * k + c + i)
        got = median_ref.denoise_salt_pepper(img, k, 1)
        a = median_ref._as3(img)
        want = np.stack([nd.median_filter(a[:, :, ch], size=(k, k), mode="nearest") for ch in range(a.shape[2])], axis=2)
        assert np.array_equal(median_ref._as3(got), want), (k, c, shape)


@pytest.mark.parametrize("k", [1, 3, 5, 7, 9, 101])
@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_restatement_equals_pixel_loop(k, c):
    for i, shape in enumerate(SHAPES[:4] + [(11, 13)]):
        img = _img(shape, c, 11 * k + c + i)
        assert np.array_equal(median_ref.denoise_salt_pepper(img, k, 1), median_ref.median_loop(img, k) if k > 1 else img)


def test_both_restatements_agree():
    img = _img((23, 29), 3, 5)
    for k in (3, 5):
        a = median_ref._pass_partition(median_ref._as3(img), k)
        b = median_ref._pass_count(median_ref._as3(img), k)
        assert np.array_equal(a, b)


def test_rows_of_a_band_equal_the_whole_page():
    img = _img((40, 17), 3, 9)
    for k, times in ((3, 2), (5, 3), (7, 1)):
        whole = median_ref.denoise_salt_pepper(img, k, times)
        for y0, y1 in ((0, 5), (12, 20), (33, 40)):
            assert np.array_equal(median_ref.denoise_salt_pepper_rows(img, k, times, y0, y1), whole[y0:y1])


def test_known_answers():
    page = np.full((7, 8), 100, np.uint8)
    for v in (0, 255):
        p = page.copy()
        p[3, 4] = v
        assert np.array_equal(median_ref.denoise_salt_pepper(p, 3, 1), page)   # an impulse vanishes at k = 3
    top = np.zeros((6, 9), np.uint8)
    top[0] = 255
    got = median_ref.denoise_salt_pepper(top, 3, 1)
    assert np.array_equal(got, top)   # replicate: row 0's window holds row 0 twice -> 6 of 9 values are 255
    # (reflect-101 would see rows 1, 0, 1: 3 of 9 -> the row would vanish)
    assert median_ref.denoise_salt_pepper(top, 3, 2)[0].tolist() == [255] * 9


def test_declared_and_exported(prl):
    from prlib_amd import _capi

    header = open(os.path.join(ROOT, "include", "prl_hip.h")).read()
    for name in ("prl_hip_median_batch_device", "prl_hip_median_host"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _capi.EXPORTED_SYMBOLS
    if shutil.which("nm") is None:
        pytest.skip("binutils not installed")
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "prlib_amd", "libprlib_hip.so")],
                         capture_output=True, text=True, check=True).stdout
    for name in ("prl_hip_median_batch_device", "prl_hip_median_host"):
        assert re.search(r"\bT " + name + r"\b", out), name
    assert os.path.exists(os.path.join(ROOT, "include", "prl", "denoiseSaltPepper.h"))


def test_statuses_without_touching_a_device(prl):
    from prlib_amd import _capi

    L = _capi.lib()
    src = np.zeros((8, 12, 4), np.uint8)
    dst = np.zeros_like(src)
    s, d = src.ctypes.data, dst.ctypes.data

    def dev(n=1, c=1, k=3, times=1, sp=s, ss=12, w=12, h=8, dp=d, ds=12):
        return L.prl_hip_median_batch_device(n, c, k, times, sp, 96 * 4, ss, w, h, dp, 96 * 4, ds, None)

    def host(c=1, k=3, times=1, sp=s, ss=12, w=12, h=8, dp=d, ds=12):
        return L.prl_hip_median_host(c, k, times, sp, ss, w, h, dp, ds)

    for f in (dev, host):
        assert f(w=0) == _capi.PRL_ERR_EMPTY and f(h=-1) == _capi.PRL_ERR_EMPTY
        for k in (0, -1, 2, 4, -3):
            assert f(k=k) == _capi.PRL_ERR_BAD_WINDOW, k
        for c in (0, 5, -1):
            assert f(c=c) == _capi.PRL_ERR_BAD_CHANNELS
        assert f(c=2, k=7, ss=24, ds=24) == _capi.PRL_ERR_BAD_CHANNELS
        assert f(c=2, k=101, ss=24, ds=24) == _capi.PRL_ERR_BAD_CHANNELS
        assert f(sp=None) == _capi.PRL_ERR_BAD_ARG and f(dp=None) == _capi.PRL_ERR_BAD_ARG
        assert f(ss=11) == _capi.PRL_ERR_BAD_ARG and f(ds=11) == _capi.PRL_ERR_BAD_ARG
        assert f(c=3, ss=35, ds=36) == _capi.PRL_ERR_BAD_ARG
        assert f(w=32769, ss=40000, ds=40000) == _capi.PRL_ERR_BAD_ARG and f(h=32769) == _capi.PRL_ERR_BAD_ARG
        assert f(k=65537) == _capi.PRL_ERR_BAD_ARG
    assert dev(n=-1) == _capi.PRL_ERR_BAD_ARG
    assert dev(n=0) == _capi.PRL_OK
    # any overlap of source and destination other than the same pages at the same strides
    assert L.prl_hip_median_batch_device(2, 1, 3, 1, s, 96, 12, 12, 8, s + 12, 96, 12, None) == _capi.PRL_ERR_BAD_ARG
    assert src.max() == 0 and dst.max() == 0


def test_valid_call_without_a_device(prl):
    import torch

    from prlib_amd import _capi

    if torch.cuda.is_available():
        pytest.skip("a device is present; the no-device behaviour is checked on the CPU box")
    img = np.zeros((8, 12, 3), np.uint8)
    out = np.zeros_like(img)
    for k, times in ((3, 1), (1, 1), (3, 0), (9, 2)):
        st = _capi.lib().prl_hip_median_host(3, k, times, img.ctypes.data, 36, 12, 8, out.ctypes.data, 36)
        assert st == _capi.PRL_ERR_NO_DEVICE, (k, times)
    with pytest.raises(_capi.PrlError) as e:
        prl.denoiseSaltPepper(img, 3, 1)
    assert e.value.status == _capi.PRL_ERR_NO_DEVICE
    with pytest.raises(_capi.PrlError) as e:
        prl.denoiseSaltPepper(img, 4, 1)
    assert e.value.status == _capi.PRL_ERR_BAD_WINDOW


def build_dropin(out_dir):
    """g++ of tests/cpp/test_median_dropin.cpp + prl_host.cpp, with only -I include/prl for the drop-in header."""
    exe = os.path.join(out_dir, "test_median_dropin")
    flags = []
    for pc in ("opencv4", "opencv"):
        r = subprocess.run(["pkg-config", "--cflags", "--libs", pc], capture_output=True, text=True) if shutil.which("pkg-config") else None
        if r is not None and r.returncode == 0:
            flags = r.stdout.split()
            break
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include", "prl"),
           os.path.join(ROOT, "tests", "cpp", "test_median_dropin.cpp"), os.path.join(ROOT, "prlib_amd", "csrc", "prl", "prl_host.cpp"),
           ] + flags + ["-L", os.path.join(ROOT, "prlib_amd"), "-lprlib_hip", "-Wl,-rpath," + os.path.join(ROOT, "prlib_amd"),
                        "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_dropin_header_contract_without_device(prl, tmp_path):
    import torch

    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    exe = build_dropin(str(tmp_path))
    if torch.cuda.is_available():
        pytest.skip("a device is present; the no-device behaviour is checked on the CPU box")
    r = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "median dropin cpu: OK" in r.stdout, r.stdout + r.stderr
