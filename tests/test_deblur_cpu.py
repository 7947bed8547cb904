"""prl::basicDeblur and the float32 cv::GaussianBlur under it without a device: the weights and the size rule of the C ABI against
tests/deblur_ref.py bit for bit, deblur_ref against a float64 scipy model within a derived distance and against an independently
written sample-by-sample loop, gauss.h's plain loops (a stand-alone g++ program, once more under the address and undefined-behaviour
sanitizers) against deblur_ref bit for bit, the C ABI's statuses in their documented order, the exports, and the drop-in header's
C++ contract."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import adaptive_ref
import deblur_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("prl_hip_basic_deblur_batch_device", "prl_hip_basic_deblur_host", "prl_hip_gaussian_blur_f32_batch_device",
           "prl_hip_gaussian_blur_f32_host", "prl_hip_gaussian_blur_size", "prl_hip_gaussian_kernel_f32")
WEIGHT_CASES = [(n, s) for n in (1, 3, 5, 7) for s in (0.0, -1.0)] + [(n, s) for n in (1, 3, 5, 7) for s in (0.6, 1.0, 9.0)] + \
               [(n, s) for n in (9, 73, 255) for s in (0.0, -2.0, 1.0, 9.0, 31.75)]


# ---- the weights and the size rule ------------------------------------------------------------------------------------------

def _c_kernel(L, n, sigma):
    w = np.full(n, -7.0, np.float32)
    assert L.prl_hip_gaussian_kernel_f32(n, sigma, w.ctypes.data) == 0
    return w


def test_weights_equal_the_restatement(prl):
    from prlib_amd import _capi

    L = _capi.lib()
    for n, sigma in WEIGHT_CASES:
        want = dr.kernel(n, sigma)
        assert want.dtype == np.float32 and len(want) == n
        assert dr.same_bits(_c_kernel(L, n, sigma), want), (n, sigma)
        assert dr.same_bits(prl.gaussianKernelF32(n, sigma), want), (n, sigma)
        assert dr.same_bits(want, want[::-1]), (n, sigma)                         # symmetric bit for bit
        assert abs(float(want.astype(np.float64).sum()) - 1.0) < n * 2.0 ** -24
    for n in (3, 5, 7):   # the tables apply only without a sigma
        assert not dr.same_bits(dr.kernel(n, 0.0), dr.kernel(n, ((n - 1) * 0.5 - 1) * 0.3 + 0.8)), n
        assert dr.kernel(n, 0.0).tolist() == dr._TABLES[n]
    assert dr.kernel(1, 0.0).tolist() == [1.0] and dr.kernel(1, 5.0).tolist() == [1.0]
    for bs in (3, 5, 7, 9, 19, 73, 255):   # cv::adaptiveThreshold's Gaussian is this routine without a sigma
        assert dr.same_bits(dr.kernel(bs, 0.0), adaptive_ref.gauss_weights(bs)), bs
        assert dr.same_bits(prl.gaussianKernelF32(bs), adaptive_ref.gauss_weights(bs)), bs
    W, A = _capi.PRL_ERR_BAD_WINDOW, _capi.PRL_ERR_BAD_ARG
    w = np.full(300, 3.0, np.float32)
    for n in (0, -1, 2, 4, 256, 257, 1 << 20):
        assert L.prl_hip_gaussian_kernel_f32(n, 1.0, w.ctypes.data) == W, n
        assert L.prl_hip_gaussian_kernel_f32(n, float("nan"), None) == W, n
    assert L.prl_hip_gaussian_kernel_f32(3, 1.0, None) == A
    assert L.prl_hip_gaussian_kernel_f32(3, float("nan"), w.ctypes.data) == A and L.prl_hip_gaussian_kernel_f32(3, float("inf"), w.ctypes.data) == A
    assert w.tolist() == [3.0] * 300


def _c_size(L, kw, kh, sx, sy):
    a, b = ctypes.c_int(-5), ctypes.c_int(-5)
    st = L.prl_hip_gaussian_blur_size(kw, kh, sx, sy, ctypes.byref(a), ctypes.byref(b))
    return st, a.value, b.value


def test_size_rule(prl):
    from prlib_amd import _capi

    L = _capi.lib()
    W, A = _capi.PRL_ERR_BAD_WINDOW, _capi.PRL_ERR_BAD_ARG
    assert _c_size(L, 0, 0, 9.0, 0.0) == (0, 73, 73) and dr.plan(0, 0, 9.0, 0.0)[:2] == (73, 73)
    assert _c_size(L, 0, 0, 1.0, 3.0) == (0, 9, 25) and dr.plan(0, 0, 1.0, 3.0) == (9, 25, 1.0, 3.0, False)
    assert _c_size(L, 5, 5, 9.0, 0.0) == (0, 5, 5)
    assert dr.plan(5, 5, 9.0, 0.0) == (5, 5, 9.0, 9.0, True)                 # ... and its weights come from exp, not from the table
    assert dr.same_bits(dr.kernels(5, 5, 9.0, 0.0)[0], dr.kernel(5, 9.0)) and not dr.same_bits(dr.kernel(5, 9.0), dr.kernel(5, 0.0))
    assert _c_size(L, 0, 0, 0.0, 0.0)[0] == W and dr.plan(0, 0, 0.0, 0.0)[:2] == (None, None)
    for sx, sy in ((1.0, 1.0), (0.0, 0.0), (9.0, 0.0)):
        assert _c_size(L, 4, 4, sx, sy)[0] == W and dr.plan(4, 4, sx, sy)[:2] == (None, None)
    assert _c_size(L, -3, 0, 0.5, 0.0) == (0, 5, 5)                              # cvRound(5.0) | 1
    assert _c_size(L, 0, 0, 0.3, 0.0) == (0, 3, 3)                               # cvRound(3.4) | 1
    assert _c_size(L, 0, 0, 0.4375, 0.0) == (0, 5, 5)                            # cvRound(4.5) = 4 (half to even), | 1
    assert _c_size(L, 0, 0, 0.6875, 0.0) == (0, 7, 7)                            # cvRound(6.5) = 6, | 1
    assert _c_size(L, 3, 0, 0.0, 0.0)[0] == W and _c_size(L, 0, 3, 0.0, 2.0)[0] == W   # one side underivable
    assert _c_size(L, 0, 7, -1.0, 2.0)[0] == W and _c_size(L, 7, 0, -1.0, 2.0) == (0, 7, 17)
    assert _c_size(L, 255, 255, 0.0, 0.0) == (0, 255, 255) and _c_size(L, 257, 3, 0.0, 0.0)[0] == W
    assert _c_size(L, 0, 0, 31.75, 0.0) == (0, 255, 255) and _c_size(L, 0, 0, 32.0, 0.0)[0] == W   # 8 sigma + 1 = 257
    assert _c_size(L, (1 << 32) | 3, 3, 1.0, 1.0)[0] == W and _c_size(L, 3, -(1 << 40), 1.0, 1.0)[0] == W
    assert _c_size(L, 0, 0, float("nan"), 0.0)[0] == W and _c_size(L, 0, 0, float("inf"), 0.0)[0] == W
    assert _c_size(L, 3, 3, float("nan"), 0.0)[0] == A and _c_size(L, 3, 3, 1.0, float("inf"))[0] == A
    assert L.prl_hip_gaussian_blur_size(3, 3, 1.0, 1.0, None, None) == A
    assert prl.gaussianBlurSize((0, 0), 1.0, 3.0) == (9, 25) and prl.gaussianBlurSize() == (73, 73)
    for kw, kh, sx, sy in ((0, 0, 9.0, 0.0), (0, 0, 1.0, 3.0), (7, 3, 0.0, 0.0), (0, 5, 2.5, -1.0), (0, 0, 0.3, 7.1)):
        assert _c_size(L, kw, kh, sx, sy)[1:] == dr.plan(kw, kh, sx, sy)[:2], (kw, kh, sx, sy)


# ---- the restatement itself --------------------------------------------------------------------------------------------------

def test_reflect101():
    assert [dr.reflect101(i, 5) for i in (-2, -1, 0, 4, 5, 6)] == [2, 1, 0, 4, 3, 2]
    assert [dr.reflect101(i, 3) for i in range(-6, 9)] == [2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0]
    assert [dr.reflect101(i, 2) for i in (-3, -2, -1, 0, 1, 2, 3)] == [1, 0, 1, 0, 1, 0, 1]
    assert [dr.reflect101(i, 1) for i in (-40, -1, 0, 1, 40)] == [0] * 5


def test_known_answers():
    page = np.array([[10, 20, 30, 40, 250]], np.uint8)
    g = dr.blur(page, (3, 3), 0.0, 0.0)
    assert g.tolist() == [[15.0, 20.0, 30.0, 90.0, 145.0]]                         # the border is 20 | 10 ... 250 | 40
    assert dr.blur(page.T.copy(), (3, 3), 0.0, 0.0).T.tolist() == g.tolist()
    assert dr.deblur(page, 3, 0.0, 0.0, 0.75).tolist() == [[8, 20, 30, 15, 255]]   # 7.5 -> 8 (half to even), 302.5 -> 255
    assert dr.deblur(page, 3, 0.0, 0.0, 0.5).tolist() == [[0, 0, 0, 0, 105]]
    assert dr.deblur(page, 3, 0.0, 0.0, 1.0).tolist() == [[20, 40, 60, 80, 255]]   # beta = 0
    assert dr.deblur(page, 3, 0.0, 0.0, 0.0).tolist() == [[0] * 5]
    assert dr.deblur(page, 1, 0.0, 0.0, 0.75).tolist() == page.tolist()            # 1 x 1: g = x, and 1.5 x - 0.5 x = x
    assert dr.same_bits(dr.blur(page, (1, 1), 4.0, 0.0), page.astype(np.float32))
    assert dr.sat_u8(np.array([0.5, 1.5, 2.5, -0.5, 254.5, 255.5, 1e9, 3e9, -3e9, np.nan, np.inf], np.float32)).tolist() == \
        [0, 2, 2, 0, 254, 255, 255, 0, 0, 0, 0]
    for v in (0, 255):   # a flat page stays flat wherever the weights sum to 1 in float32; the defaults keep it within a byte
        out = dr.deblur(dr.flat(9, 11, v), 0, 9.0, 0.0, 0.75)
        assert np.abs(out.astype(int) - v).max() <= 1


@pytest.mark.parametrize("case", [((3, 3), 0.0, 0.0), ((5, 5), 0.0, 0.0), ((5, 5), 9.0, 0.0), ((7, 7), 0.0, 0.0), ((9, 25), 1.0, 3.0),
                                  ((1, 9), 0.0, 0.0), ((9, 1), 2.0, 0.0), ((0, 0), 1.0, 0.0), ((25, 25), 0.0, 0.0)], ids=str)
def test_ref_equals_the_sample_by_sample_loop(case):
    ksize, sx, sy = case
    for h, w in ((1, 1), (1, 5), (5, 1), (2, 3), (3, 2), (6, 7), (13, 9)):
        page = dr.noise(h, w, 1, 4)
        assert dr.same_bits(dr.blur(page, ksize, sx, sy), dr.blur_loop(page, ksize, sx, sy)), (case, h, w)


def _gamma(k):
    u = 2.0 ** -24
    return k * u / (1 - k * u)


@pytest.mark.parametrize("case", [((3, 3), 0.0, 0.0), ((5, 5), 1.5, 0.0), ((9, 25), 1.0, 3.0), ((0, 0), 9.0, 0.0), ((255, 255), 0.0, 0.0),
                                  ((1, 9), 0.0, 0.0), ((73, 1), 9.0, 0.0)], ids=str)
def test_ref_against_float64(case):
    """scipy.ndimage.correlate1d(mode="mirror") (d c b | a b c d | c b a: REFLECT_101) in float64 with the float32 weights taken as
    exact numbers.  The allowed distance follows from the tap counts: a pass of n taps makes at most n products and n - 1 sums (and,
    in the pair forms, one more sum per term) of non-negative terms, each within u = 2^-24 relative, so its result is within
    gamma(n + 1) = (n + 1) u / (1 - (n + 1) u) of the exact sum of what it was given, and that sum is at most 255 Sx (Sx, Sy: the
    sums of the weights).  Two passes: |g - G| <= 255 Sx Sy ((1 + gamma(nx + 1)) (1 + gamma(ny + 1)) - 1)."""
    ndi = pytest.importorskip("scipy.ndimage")
    ksize, sx, sy = case
    wx, wy = dr.kernels(ksize[0], ksize[1], sx, sy)
    s_x, s_y = float(wx.astype(np.float64).sum()), float(wy.astype(np.float64).sum())
    bound = 255.0 * s_x * s_y * ((1 + _gamma(len(wx) + 1)) * (1 + _gamma(len(wy) + 1)) - 1) + 1e-9
    worst = 0.0
    for h, w in ((2, 2), (3, 7), (7, 3), (40, 33), (64, 90)):
        for page in (dr.noise(h, w, 1, 2), dr.checkerboard(h, w), dr.flat(h, w, 255)):
            exact = ndi.correlate1d(ndi.correlate1d(page.astype(np.float64), wx.astype(np.float64), axis=1, mode="mirror"),
                                    wy.astype(np.float64), axis=0, mode="mirror")
            err = float(np.abs(dr.blur(page, ksize, sx, sy).astype(np.float64) - exact).max())
            worst = max(worst, err)
            assert err <= bound, (case, h, w, err, bound)
    print("float64 distance", case, "worst", worst, "bound", bound)
    assert bound < 255 * 2 * 258 * 2.0 ** -24   # the bound itself is small: 8e-3 for the largest kernel


# ---- gauss.h on the CPU --------------------------------------------------------------------------------------------------------

def _build(tmp, name, extra):
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    exe = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-ffp-contract=off"] + extra +
                       [os.path.join(ROOT, "tests", "cpp", "test_deblur.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def deblur_exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("deblur"), "test_deblur", [])


def _padded(page, pad, tmp_path):
    p3 = page if page.ndim == 3 else page[:, :, None]
    h, w, c = p3.shape
    buf = np.full((h, w * c + pad), 0xAB, np.uint8)
    buf[:, :w * c] = p3.reshape(h, w * c)
    path = os.path.join(str(tmp_path), "page.raw")
    buf.tofile(path)
    return h, w, c, path


def _run_blur(exe, page, ksize, sx, sy, tmp_path, pad=0):
    h, w, c, path = _padded(page, pad, tmp_path)
    out = os.path.join(str(tmp_path), "out.raw")
    r = subprocess.run([exe, "blur", str(h), str(w), str(c), str(ksize[0]), str(ksize[1]), repr(sx), repr(sy), str(w * c + pad), path, out],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    return np.fromfile(out, np.float32).reshape(page.shape)


def _run_deblur(exe, page, k, sx, sy, weight, tmp_path, pad=0):
    h, w, c, path = _padded(page, pad, tmp_path)
    out = os.path.join(str(tmp_path), "out.raw")
    r = subprocess.run([exe, "deblur", str(h), str(w), str(c), str(k), repr(sx), repr(sy), repr(weight), str(w * c + pad), path, out],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    return np.fromfile(out, np.uint8).reshape(page.shape)


def test_header_self_check(deblur_exe):
    r = subprocess.run([deblur_exe, "self"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "deblur self: OK" in r.stdout, r.stdout + r.stderr


def test_header_weights_equal_the_restatement(deblur_exe):
    for n, sigma in WEIGHT_CASES:
        r = subprocess.run([deblur_exe, "weights", str(n), repr(sigma)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0
        got = np.array([int(v, 16) for v in r.stdout.split()], np.uint32).view(np.float32)
        assert dr.same_bits(got, dr.kernel(n, sigma)), (n, sigma)


@pytest.mark.parametrize("channels", (1, 2, 3, 4))
def test_plain_loop_equals_ref(deblur_exe, tmp_path, channels):
    sizes = [(1, 1), (1, 7), (7, 1), (2, 3), (3, 2), (9, 13), (40, 33)]
    for i, (h, w) in enumerate(sizes):
        page = dr.noise(h, w, channels, 5) if i % 2 else dr.checkerboard(h, w, channels)
        for ksize, sx, sy in (((0, 0), 9.0, 0.0), ((3, 3), 0.0, 0.0), ((5, 5), 0.0, 0.0), ((5, 5), 9.0, 0.0), ((7, 7), 0.0, 0.0), ((9, 25), 1.0, 3.0),
                              ((1, 9), 0.0, 0.0), ((9, 1), 0.0, 0.0), ((1, 1), 0.0, 0.0)):
            got = _run_blur(deblur_exe, page, ksize, sx, sy, tmp_path, pad=(h + w) % 3)
            assert dr.same_bits(got, dr.blur(page, ksize, sx, sy)), (h, w, channels, ksize, sx, sy)
        for k, sx, weight in ((0, 9.0, 0.75), (0, 9.0, 0.5), (3, 0.0, 1.0), (5, 1.0, 2.0), (7, 0.0, 0.0), (1, 0.0, 0.75), (0, 9.0, 1e30), (3, 0.0, -4.0)):
            got = _run_deblur(deblur_exe, page, k, sx, 0.0, weight, tmp_path, pad=(h * w) % 2)
            assert np.array_equal(got, dr.deblur(page, k, sx, 0.0, weight)), (h, w, channels, k, sx, weight)
    big = dr.noise(30, 41, channels, 6)
    assert dr.same_bits(_run_blur(deblur_exe, big, (255, 255), 0.0, 0.0, tmp_path), dr.blur(big, (255, 255), 0.0, 0.0))


def test_plain_loop_under_the_sanitizers(tmp_path):
    """the stand-alone program on pages narrower and shorter than the radius, with address and undefined-behaviour checks"""
    # (the runtimes linked statically: the program does not depend on where the loader finds them)
    exe = _build(tmp_path, "test_deblur_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                                               "-static-libubsan"])
    for mode in ("narrow", "self"):
        r = subprocess.run([exe, mode], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "deblur %s: OK" % mode in r.stdout, r.stdout + r.stderr[-3000:]


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------

def test_declared_and_exported(prl):
    from prlib_amd import _capi

    header = open(os.path.join(ROOT, "include", "prl_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _capi.EXPORTED_SYMBOLS
        for m in ("prl_hip.map", "prl_hip_testhooks.map"):
            assert re.search(r"\b" + name + r";", open(os.path.join(ROOT, "prlib_amd", "csrc", m)).read()), (name, m)
    assert re.search(r"#define PRL_HIP_ABI_VERSION 4\b", header)
    assert re.search(r"#define PRL_GAUSS_MAX_SIDE %d\b" % dr.MAX_SIDE, header) and prl.deblur.MAX_SIDE == dr.MAX_SIDE
    for f in ("basicDeblur", "gaussianBlurF32", "gaussianKernelF32"):
        assert callable(getattr(prl, f)) and f in prl.__all__, f
    r = subprocess.run(["python", os.path.join(ROOT, "tools", "gen_export_map.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    assert os.path.exists(os.path.join(ROOT, "include", "prl", "basicDeblur.h"))
    assert "prl_hip_basic_deblur_batch_device" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for build_file in ("CMakeLists.txt", os.path.join("prlib_amd", "csrc", "Makefile")):
        assert re.search(r"\bdeblur\b", open(os.path.join(ROOT, build_file)).read()), build_file
    if shutil.which("nm") is None:
        return
    for lib in ("libprlib_hip.so", "libprlib_hip_testhooks.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "prlib_amd", lib)], capture_output=True, text=True,
                             check=True).stdout
        for name in SYMBOLS:
            assert re.search(r"\bT " + name + r"\b", out), (lib, name)


def test_statuses_in_their_order_without_touching_a_device(prl):
    import torch

    from prlib_amd import _capi

    L = _capi.lib()
    no_gpu = not torch.cuda.is_available()   # a valid device call on these host arrays must never reach a device
    buf = np.zeros(1 << 16, np.uint8)
    out = np.zeros(1 << 18, np.uint8)
    s, o = buf.ctypes.data, out.ctypes.data
    assert o % 4 == 0
    E, W, A = _capi.PRL_ERR_EMPTY, _capi.PRL_ERR_BAD_WINDOW, _capi.PRL_ERR_BAD_ARG
    nan, inf = float("nan"), float("inf")

    def fused_dev(n=1, c=1, k=0, sx=9.0, sy=0.0, wt=0.75, src=s, ss=256, w=64, h=60, dst=o, ds=256, spage=256 * 60, dpage=256 * 60):
        return L.prl_hip_basic_deblur_batch_device(n, c, k, sx, sy, wt, src, spage, ss, w, h, dst, dpage, ds, None)

    def fused_host(n=1, c=1, k=0, sx=9.0, sy=0.0, wt=0.75, src=s, ss=256, w=64, h=60, dst=o, ds=256, **_):
        return L.prl_hip_basic_deblur_host(c, k, sx, sy, wt, src, ss, w, h, dst, ds)

    def blur_dev(n=1, c=1, k=0, sx=9.0, sy=0.0, wt=0.75, src=s, ss=256, w=64, h=60, dst=o, ds=1024, spage=256 * 60, dpage=1024 * 60):
        return L.prl_hip_gaussian_blur_f32_batch_device(n, c, k, k, sx, sy, src, spage, ss, w, h, dst, dpage, ds, None)

    def blur_host(n=1, c=1, k=0, sx=9.0, sy=0.0, wt=0.75, src=s, ss=256, w=64, h=60, dst=o, ds=1024, **_):
        return L.prl_hip_gaussian_blur_f32_host(c, k, k, sx, sy, src, ss, w, h, dst, ds)

    for f in (fused_dev, fused_host, blur_dev, blur_host):
        dev, f32 = f in (fused_dev, blur_dev), f in (blur_dev, blur_host)
        assert f(w=0) == E and f(h=-1) == E and f(w=0, k=4, c=9, src=None, sx=nan) == E                        # 1. empty
        for bad in (dict(k=4), dict(k=2), dict(k=257), dict(k=0, sx=0.0), dict(k=0, sx=-1.0), dict(k=0, sx=nan), dict(k=0, sx=32.0),   # 2. the window
                    dict(k=0, sx=inf), dict(k=(1 << 32) | 3), dict(k=0, sx=1.0, sy=40.0)):
            assert f(**bad) == W and f(c=9, **bad) == W and f(src=None, **bad) == W and f(ss=1, **bad) == W, bad
        for c in (0, 5, -1):                                                                                  # 3. the rest
            assert f(c=c) == A and f(c=c, src=None) == A, c
        assert f(k=3, sx=nan) == A and f(k=3, sx=inf) == A and f(k=3, sy=nan) == A and f(k=3, sx=1.0, sy=inf) == A
        if not f32:
            assert f(wt=nan) == A and f(wt=inf) == A and f(wt=-inf) == A
        assert f(src=None) == A and f(dst=None) == A and f(ss=63) == A and f(c=3, ss=191) == A
        assert f(ds=(64 * 4 - 1) if f32 else 63) == A and f(c=4, ds=(1023 if f32 else 255)) == A
        assert f(w=32769, ss=1 << 18, ds=1 << 20) == A and f(h=32769) == A
        if f32:
            assert f(dst=o + 2) == A and f(ds=1026) == A
            if dev:
                assert f(n=2, dpage=1024 * 60 + 2) == A
        # source and destination may not share a byte: in place, from the source's last byte, a destination inside a source row's padding
        assert f(dst=s, ds=256 * (4 if f32 else 1)) == A
        assert f(dst=s + 15 * 256 + 60, ds=256 * (4 if f32 else 1), h=16) == A
        assert f(dst=s + 128, w=16, h=4, ds=256 * (4 if f32 else 1)) == A
        if dev:
            assert f(n=-1) == A and f(n=0) == _capi.PRL_OK and f(n=0, src=None) == A and f(n=0, k=4) == W
        if no_gpu:
            for c in (1, 2, 3, 4):
                for k, sx in ((0, 9.0), (1, 0.0), (255, 0.0), (0, 31.75), (5, 1.0)):
                    assert f(c=c, k=k, sx=sx, ss=256, ds=1024) == _capi.PRL_ERR_NO_DEVICE, (c, k)
    assert buf.max() == 0 and out.max() == 0


def test_valid_call_without_a_device(prl):
    import torch

    from prlib_amd import _capi

    if torch.cuda.is_available():
        pytest.skip("a device is present; the no-device behaviour is checked on the CPU box")
    img = np.zeros((60, 64, 3), np.uint8)
    for call in (lambda: prl.basicDeblur(img), lambda: prl.basicDeblur(img[:, :, 0]), lambda: prl.gaussianBlurF32(img), lambda: prl.gaussianBlurF32(img, (9, 25), 1.0, 3.0)):
        with pytest.raises(_capi.PrlError) as e:
            call()
        assert e.value.status == _capi.PRL_ERR_NO_DEVICE
    with pytest.raises(_capi.PrlError) as e:
        prl.basicDeblur(img, 4)
    assert e.value.status == _capi.PRL_ERR_BAD_WINDOW
    with pytest.raises(_capi.PrlError) as e:
        prl.basicDeblur(img, out=img)
    assert e.value.status == _capi.PRL_ERR_BAD_ARG
    with pytest.raises(_capi.PrlError) as e:
        prl.basicDeblur(img, imageWeight=float("nan"))
    assert e.value.status == _capi.PRL_ERR_BAD_ARG


# ---- the C++ drop-in ---------------------------------------------------------------------------------------------------------------

def build_dropin(out_dir):
    """g++ of tests/cpp/test_deblur_dropin.cpp + prl_host.cpp, with only -I include/prl for the drop-in header."""
    exe = os.path.join(out_dir, "test_deblur_dropin")
    flags = []
    for pc in ("opencv4", "opencv"):
        r = subprocess.run(["pkg-config", "--cflags", "--libs", pc], capture_output=True, text=True) if shutil.which("pkg-config") else None
        if r is not None and r.returncode == 0:
            flags = r.stdout.split()
            break
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include", "prl"),
           os.path.join(ROOT, "tests", "cpp", "test_deblur_dropin.cpp"), os.path.join(ROOT, "prlib_amd", "csrc", "prl", "prl_host.cpp"),
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
    assert r.returncode == 0 and "deblur dropin cpu: OK" in r.stdout, r.stdout + r.stderr
