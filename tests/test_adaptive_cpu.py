"""The adaptive-threshold binarizers without a device: the restatement (tests/adaptive_ref.py) against its per-pixel model
and scipy, the known answers of the canonical arithmetic, the C ABI's statuses, their order and the exports, and the drop-in
headers' C++ contract."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import zlib

import numpy as np
import pytest

import adaptive_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("prl_hip_adaptive_threshold_batch_device", "prl_hip_adaptive_threshold_host", "prl_hip_default_adaptive_params",
               "prl_hip_binarize_adaptive_batch_device", "prl_hip_binarize_adaptive_host")
SMALL_SHAPES = [(1, 1), (1, 9), (9, 1), (2, 3), (5, 4), (13, 17)]


def crc(a):
    return "%08x" % (zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF)


def _page(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


@pytest.mark.parametrize("bs", [3, 5, 7, 9, 19])
def test_restatement_equals_pixel_loop(bs):
    """1 x 1, 1 x N, N x 1 and pages smaller than the block included"""
    for i, shape in enumerate(SMALL_SHAPES):
        g = _page(shape, 100 * bs + i)
        assert np.array_equal(ar.mean_gauss(g, bs), ar.mean_gauss_loop(g, bs)), ("gauss", bs, shape)
        assert np.array_equal(ar.mean_box(g, bs), ar.mean_box_loop(g, bs)), ("box", bs, shape)


def test_restatement_equals_pixel_loop_at_a_wide_block():
    g = _page((6, 7), 3)
    assert np.array_equal(ar.mean_gauss(g, 31), ar.mean_gauss_loop(g, 31))
    assert np.array_equal(ar.mean_box(g, 31), ar.mean_box_loop(g, 31))


@pytest.mark.parametrize("bs", [3, 5, 7, 19, 101, 255])
def test_box_mean_equals_scipy_integer_convolution(bs):
    nd = pytest.importorskip("scipy.ndimage")
    for i, shape in enumerate([(1, 1), (3, 40), (40, 3), (57, 61)]):
        g = _page(shape, 7 * bs + i)
        s = nd.convolve(g.astype(np.int64), np.ones((bs, bs), np.int64), mode="nearest")
        assert np.array_equal(s, ar.block_sum(g, bs)), (bs, shape)
        want = np.clip(np.rint(s * (1.0 / (bs * bs))), 0, 255).astype(np.uint8)
        assert np.array_equal(ar.mean_box(g, bs), want)
        assert np.array_equal(ar.mean_box_integer(g, bs), want), "(2 S + bs^2) // (2 bs^2) is the same byte"


def test_weights():
    for bs in (3, 5, 7, 9, 19, 101, 255):
        w = ar.gauss_weights(bs)
        assert w.dtype == np.float32 and len(w) == bs and np.array_equal(w, w[::-1]), bs   # symmetric bit for bit
        assert abs(float(w.astype(np.float64).sum()) - 1.0) < 1e-6
    assert ar.gauss_weights(7).tolist() == [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]


KNOWN = {
    "synth": {"gauss": {3: "3181fdfc", 7: "0a27a911", 19: "c4946ead", 101: "e76bf804"},
              "box": {3: "fcb6c56f", 7: "5d9f4f60", 19: "ba6bde89", 101: "1cf0948f"}, "white": 0.9366, "mask": "b760b577"},
    "noise": {"gauss": {3: "047c5206", 7: "ad35411c", 19: "22080b4c", 101: "5acf7e43"},
              "box": {3: "cbd626dd", 7: "46c36b7b", 19: "3d01c1b3", 101: "79d99659"}, "white": 0.6641, "mask": "ce08d311"},
}


def known_pages():
    from prlib_amd import synth

    return {"synth": synth.page_numpy(300, 200, index=3),
            "noise": np.random.default_rng(7).integers(0, 256, (300, 200), dtype=np.uint8)}


def test_known_mean_planes():
    for name, g in known_pages().items():
        for bs in (3, 7, 19, 101):
            assert crc(ar.mean_gauss(g, bs)) == KNOWN[name]["gauss"][bs], (name, "gauss", bs)
            assert crc(ar.mean_box(g, bs)) == KNOWN[name]["box"][bs], (name, "box", bs)


def test_known_native_adaptive_defaults():
    for name, g in known_pages().items():
        unflipped = ar.adaptive_threshold(ar.median_ref.denoise_salt_pepper(g, 5, 1), 255.0, ar.GAUSSIAN_C, ar.BINARY_INV, 19, 9.0)
        assert ar.flips(unflipped), name
        m = ar.binarize_native_adaptive(g)
        assert np.array_equal(m, 255 - unflipped)
        assert round(float((m == 255).mean()), 4) == KNOWN[name]["white"], name
        assert crc(m) == KNOWN[name]["mask"], name


def test_flat_pages():
    for v in (0, 1, 127, 254, 255):
        g = np.full((40, 50), v, np.uint8)
        for bs in (3, 7, 19, 101):
            assert (ar.mean_gauss(g, bs) == v).all() and (ar.mean_box(g, bs) == v).all(), (v, bs)
    flat = np.full((30, 40), 77, np.uint8)
    for delta, binary, inv in ((0.5, 255, 255), (-0.5, 0, 255), (1.0, 255, 0)):
        assert (ar.adaptive_threshold(flat, 255, ar.MEAN_C, ar.BINARY, 3, delta) == binary).all(), delta
        assert (ar.adaptive_threshold(flat, 255, ar.MEAN_C, ar.BINARY_INV, 3, delta) == inv).all(), delta


def test_flip_boundary():
    flat = np.full((30, 40), 77, np.uint8)
    for mv, unflipped, final in ((128.0, 128, 128), (127.0, 127, 128), (127.5, 128, 128), (128.5, 128, 128)):
        m = ar.adaptive_threshold(flat, mv, ar.GAUSSIAN_C, ar.BINARY_INV, 19, 0.0)
        assert (m == unflipped).all(), mv
        assert ar.flips(m) == (unflipped < 128)
        assert (ar.adaptive_threshold(flat, mv, ar.GAUSSIAN_C, ar.BINARY_INV, 19, 0.0, auto_invert=True) == final).all(), mv
    assert (ar.adaptive_threshold(flat, -1.0, ar.MEAN_C, ar.BINARY, 3, 0.0) == 0).all()
    assert (ar.adaptive_threshold(flat, -1.0, ar.MEAN_C, ar.BINARY, 3, 0.0, auto_invert=True) == 255).all()


def test_stripes_page_does_not_flip():
    s = ar.stripes_page()
    assert np.array_equal(ar.median_ref.denoise_salt_pepper(s, 5, 1), s)
    m = ar.adaptive_threshold(s, 255.0, ar.GAUSSIAN_C, ar.BINARY_INV, 19, 9.0)
    assert not ar.flips(m) and round(float((m == 255).mean()), 3) == 0.653
    assert np.array_equal(ar.binarize_native_adaptive(s), m)


def test_auto_block_size():
    assert ar.auto_block_size(4096, 4096) == 24      # even: the call must fail
    assert ar.auto_block_size(3508, 2480) == 19
    assert ar.auto_block_size(9, 11) == 7


def test_declared_and_exported(prl):
    from prlib_amd import _capi

    header = open(os.path.join(ROOT, "include", "prl_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _capi.EXPORTED_SYMBOLS
    assert re.search(r"^#define PRL_HIP_ABI_VERSION 4\b", header, flags=re.M), "additions only: the ABI version stays"
    for m in ("prl_hip.map", "prl_hip_testhooks.map"):
        text = open(os.path.join(ROOT, "prlib_amd", "csrc", m)).read()
        for name in NEW_SYMBOLS:
            assert re.search(r"^\s+" + name + r";$", text, flags=re.M), (m, name)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_export_map.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    for h in ("binarizeNativeAdaptive.h", "binarizeAT.h", "binarizeAGT.h", "binarizePureAdaptiveGaussian.h"):
        assert os.path.exists(os.path.join(ROOT, "include", "prl", h)), h
    for name in ("adaptiveThreshold", "binarizeNativeAdaptive", "binarizeAT", "binarizeAGT", "binarizePureAdaptiveGaussian"):
        assert callable(getattr(prl, name)) and name in prl.__all__
    if shutil.which("nm") is None:
        pytest.skip("binutils not installed")
    for lib in ("libprlib_hip.so", "libprlib_hip_testhooks.so"):
        path = os.path.join(ROOT, "prlib_amd", lib)
        if not os.path.exists(path):
            continue
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for name in NEW_SYMBOLS:
            assert re.search(r"\bT " + name + r"\b", out), (lib, name)


def test_default_params_are_the_reference_header(prl):
    from prlib_amd import _capi

    p = _capi.AdaptiveParams()
    _capi.lib().prl_hip_default_adaptive_params(C.byref(p))
    assert (p.median_ksize, p.median_on_color, p.method, p.type, p.max_value, p.block_size, p.delta, p.auto_invert) == \
        (5, 0, 1, 1, 255.0, 19, 9.0, 1)
    _capi.lib().prl_hip_default_adaptive_params(None)   # a null pointer is ignored
    assert C.sizeof(_capi.AdaptiveParams) == 40


def test_entry_statuses_without_a_device(prl):
    """Every status of the four entries and the order of the checks: each row breaks one more thing than the row that names
    the earlier status, and the earlier status wins."""
    from prlib_amd import _capi

    L = _capi.lib()
    E, W, CH, A = _capi.PRL_ERR_EMPTY, _capi.PRL_ERR_BAD_WINDOW, _capi.PRL_ERR_BAD_CHANNELS, _capi.PRL_ERR_BAD_ARG
    src = np.zeros((8, 12, 4), np.uint8)
    dst = np.zeros((8, 12), np.uint8)
    s, d = src.ctypes.data, dst.ctypes.data
    nan = float("nan")

    def bare_dev(n=1, method=0, type_=0, mv=255.0, bs=3, delta=0.0, inv=0, sp=s, ss=12, w=12, h=8, dp=d, ds=12, **_):
        return L.prl_hip_adaptive_threshold_batch_device(n, method, type_, mv, bs, delta, inv, sp, 96, ss, w, h, dp, 96, ds, None)

    def bare_host(method=0, type_=0, mv=255.0, bs=3, delta=0.0, inv=0, sp=s, ss=12, w=12, h=8, dp=d, ds=12, **_):
        return L.prl_hip_adaptive_threshold_host(method, type_, mv, bs, delta, inv, sp, ss, w, h, dp, ds)

    def params(med=5, on_color=0, method=1, type_=1, mv=255.0, bs=19, delta=9.0, inv=1):
        p = _capi.AdaptiveParams()
        p.median_ksize, p.median_on_color, p.method, p.type = med, on_color, method, type_
        p.max_value, p.block_size, p.delta, p.auto_invert = mv, bs, delta, inv
        return p

    def full_dev(n=1, c=1, sp=s, ss=None, w=12, h=8, dp=d, ds=12, null_params=False, **kw):
        p = params(**kw)
        return L.prl_hip_binarize_adaptive_batch_device(None if null_params else C.byref(p), n, c, sp, 96 * 4, 12 * c if ss is None else ss,
                                                        w, h, dp, 96, ds, None)

    def full_host(c=1, sp=s, ss=None, w=12, h=8, dp=d, ds=12, null_params=False, **kw):
        p = params(**kw)
        return L.prl_hip_binarize_adaptive_host(None if null_params else C.byref(p), c, sp, 12 * c if ss is None else ss, w, h, dp, ds)

    for f in (bare_dev, bare_host, full_dev, full_host):
        full = f in (full_dev, full_host)
        # PRL_ERR_EMPTY first, whatever else is wrong
        assert f(w=0) == E and f(h=-1) == E and f(w=0, bs=4, sp=None) == E
        # block size: even, < 3, above the documented limit of 255; before the pointers and the values
        for bs in (4, 2, 1, 0, -3, 20, 257, 1001):
            assert f(bs=bs) == W, bs
        assert f(bs=4, sp=None) == W and f(bs=4, mv=nan) == W and f(bs=4, method=7) == W
        for bs in (3, 255):
            assert f(bs=bs, sp=None) == A   # a good block size gets as far as the pointers
        # PRL_ERR_BAD_ARG
        assert f(sp=None) == A and f(dp=None) == A
        assert f(ss=11) == A and f(ds=11) == A
        assert f(w=32769, ss=200000, ds=40000) == A and f(h=32769) == A
        assert f(method=2) == A and f(method=-1) == A and f(type_=2) == A and f(type_=-1) == A
        assert f(mv=nan) == A and f(delta=nan) == A
        if full:
            assert f(null_params=True) == A and f(null_params=True, w=0) == E
            # the median's window: after the block size, before the channels
            for med in (-1, 2, 4, -3):
                assert f(med=med) == W, med
            assert f(med=4, c=2) == W and f(med=4, bs=4) == W
            assert f(med=65537) == A
            for c in (0, 2, 5, -1):
                assert f(c=c, ss=64) == CH, c
            assert f(c=2, sp=None, ss=64) == CH   # channels before the pointers
            assert f(c=3, ss=35) == A and f(c=4, ss=47) == A
    assert bare_dev(n=-1) == A and full_dev(n=-1) == A
    assert bare_dev(n=0) == _capi.PRL_OK and full_dev(n=0) == _capi.PRL_OK
    # overlapping source and destination, in place included
    assert L.prl_hip_adaptive_threshold_batch_device(1, 0, 0, 255.0, 3, 0.0, 0, s, 96, 12, 12, 8, s, 96, 12, None) == A
    assert L.prl_hip_adaptive_threshold_batch_device(2, 0, 0, 255.0, 3, 0.0, 0, s, 96, 12, 12, 8, s + 100, 96, 12, None) == A
    assert src.max() == 0 and dst.max() == 0


def test_valid_calls_without_a_device(prl):
    import torch

    from prlib_amd import _capi

    if torch.cuda.is_available():
        pytest.skip("a device is present; the no-device behaviour is checked on the CPU box")
    gray = np.zeros((8, 12), np.uint8)
    bgr = np.zeros((8, 12, 3), np.uint8)
    out = np.zeros((8, 12), np.uint8)
    L = _capi.lib()
    for method in (0, 1):
        for type_ in (0, 1):
            for inv in (0, 1):
                st = L.prl_hip_adaptive_threshold_host(method, type_, -1.0, 255, 1e300, inv, gray.ctypes.data, 12, 12, 8, out.ctypes.data, 12)
                assert st == _capi.PRL_ERR_NO_DEVICE
    calls = [lambda: prl.adaptiveThreshold(gray, 255, 1, 0, 19, 9), lambda: prl.binarizeNativeAdaptive(gray), lambda: prl.binarizeNativeAdaptive(bgr),
             lambda: prl.binarizeNativeAdaptive(gray, adaptiveThresholdingBlockSize=0), lambda: prl.binarizeAT(bgr, 5, 255, 19, 9),
             lambda: prl.binarizeAGT(bgr, 1, 255, 19, 9), lambda: prl.binarizePureAdaptiveGaussian(bgr, 255, 19, 9)]
    for call in calls:
        with pytest.raises(_capi.PrlError) as e:
            call()
        assert e.value.status == _capi.PRL_ERR_NO_DEVICE


def test_python_layer_rejections(prl):
    from prlib_amd import _capi

    gray = np.zeros((8, 12), np.uint8)
    bgr = np.zeros((8, 12, 3), np.uint8)
    cases = [
        (lambda: prl.adaptiveThreshold(gray, 255, 0, 0, 4, 0), _capi.PRL_ERR_BAD_WINDOW),
        (lambda: prl.adaptiveThreshold(gray, float("nan"), 0, 0, 3, 0), _capi.PRL_ERR_BAD_ARG),
        (lambda: prl.binarizeNativeAdaptive(gray, adaptiveThresholdingMaxValue=256.0), _capi.PRL_ERR_BAD_ARG),
        (lambda: prl.binarizeNativeAdaptive(gray, adaptiveThresholdingMaxValue=float("nan")), _capi.PRL_ERR_BAD_ARG),
        (lambda: prl.binarizeNativeAdaptive(gray, medianBlurKernelSize=1), _capi.PRL_ERR_BAD_WINDOW),
        (lambda: prl.binarizeNativeAdaptive(gray, medianBlurKernelSize=4), _capi.PRL_ERR_BAD_WINDOW),
        (lambda: prl.binarizeNativeAdaptive(np.zeros((4096, 4096), np.uint8), adaptiveThresholdingBlockSize=0), _capi.PRL_ERR_BAD_WINDOW),
        (lambda: prl.binarizeAT(gray, 5, 255, 19, 9), _capi.PRL_ERR_BAD_CHANNELS),
        (lambda: prl.binarizeAGT(gray, 5, 255, 19, 9), _capi.PRL_ERR_BAD_CHANNELS),
        (lambda: prl.binarizePureAdaptiveGaussian(gray, 255, 19, 9), _capi.PRL_ERR_BAD_CHANNELS),
        (lambda: prl.binarizeAT(bgr, 4, 255, 19, 9), _capi.PRL_ERR_BAD_WINDOW),
        (lambda: prl.binarizeAGT(bgr, 5, 255, 20, 9), _capi.PRL_ERR_BAD_WINDOW),
        (lambda: prl.binarizeNativeAdaptive(np.zeros((8, 12, 2), np.uint8)), _capi.PRL_ERR_BAD_CHANNELS),
    ]
    for i, (call, status) in enumerate(cases):
        with pytest.raises(_capi.PrlError) as e:
            call()
        assert e.value.status == status, i
    with pytest.raises(NotImplementedError):
        prl.binarizeNativeAdaptive(gray, isGaussianBlurReqiured=True)
    with pytest.raises(NotImplementedError):
        prl.binarizeNativeAdaptive(gray, bilateralFilterBlockSize=3)


def build_dropin(out_dir):
    """g++ of tests/cpp/test_adaptive_dropin.cpp + prl_host.cpp, with only -I include/prl for the drop-in headers."""
    exe = os.path.join(out_dir, "test_adaptive_dropin")
    flags = []
    for pc in ("opencv4", "opencv"):
        r = subprocess.run(["pkg-config", "--cflags", "--libs", pc], capture_output=True, text=True) if shutil.which("pkg-config") else None
        if r is not None and r.returncode == 0:
            flags = r.stdout.split()
            break
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include", "prl"),
           os.path.join(ROOT, "tests", "cpp", "test_adaptive_dropin.cpp"), os.path.join(ROOT, "prlib_amd", "csrc", "prl", "prl_host.cpp"),
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
    assert r.returncode == 0 and "adaptive dropin cpu: OK" in r.stdout, r.stdout + r.stderr
