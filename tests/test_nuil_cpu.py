"""prl::correctNUIL and the flat-element morphology under it, without a device: the restatement (tests/nuil_ref.py) against
scipy and the per-pixel definition, the known answers of the elements and of whole pages, the C ABI's statuses in their
documented order, the exports, and the drop-in header's C++ contract."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import nuil_ref as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("prl_hip_morphology_batch_device", "prl_hip_morphology_host", "prl_hip_correct_nuil_batch_device",
           "prl_hip_correct_nuil_host")
PAGE_SHAPES = [(1, 1), (1, 9), (9, 1), (2, 2), (23, 31)]


def _img(shape, c, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, size=shape + (c,), dtype=np.uint8)
    return a[:, :, 0] if c == 1 and seed % 2 else a


@pytest.mark.parametrize("shape", nr.SHAPES)
@pytest.mark.parametrize("k", [(1, 1), (3, 3), (5, 5), (15, 15), (31, 31), (7, 3), (3, 9), (101, 101)])
def test_restatement_equals_scipy(shape, k):
    nd = pytest.importorskip("scipy.ndimage")
    kw, kh = k
    mask = nr.element_mask(shape, kw, kh)
    assert np.array_equal(mask, mask[::-1, ::-1])   # odd sizes: symmetric, so scipy's reflection of the footprint is moot
    for i, ps in enumerate(PAGE_SHAPES):
        for c in (1, 3):
            img = _img(ps, c, 5 * kw + kh + i + c)
            a = nr._as3(img)
            want_d = np.stack([nd.grey_dilation(a[:, :, ch], footprint=mask, mode="constant", cval=0) for ch in range(c)], axis=2)
            want_e = np.stack([nd.grey_erosion(a[:, :, ch], footprint=mask, mode="constant", cval=255) for ch in range(c)], axis=2)
            assert np.array_equal(nr._as3(nr.dilate(img, shape, kw, kh)), want_d), (shape, k, ps, c)
            assert np.array_equal(nr._as3(nr.erode(img, shape, kw, kh)), want_e), (shape, k, ps, c)


@pytest.mark.parametrize("op", nr.OPS)
@pytest.mark.parametrize("shape", nr.SHAPES)
def test_restatement_equals_pixel_loop(op, shape):
    for i, (kw, kh) in enumerate([(1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (2, 5), (6, 3), (7, 4), (1, 4), (4, 1), (15, 15)]):
        for c, ps in ((1, (8, 11)), (3, (5, 4)), (2, (1, 7))):
            img = _img(ps, c, 13 * i + c + op)
            assert np.array_equal(nr.morphology_ex(img, op, shape, kw, kh), nr.morphology_loop(img, op, shape, kw, kh)), (kw, kh, c)


def test_correct_nuil_equals_pixel_loop_and_its_bands():
    for size, c, ps in ((1, 1, (6, 7)), (2, 3, (6, 7)), (3, 2, (9, 8)), (4, 1, (9, 8)), (5, 4, (7, 9)), (15, 1, (12, 10))):
        img = _img(ps, c, size + c)
        img[:, :, ...] = img // (1 + (size % 2))    # some pages dark enough to be inverted
        assert np.array_equal(nr.correct_nuil(img, size), nr.correct_nuil_loop(img, size)), (size, c)
    tall = _img((150, 21), 3, 77)
    whole = nr.correct_nuil(tall, 7)
    for y0, y1 in ((0, 9), (60, 75), (141, 150)):
        assert np.array_equal(nr.correct_nuil_rows(tall, 7, y0, y1), whole[y0:y1])


def test_element_known_answers():
    assert np.array_equal(nr.element_mask(nr.ELLIPSE, 3, 3), nr.element_mask(nr.CROSS, 3, 3))
    assert ["".join("1" if v else "0" for v in r) for r in nr.element_mask(nr.ELLIPSE, 5, 5)] == \
        ["00100", "11111", "11111", "11111", "00100"]
    e31 = nr.element_mask(nr.ELLIPSE, 31, 31)
    assert e31[0].sum() == 1 and e31[30].sum() == 1 and e31[0, 15] and e31[30, 15] and e31[15].all()
    assert nr.element_mask(nr.RECT, 4, 3).all()
    cross = nr.element_mask(nr.CROSS, 4, 5)
    assert cross[2].all() and cross[:, 2].all() and cross.sum() == 4 + 5 - 1
    for shape in nr.SHAPES:
        assert nr.element_mask(shape, 1, 1).tolist() == [[True]]
    assert nr.cv_round(0.5) == 0 and nr.cv_round(1.5) == 2 and nr.cv_round(2.5) == 2 and nr.cv_round(2.4999) == 2
    with pytest.raises(ValueError):
        nr.element_spans(nr.ELLIPSE, 0, 0)
    # an even element is not reflected between erode and dilate: a single bright pixel grows towards -x / -y under dilate
    dot = np.zeros((5, 5), np.uint8)
    dot[2, 2] = 200
    assert np.argwhere(nr.dilate(dot, nr.RECT, 2, 2)).tolist() == [[2, 2], [2, 3], [3, 2], [3, 3]]
    hole = 255 - dot
    assert np.argwhere(nr.erode(hole, nr.RECT, 2, 2) < 255).tolist() == [[2, 2], [2, 3], [3, 2], [3, 3]]


def test_page_known_answers():
    for v in (0, 1, 127, 128, 200, 255):
        for c in (1, 3):
            flat = np.full((9, 12, c), v, np.uint8)
            assert (nr.correct_nuil(flat, 31) == 255).all() and (nr.correct_nuil(flat, 4) == 255).all()
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, size=(10, 13, 4), dtype=np.uint8)
    assert (nr.correct_nuil(img, 1) == 255).all()
    # dark text on a light page and its inverse: the same result
    page = np.full((20, 24), 220, np.uint8)
    page[5:8, 4:20] = 30
    page[12, 3:21] = 10
    got = nr.correct_nuil(page, 7)
    assert np.array_equal(got, nr.correct_nuil(255 - page, 7))
    assert got[6, 10] < 100 and got[0, 0] == 255
    # the mean threshold: sum == 128 * W * H is not inverted, one less is
    at = np.full((4, 8), 128, np.uint8)
    at[0, 0], at[0, 1] = 100, 156
    assert int(at.sum()) == 128 * 32 and nr.channel_inverted(at) == [False]
    below = at.copy()
    below[3, 7] = 127
    assert nr.channel_inverted(below) == [True]
    assert np.array_equal(nr.correct_nuil(below, 3), nr.correct_nuil(255 - below, 3, inverted=[False]))
    assert not np.array_equal(nr.correct_nuil(at, 3), nr.correct_nuil(255 - at, 3, inverted=[False]))
    two = np.dstack([at, below])   # decided per channel
    assert nr.channel_inverted(two) == [False, True]


def test_declared_and_exported(prl):
    from prlib_amd import _capi

    header = open(os.path.join(ROOT, "include", "prl_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _capi.EXPORTED_SYMBOLS
    assert re.search(r"#define PRL_HIP_ABI_VERSION 4\b", header)
    for name, value in (("PRL_MORPH_ERODE", 0), ("PRL_MORPH_DILATE", 1), ("PRL_MORPH_OPEN", 2), ("PRL_MORPH_CLOSE", 3),
                        ("PRL_MORPH_TOPHAT", 5), ("PRL_MORPH_BLACKHAT", 6), ("PRL_SHAPE_RECT", 0), ("PRL_SHAPE_CROSS", 1),
                        ("PRL_SHAPE_ELLIPSE", 2)):
        assert re.search(r"#define " + name + r" " + str(value) + r"\b", header), name
    assert (prl.morphology.MORPH_TOPHAT, prl.morphology.MORPH_BLACKHAT, prl.morphology.MORPH_ELLIPSE) == (nr.TOPHAT, nr.BLACKHAT, nr.ELLIPSE)
    assert callable(prl.correctNUIL) and callable(prl.morphologyEx)
    r = subprocess.run(["python", os.path.join(ROOT, "tools", "gen_export_map.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    assert os.path.exists(os.path.join(ROOT, "include", "prl", "correctNUIL.h"))
    if shutil.which("nm") is None:
        pytest.skip("binutils not installed")
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "prlib_amd", "libprlib_hip.so")],
                         capture_output=True, text=True, check=True).stdout
    for name in SYMBOLS:
        assert re.search(r"\bT " + name + r"\b", out), name


def test_statuses_in_their_order_without_touching_a_device(prl):
    from prlib_amd import _capi

    L = _capi.lib()
    src = np.zeros((8, 12, 4), np.uint8)
    dst = np.zeros_like(src)
    s, d = src.ctypes.data, dst.ctypes.data
    E, A, CH = _capi.PRL_ERR_EMPTY, _capi.PRL_ERR_BAD_ARG, _capi.PRL_ERR_BAD_CHANNELS

    def mdev(n=1, c=1, op=nr.CLOSE, shape=nr.ELLIPSE, kw=5, kh=5, sp=s, ss=12, w=12, h=8, dp=d, ds=12):
        return L.prl_hip_morphology_batch_device(n, c, op, shape, kw, kh, sp, 96 * 4, ss, w, h, dp, 96 * 4, ds, None)

    def mhost(n=1, c=1, op=nr.CLOSE, shape=nr.ELLIPSE, kw=5, kh=5, sp=s, ss=12, w=12, h=8, dp=d, ds=12):
        return L.prl_hip_morphology_host(c, op, shape, kw, kh, sp, ss, w, h, dp, ds)

    def ndev(n=1, c=1, size=5, sp=s, ss=12, w=12, h=8, dp=d, ds=12):
        return L.prl_hip_correct_nuil_batch_device(n, c, size, sp, 96 * 4, ss, w, h, dp, 96 * 4, ds, None)

    def nhost(n=1, c=1, size=5, sp=s, ss=12, w=12, h=8, dp=d, ds=12):
        return L.prl_hip_correct_nuil_host(c, size, sp, ss, w, h, dp, ds)

    for f in (mdev, mhost):
        assert f(w=0) == E and f(h=-1) == E
        assert f(w=0, op=4, c=9, sp=None) == E                      # empty first
        for op in (-1, 4, 7, 100):
            assert f(op=op) == A, op
        for shape in (-1, 3):
            assert f(shape=shape) == A, shape
        for k in (0, -1, 256, 1000):
            assert f(kw=k) == A and f(kh=k) == A, k
        assert f(op=4, c=0) == A and f(kw=0, c=5) == A and f(shape=7, c=9) == A   # op / shape / size before the channels
        for c in (0, 5, -1):
            assert f(c=c) == CH, c
        assert f(c=5, sp=None) == CH and f(c=0, ss=1) == CH        # channels before the pointers and strides
        assert f(sp=None) == A and f(dp=None) == A and f(ss=11) == A and f(ds=11) == A
        assert f(c=3, ss=35, ds=36) == A
        assert f(w=32769, ss=40000, ds=40000) == A and f(h=32769) == A
    for f in (ndev, nhost):
        assert f(w=0) == E and f(h=0) == E and f(w=0, size=0, c=7) == E
        for size in (0, -1, 256):
            assert f(size=size) == A and f(size=size, c=0) == A
        for c in (0, 5):
            assert f(c=c) == CH and f(c=c, dp=None) == CH
        assert f(sp=None) == A and f(dp=None) == A and f(ss=11) == A and f(ds=11) == A and f(h=32769) == A
    for f in (mdev, ndev):
        assert f(n=-1) == A
        assert f(n=0) == _capi.PRL_OK
    # any overlap of source and destination other than the same pages at the same strides
    assert L.prl_hip_morphology_batch_device(2, 1, nr.ERODE, nr.RECT, 3, 3, s, 96, 12, 12, 8, s + 12, 96, 12, None) == A
    assert L.prl_hip_correct_nuil_batch_device(2, 1, 3, s, 96, 12, 12, 8, s + 12, 96, 12, None) == A
    assert src.max() == 0 and dst.max() == 0


def test_valid_call_without_a_device(prl):
    import torch

    from prlib_amd import _capi

    if torch.cuda.is_available():
        pytest.skip("a device is present; the no-device behaviour is checked on the CPU box")
    img = np.zeros((8, 12, 3), np.uint8)
    out = np.zeros_like(img)
    for size in (1, 31, 255):
        assert _capi.lib().prl_hip_correct_nuil_host(3, size, img.ctypes.data, 36, 12, 8, out.ctypes.data, 36) == _capi.PRL_ERR_NO_DEVICE
    with pytest.raises(_capi.PrlError) as e:
        prl.correctNUIL(img)
    assert e.value.status == _capi.PRL_ERR_NO_DEVICE
    with pytest.raises(_capi.PrlError) as e:
        prl.morphologyEx(img, nr.TOPHAT, nr.CROSS, (3, 5))
    assert e.value.status == _capi.PRL_ERR_NO_DEVICE
    with pytest.raises(_capi.PrlError) as e:
        prl.correctNUIL(img, 0)
    assert e.value.status == _capi.PRL_ERR_BAD_ARG
    with pytest.raises(_capi.PrlError) as e:
        prl.morphologyEx(img, 4, nr.RECT, 3)
    assert e.value.status == _capi.PRL_ERR_BAD_ARG
    assert out.max() == 0


def build_dropin(out_dir):
    """g++ of tests/cpp/test_nuil_dropin.cpp + prl_host.cpp, with only -I include/prl for the drop-in header."""
    exe = os.path.join(out_dir, "test_nuil_dropin")
    flags = []
    for pc in ("opencv4", "opencv"):
        r = subprocess.run(["pkg-config", "--cflags", "--libs", pc], capture_output=True, text=True) if shutil.which("pkg-config") else None
        if r is not None and r.returncode == 0:
            flags = r.stdout.split()
            break
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include", "prl"),
           os.path.join(ROOT, "tests", "cpp", "test_nuil_dropin.cpp"), os.path.join(ROOT, "prlib_amd", "csrc", "prl", "prl_host.cpp"),
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
    assert r.returncode == 0 and "nuil dropin cpu: OK" in r.stdout, r.stdout + r.stderr
