"""prl::warpCrop without a device: the two restatements of tests/warp_ref.py against each other and against answers worked out
by hand, the fixtures' power to tell OpenCV's block rule from a walk without blocks, the host routines of the library
(prl_hip_perspective_transform, prl_hip_warp_crop_size) bit for bit against the restatement, every status of the entries, the
exports, and the C++ contract through the drop-in test binary."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import warp_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE_IDS = [f"{ow}x{oh}" for ow, oh in wr.SIZES]
NEW_EXPORTS = ("prl_hip_warp_crop_size", "prl_hip_perspective_transform", "prl_hip_warp_perspective_batch_device",
               "prl_hip_warp_crop_batch_device", "prl_hip_warp_crop_host")


def _inverted(name, sw, sh, ow, oh):
    m, inv = wr.matrix_case(name, sw, sh, ow, oh)
    return m if inv else wr.invert3(m)


# ---- the restatements -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", wr.SIZES, ids=SIZE_IDS)
def test_loop_equals_numpy_on_all_pixels(size):
    """every size, every matrix, both borders; the small source everywhere, the large one at the sizes with a seam"""
    ow, oh = size
    sources = wr.SOURCES if wr.multi_block(ow, oh) else wr.SOURCES[:1]
    for sw, sh in sources:
        src = wr.noise_page(sw, sh, 2, seed=sw)
        for name in wr.MATRICES:
            m = _inverted(name, sw, sh, ow, oh)
            assert wr.matrix_ok(m)
            for border, value in ((wr.BORDER_CONSTANT, (200, 7, 0, 0)), (wr.BORDER_REPLICATE, (0, 0, 0, 0))):
                a = wr.warp_loop(src, m, ow, oh, border, value)
                b = wr.warp_numpy(src, m, ow, oh, border, value)
                assert np.array_equal(a, b), (name, border, np.argwhere(a != b)[:5].tolist())


@pytest.mark.parametrize("size", [s for s in wr.SIZES if wr.multi_block(*s)], ids=[f"{w}x{h}" for w, h in wr.SIZES if wr.multi_block(w, h)])
@pytest.mark.parametrize("source", wr.SOURCES, ids=["67x45", "300x130"])
def test_fixtures_tell_the_block_rule_apart(size, source):
    """A condition on the fixtures: at every result size with more than one block per row some matrix of the set gives different
    bytes with and without the block rule - a kernel that forms M[0] * x in one piece cannot pass the byte-equality tests."""
    ow, oh = size
    sw, sh = source
    src = wr.noise_page(sw, sh, 1, seed=sw)
    differing = []
    for name in wr.MATRICES:
        m = _inverted(name, sw, sh, ow, oh)
        a, b = wr.warp_numpy(src, m, ow, oh), wr.warp_numpy(src, m, ow, oh, block_rule=False)
        if not np.array_equal(a, b):
            differing.append(name)
            assert (a != b)[:, wr.block_width(ow, oh):].any() and not (a != b)[:, :wr.block_width(ow, oh)].any(), "only behind the first seam"
    assert differing, "no matrix distinguishes the block rule at this size"


def test_sizes_cover_the_block_widths():
    assert {wr.block_width(ow, oh) for ow, oh in wr.SIZES if wr.multi_block(ow, oh)} == {341, 64}
    assert wr.block_width(400, 1) == 400 and wr.block_width(400, 3) == 341 and wr.block_width(65, 17) == 64


def test_the_matrices_reach_what_they_are_for():
    sw, sh, ow, oh = 67, 45, 400, 17
    x = np.arange(ow, dtype=np.float64)[None, :]
    y = np.arange(oh, dtype=np.float64)[:, None]
    m = _inverted("horizon", sw, sh, ow, oh)
    w = m[6] * x + m[7] * y + m[8]
    assert (w == 0).any() and (w > 0).any() and (w < 0).any()
    m = _inverted("huge", sw, sh, ow, oh)
    fx = (m[0] * x + m[2]) * 32
    assert (fx > 2.0 ** 31).any() and (fx < -2.0 ** 31).any()
    m = _inverted("far", sw, sh, ow, oh)
    fx = (m[0] * x + m[2]) * 32
    assert (np.abs(fx) < 2.0 ** 31).all() and (fx / 32 > 32768).any() and (fx / 32 < -32769).any()   # the source column leaves the short range
    src = wr.noise_page(sw, sh, 1, 5) | 1
    out = wr.warp_numpy(src, _inverted("outside", sw, sh, ow, oh), ow, oh)
    assert 0 < (out != 0).mean() < 0.5


# ---- known answers --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(67, 45), (300, 130)])
def test_identity_quad(w, h):
    quad = [0, 0, w, 0, w, h, 0, h]
    assert wr.crop_size(quad, -1.0) == (w, h)
    m = wr.crop_matrix(quad, w, h)
    assert m == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    assert wr.invert3(m) == m
    for name, page in wr.families(w, h, 3, seed=2):
        assert np.array_equal(wr.warp_crop(page, quad), page), name
        assert np.array_equal(wr.warp_loop(page, m, w, h), page), name


def test_integer_translation():
    w, h, dx, dy = 40, 23, 7, -4
    page = wr.noise_page(w, h, 3, 9)
    m = [1.0, 0.0, float(dx), 0.0, 1.0, float(dy), 0.0, 0.0, 1.0]   # result (x, y) reads source (x + dx, y + dy)
    want = np.empty_like(page)
    want[:] = np.array([9, 255, 0], np.uint8)
    want[-dy:, :w - dx] = page[:h + dy, dx:]
    for fn in (wr.warp_loop, wr.warp_numpy):
        got = fn(page, m, w, h, wr.BORDER_CONSTANT, (9.2, 300.0, -3.0, 0.0))
        assert np.array_equal(got, want)
    # the forward form: warpPerspective inverts it
    fwd = [1.0, 0.0, float(-dx), 0.0, 1.0, float(-dy), 0.0, 0.0, 1.0]
    assert np.array_equal(wr.warp_perspective(page, fwd, w, h, False, wr.BORDER_CONSTANT, (9.2, 300.0, -3.0, 0.0)), want)
    rep = wr.warp_numpy(page, m, w, h, wr.BORDER_REPLICATE)
    assert np.array_equal(rep[:-dy, :w - dx], np.repeat(page[:1, dx:], -dy, axis=0)) and np.array_equal(rep[5, w - dx:, 0], np.full(dx, page[1, w - 1, 0]))


def test_scale_by_two_by_hand():
    """forward matrix diag(2, 2, 1): result (x, y) reads source (x / 2, y / 2).  Row 0: X = 16 x, so sx = x >> 1, fx = 16 (x & 1), fy = 0:
    even columns copy a pixel, odd ones are (a * 16384 + b * 16384 + 2^14) >> 15 = (a + b + 1) >> 1.  Column 0 likewise down the rows."""
    src = np.array([[10, 20, 31], [40, 51, 60], [7, 9, 200]], np.uint8)[:, :, None]
    out = wr.warp_perspective(src, [2.0, 0, 0, 0, 2.0, 0, 0, 0, 1.0], 6, 6, False, wr.BORDER_CONSTANT, (100, 0, 0, 0))[:, :, 0]
    assert out[0].tolist() == [10, 15, 20, 26, 31, 66]       # (31 + 100 + 1) >> 1 = 66: the border value enters the last tap
    assert out[:, 0].tolist() == [10, 25, 40, 24, 7, 54]     # (40 + 7 + 1) >> 1 = 24, (7 + 100 + 1) >> 1 = 54
    assert out[1, 1] == (10 * 8192 + 20 * 8192 + 40 * 8192 + 51 * 8192 + (1 << 14)) >> 15
    assert np.array_equal(out, wr.warp_loop(src, wr.invert3([2.0, 0, 0, 0, 2.0, 0, 0, 0, 1.0]), 6, 6, value=(100, 0, 0, 0))[:, :, 0])


def test_size_rule_by_hand():
    assert wr.crop_size([0, 0, 3, 4, 3, 4, 0, 0], -1.0) == (5, 0)                 # a 3-4-5 side; H = 0
    assert wr.crop_size([0, 0, 10, 0, 10, 5, 0, 5], 2.0) == (2, 5)                # 2.5 -> 2: half to even
    assert wr.crop_size([0, 0, 10, 0, 10, 7, 0, 7], 2.0) == (4, 7)                # 3.5 -> 4
    assert wr.crop_size([0, 0, 10, 0, 10, 7, 0, 7], 0.0) == (10, 7) and wr.crop_size([0, 0, 10, 0, 10, 7, 0, 7], -2.0) == (10, 7)
    assert wr.crop_size([0, 0, 1, 1, 1, 2, 0, 1], -1.0) == (1, 1)                 # sqrt(2) = 1.41 -> 1
    assert wr.crop_size([-20000, -20000, 20000, 20000, 0, 0, 0, 0], -1.0)[0] == wr.INT_MIN   # the int expression wraps: NaN side
    assert wr.cv_round(0.5) == 0 and wr.cv_round(1.5) == 2 and wr.cv_round(-2.5) == -2 and wr.cv_round(float("nan")) == wr.INT_MIN


# ---- the library's host routines ------------------------------------------------------------------------------------------------

def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64).tolist()


def _c_transform(L, s, d):
    s = np.ascontiguousarray(s, dtype=np.float64)
    d = np.ascontiguousarray(d, dtype=np.float64)
    m = np.full(9, -7.0)
    return L.prl_hip_perspective_transform(s.ctypes.data, d.ctypes.data, m.ctypes.data), m


def _c_size(L, quad, ratio):
    q = np.ascontiguousarray(quad, dtype=np.int32)
    ow, oh = C.c_int(-7), C.c_int(-7)
    return L.prl_hip_warp_crop_size(q.ctypes.data, float(ratio), C.byref(ow), C.byref(oh)), ow.value, oh.value


def test_perspective_transform_bit_for_bit(prl):
    from prlib_amd import _capi

    L = _capi.lib()
    rng = np.random.default_rng(20240614)
    solved = 0
    for _ in range(200):
        s, d = rng.integers(-20000, 20001, 8), rng.integers(-20000, 20001, 8)
        st, m = _c_transform(L, s, d)
        try:
            want = wr.perspective_transform(s, d)
        except wr.Singular:
            assert st == _capi.PRL_ERR_BAD_ARG and (m == -7.0).all()
            continue
        solved += 1
        assert st == _capi.PRL_OK and _bits(m) == _bits(want), (s.tolist(), d.tolist())
    assert solved >= 190
    # corners that are not floats go through float first
    s = [0.1, 0.2, 100.3, 0.7, 99.9, 80.1, 0.4, 79.6]
    d = [0, 0, 64.5, 0, 64.5, 48.25, 0, 48.25]
    st, m = _c_transform(L, s, d)
    assert st == _capi.PRL_OK and _bits(m) == _bits(wr.perspective_transform(s, d))
    assert _bits(m) != _bits(wr.lu_solve(*_system64(s, d)) + [1.0])
    assert np.array_equal(prl.perspective_transform(s, d).ravel(), m)


def _system64(s, d):
    a, b = [], [0.0] * 8
    for half in range(2):
        for i in range(4):
            sx, sy, dx, dy = s[2 * i], s[2 * i + 1], d[2 * i], d[2 * i + 1]
            t = dy if half else dx
            a.append(([0.0, 0.0, 0.0] if half else []) + [sx, sy, 1.0] + ([] if half else [0.0, 0.0, 0.0]) + [-sx * t, -sy * t])
            b[i + 4 * half] = t
    return a, b


@pytest.mark.parametrize("quad", [[0, 0, 10, 10, 20, 20, 0, 30], [0, 0, 100, 0, 50, 0, 0, 80], [5, 4, 5, 4, 52, 35, 3, 33],
                                  [5, 4, 50, 6, 50, 6, 3, 33], [7, 7, 7, 7, 7, 7, 7, 7]],
                         ids=["collinear", "collinear_top", "repeated01", "repeated12", "all_equal"])
def test_singular_corners(prl, quad):
    from prlib_amd import _capi

    L = _capi.lib()
    d = [0, 0, 30, 0, 30, 20, 0, 20]
    with pytest.raises(wr.Singular):
        wr.perspective_transform(quad, d)
    st, m = _c_transform(L, quad, d)
    assert st == _capi.PRL_ERR_BAD_ARG and (m == -7.0).all()
    with pytest.raises(_capi.PrlError):
        prl.perspective_transform(quad, d)


def test_warp_crop_size_bit_for_bit(prl):
    from prlib_amd import _capi

    L = _capi.lib()
    rng = np.random.default_rng(20240615)
    quads = [rng.integers(-20000, 20001, 8) for _ in range(200)]
    quads += [rng.integers(0, 3000, 8) for _ in range(50)]
    quads += [np.array(q) for q in ([0, 0, 10, 0, 10, 5, 0, 5], [0, 0, 10, 0, 10, 7, 0, 7], [0, 0, 3, 4, 3, 4, 0, 0], [0, 0, 32767, 0, 32767, 1, 0, 1],
                                    [0, 0, 32768, 0, 32768, 1, 0, 1], [-20000, -20000, 20000, 20000, 0, 0, 0, 0], [0, 0, 5, 0, 5, 5, 0, 5])]
    seen = {"ok": 0, "bad": 0}
    for q in quads:
        for ratio in (-1.0, 0.0, 2.0, 1.4142135623730951, 10.0 / 3.0, 1e-9, 250.0):
            w, h = wr.crop_size(q, ratio)
            st, ow, oh = _c_size(L, q, ratio)
            if wr.size_ok(w, h):
                assert (st, ow, oh) == (_capi.PRL_OK, w, h), (q.tolist(), ratio)
                seen["ok"] += 1
            else:
                assert (st, ow, oh) == (_capi.PRL_ERR_BAD_ARG, -7, -7), (q.tolist(), ratio, w, h)
                seen["bad"] += 1
    assert seen["ok"] > 300 and seen["bad"] > 300
    assert _c_size(L, [0, 0, 10, 0, 10, 5, 0, 5], 2.0)[1:] == (2, 5) and _c_size(L, [0, 0, 10, 0, 10, 7, 0, 7], 2.0)[1:] == (4, 7)   # half to even
    assert prl.warp_crop_size([0, 0, 10, 0, 10, 7, 0, 7], 2.0) == (4, 7)


# ---- statuses, exports, the C++ contract ----------------------------------------------------------------------------------------

def test_statuses_without_touching_a_device(prl):
    """every status of the three page entries, in the documented order; the arguments that pass them all reach the device check"""
    import torch

    from prlib_amd import _capi

    L = _capi.lib()
    src = np.zeros((8, 12, 3), np.uint8)
    dst = np.zeros((16, 16, 3), np.uint8)
    ident = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1])
    wh = np.array([12, 8], np.int32)
    quad = np.array([0, 0, 12, 0, 12, 8, 0, 8], np.int32)
    val = np.zeros(4)

    def persp(n=1, ch=3, m=ident, inv=0, s=src.ctypes.data, step=36, w=12, h=8, d=dst.ctypes.data, dstep=48, sizes=wh, mode=0, v=val.ctypes.data):
        m = np.ascontiguousarray(m, dtype=np.float64)
        sizes = None if sizes is None else np.ascontiguousarray(sizes, dtype=np.int32)
        return L.prl_hip_warp_perspective_batch_device(n, ch, m.ctypes.data, inv, s, 0, step, w, h, d, 0, dstep,
                                                       None if sizes is None else sizes.ctypes.data, mode, v, None)

    def crop(n=1, ch=3, q=quad, ratio=-1.0, s=src.ctypes.data, step=36, w=12, h=8, d=dst.ctypes.data, dstep=48, mode=0, out=True):
        q = np.ascontiguousarray(q, dtype=np.int32)
        o = np.full(2, -7, np.int32)
        st = L.prl_hip_warp_crop_batch_device(n, ch, q.ctypes.data, ratio, s, 0, step, w, h, d, 0, dstep, o.ctypes.data if out else None, mode,
                                              None, None)
        assert st == _capi.PRL_OK or (o == -7).all()
        return st

    def host(ch=3, q=quad, ratio=-1.0, s=src.ctypes.data, step=36, w=12, h=8, d=dst.ctypes.data, dstep=48, mode=0):
        q = np.ascontiguousarray(q, dtype=np.int32)
        return L.prl_hip_warp_crop_host(ch, q.ctypes.data, ratio, s, step, w, h, d, dstep, mode, None)

    E = _capi
    for fn in (persp, crop, host):
        assert fn(w=0) == E.PRL_ERR_EMPTY and fn(h=-1) == E.PRL_ERR_EMPTY
        assert fn(w=0, ch=9, mode=7) == E.PRL_ERR_EMPTY                       # the order of the checks
        assert fn(ch=0) == E.PRL_ERR_BAD_CHANNELS and fn(ch=5) == E.PRL_ERR_BAD_CHANNELS and fn(ch=5, mode=7) == E.PRL_ERR_BAD_CHANNELS
        for mode in (2, 3, 4, 5, -1, 16):
            assert fn(mode=mode) == E.PRL_ERR_UNSUPPORTED
        assert fn(mode=2, step=1) == E.PRL_ERR_UNSUPPORTED
        assert fn(step=35) == E.PRL_ERR_BAD_ARG and fn(d=None) == E.PRL_ERR_BAD_ARG
        assert fn(w=32768, step=32768 * 3) == E.PRL_ERR_BAD_ARG and fn(h=32768) == E.PRL_ERR_BAD_ARG
    assert host(s=None) == E.PRL_ERR_EMPTY     # the host entries call a null image empty
    for fn in (persp, crop):
        assert fn(s=None) == E.PRL_ERR_BAD_ARG and fn(n=-1) == E.PRL_ERR_BAD_ARG
        assert fn(d=src.ctypes.data) == E.PRL_ERR_BAD_ARG    # in place
        assert fn(n=0) == E.PRL_OK
    assert persp(sizes=None) == E.PRL_ERR_BAD_ARG and crop(out=False) == E.PRL_ERR_BAD_ARG
    # per page: sizes, destination rows, matrices
    for sizes in ([0, 8], [12, 0], [-3, 8], [32768, 8], [12, 32768]):
        assert persp(sizes=sizes, dstep=1 << 20) == E.PRL_ERR_BAD_ARG
    assert persp(dstep=35) == E.PRL_ERR_BAD_ARG and crop(dstep=35) == E.PRL_ERR_BAD_ARG and host(dstep=35) == E.PRL_ERR_BAD_ARG
    for bad in (np.nan, np.inf, -np.inf, 2.0 ** 501, -(2.0 ** 501)):
        m = ident.copy()
        m[2] = bad
        assert persp(m=m, inv=1) == E.PRL_ERR_BAD_ARG and persp(m=m, inv=0) == E.PRL_ERR_BAD_ARG
    assert persp(m=np.zeros(9)) == E.PRL_ERR_BAD_ARG                                   # det == 0
    assert persp(m=[1, 2, 3, 2, 4, 6, 0, 0, 1]) == E.PRL_ERR_BAD_ARG                   # det == 0
    assert persp(m=[2.0 ** -501, 0, 0, 0, 2.0 ** -501, 0, 0, 0, 1]) == E.PRL_ERR_BAD_ARG   # the inverse leaves the limit
    second_bad = np.concatenate([ident, np.zeros(9)])
    assert persp(n=2, m=second_bad, sizes=[12, 8, 12, 8]) == E.PRL_ERR_BAD_ARG         # any page
    for q in ([0, 0, 10, 10, 20, 20, 0, 30], [5, 4, 5, 4, 52, 35, 3, 33], [7, 7, 7, 7, 7, 7, 7, 7], [0, 0, 3, 4, 3, 4, 0, 0]):
        assert crop(q=q) == E.PRL_ERR_BAD_ARG and host(q=q) == E.PRL_ERR_BAD_ARG
    assert crop(ratio=1e-9) == E.PRL_ERR_BAD_ARG and host(ratio=1e-9) == E.PRL_ERR_BAD_ARG
    assert crop(q=[0, 0, 40000, 0, 40000, 8, 0, 8], dstep=1 << 20) == E.PRL_ERR_BAD_ARG
    sz = C.c_int(0)
    assert L.prl_hip_warp_crop_size(None, -1.0, C.byref(sz), C.byref(sz)) == E.PRL_ERR_BAD_ARG
    assert L.prl_hip_warp_crop_size(quad.ctypes.data, -1.0, None, C.byref(sz)) == E.PRL_ERR_BAD_ARG
    assert L.prl_hip_perspective_transform(None, val.ctypes.data, val.ctypes.data) == E.PRL_ERR_BAD_ARG
    assert b"not provided" in L.prl_hip_strerror(E.PRL_ERR_UNSUPPORTED)
    if not torch.cuda.is_available():   # valid arguments get as far as the device
        assert persp() == E.PRL_ERR_NO_DEVICE and crop() == E.PRL_ERR_NO_DEVICE and host() == E.PRL_ERR_NO_DEVICE


def test_exports_maps_and_headers(prl):
    from prlib_amd import _capi

    for name in NEW_EXPORTS:
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(_capi.lib(), name)
        for m in ("prl_hip.map", "prl_hip_testhooks.map"):
            assert re.search(r"^\s+" + name + ";$", open(os.path.join(ROOT, "prlib_amd", "csrc", m)).read(), flags=re.M), (name, m)
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "prlib_amd", "libprlib_hip.so")], capture_output=True, text=True,
                         check=True).stdout
    for name in NEW_EXPORTS:
        assert re.search(r"\bT " + name + r"\b", out), name
    assert os.path.exists(os.path.join(ROOT, "include", "prl", "warp.h"))
    assert _capi.lib().prl_hip_abi_version() == 4
    for fn in ("warp_crop_size", "perspective_transform", "warp_perspective", "warp_crop"):
        assert callable(getattr(prl, fn)) and fn in prl.__all__


def build_dropin(out_dir):
    """g++ of tests/cpp/test_warp_dropin.cpp + prl_host.cpp, with only -I include/prl for the drop-in header."""
    exe = os.path.join(out_dir, "test_warp_dropin")
    flags = []
    for pc in ("opencv4", "opencv"):
        r = subprocess.run(["pkg-config", "--cflags", "--libs", pc], capture_output=True, text=True) if shutil.which("pkg-config") else None
        if r is not None and r.returncode == 0:
            flags = r.stdout.split()
            break
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include", "prl"),
           os.path.join(ROOT, "tests", "cpp", "test_warp_dropin.cpp"), os.path.join(ROOT, "prlib_amd", "csrc", "prl", "prl_host.cpp"),
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
    assert r.returncode == 0 and "warp dropin cpu: OK" in r.stdout, r.stdout + r.stderr
