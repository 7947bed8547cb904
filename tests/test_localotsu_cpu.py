"""prl::binarizeLocalOtsu's parts without a device: the 8.8 weights of the 8-bit cv::GaussianBlur (the tables of the header, every odd
side at sigma 0 and over the sigma grid 0.1 .. 100, the tie margin that lets std::exp stand for OpenCV's soft-float exp, the C entry),
self-checks of the restatement tests/localotsu_ref.py, the external-rectangle scanner of contour.h against the literal restatement
on hand-made and random maps, the statuses of every new entry in their documented order, the exports, the drop-in header's C++
contract, and gauss8.h plus the scanner in a stand-alone program under the address and undefined-behaviour sanitizers.  Every
comparison is an equality."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import localotsu_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("prl_hip_gaussian_kernel_u8", "prl_hip_sep_filter_u8_batch_device", "prl_hip_gaussian_blur_u8_batch_device",
           "prl_hip_gaussian_blur_u8_host", "prl_hip_canny_edge_detection_batch_device", "prl_hip_canny_edge_detection_host",
           "prl_hip_external_rects", "prl_hip_rect_otsu_batch_device", "prl_hip_binarize_local_otsu_batch_device",
           "prl_hip_binarize_local_otsu_host")
TABLES = {3: [64, 128, 64], 5: [16, 64, 96, 64, 16], 7: [8, 28, 56, 72, 56, 28, 8], 9: [4, 13, 30, 51, 60, 51, 30, 13, 4],
          19: [1, 1, 3, 5, 10, 15, 20, 27, 30, 32, 30, 27, 20, 15, 10, 5, 3, 1, 1]}
SIGMAS = [round(0.1 * i, 1) for i in range(1, 1001)]   # 0.1, 0.2 .. 100
ODD = range(1, lr.MAX_SIDE + 1, 2)


# ---- the weights -----------------------------------------------------------------------------------------------------------------

def test_the_five_tables_of_the_header():
    for n, want in TABLES.items():
        assert lr.kernel_u8(n) == want, n
    assert lr.kernel_u8(1) == [256]
    w25 = lr.kernel_u8(25)
    assert w25[11:14] == [25, 24, 25], "n = 25 at sigma 0: the centre is not the largest weight"


def grid_weights(n, sigmas):
    """lr.kernel_u8(n, s) for every s of `sigmas` at once (numpy over the sigma axis, the same steps in the same order) and the
    smallest tie distance of each"""
    s = np.asarray(sigmas, np.float64)
    x = np.arange(n, dtype=np.float64) - (n - 1) * 0.5
    k = np.exp((-0.5 / (s * s))[:, None] * (x * x)[None, :])
    total = np.zeros(len(s))
    for i in range(n):
        total = total + k[:, i]
    k = k / total[:, None]
    w = np.zeros((len(s), n), np.int64)
    err = np.zeros(len(s))
    margin = np.full(len(s), 0.5)
    for i in range(n // 2):
        adj = k[:, i] * 256 + err
        v = np.rint(adj)
        err = adj - v
        margin = np.minimum(margin, np.abs(adj - np.floor(adj) - 0.5))
        w[:, i] = w[:, n - 1 - i] = v.astype(np.int64)
    w[:, n // 2] = 256 - w.sum(axis=1)
    return w, margin


def test_every_side_sums_to_256_and_no_adj_is_near_a_tie(prl):
    """sigma 0 for every odd n <= 255, and n x the sigma grid: sum 256, no negative weight; the tie margin stays above 1e-9 - a
    condition on the restatement (an exp within a few ulp cannot move a weight), not a measurement; the C entry gives the same
    weights on all of them"""
    from prlib_amd import _capi

    L = _capi.lib()
    buf = np.zeros(lr.MAX_SIDE, np.uint16)
    worst0, worst = 0.5, 0.5
    for n in ODD:
        w, margin = lr.kernel_u8(n, 0.0, with_margin=True)
        assert sum(w) == 256 and min(w) >= 0 and w == w[::-1], n
        worst0 = min(worst0, margin)
        assert L.prl_hip_gaussian_kernel_u8(n, 0.0, buf.ctypes.data) == 0 and buf[:n].tolist() == w, n
        assert L.prl_hip_gaussian_kernel_u8(n, -1.0, buf.ctypes.data) == 0 and buf[:n].tolist() == w, "a negative sigma counts as 0"
    for n in ODD:
        wg, margin = grid_weights(n, SIGMAS)
        assert (wg.sum(axis=1) == 256).all() and wg.min() >= 0, n
        worst = min(worst, float(margin.min()))
        for j in range(0, len(SIGMAS), 97):   # the scalar restatement agrees with its vector form
            assert lr.kernel_u8(n, SIGMAS[j]) == wg[j].tolist(), (n, SIGMAS[j])
        for j, s in enumerate(SIGMAS):
            assert L.prl_hip_gaussian_kernel_u8(n, s, buf.ctypes.data) == 0
            if buf[:n].tolist() != wg[j].tolist():
                raise AssertionError((n, s, buf[:n].tolist(), wg[j].tolist()))
    print("tie margin at sigma 0:", worst0, "over the sigma grid:", worst)
    assert worst0 > 1e-9 and worst > 1e-9


# ---- the restatement's own checks ------------------------------------------------------------------------------------------------

def test_a_constant_page_blurs_to_itself():
    for v in (0, 1, 128, 254, 255):
        for n in (3, 19, 33):
            page = np.full((9, 13), v, np.uint8)
            assert np.array_equal(lr.blur_u8(page, (n, n)), page)
    page = np.full((5, 6), 255, np.uint8)
    assert np.array_equal(lr.blur_u8(page, (255, 255)), page), "all 255 with n = 255 stays 255"


def test_separable_equals_the_direct_double_sum():
    page = lr.noise(5, 7, 1, 3)
    for ksize, sx, sy in (((5, 3), 0.0, 0.0), ((19, 19), 0.0, 0.0), ((3, 9), 1.5, 0.7), ((1, 1), 0.0, 0.0)):
        assert np.array_equal(lr.blur_u8(page, ksize, sx, sy), lr.blur_u8_direct(page, ksize, sx, sy)), ksize
    assert np.array_equal(lr.blur_u8(page, (1, 1)), page), "a 1 x 1 kernel copies"
    colour = lr.noise(6, 5, 3, 4)
    got = lr.blur_u8(colour, (5, 5))
    for c in range(3):
        assert np.array_equal(got[:, :, c], lr.blur_u8(np.ascontiguousarray(colour[:, :, c]), (5, 5)))


def test_otsu_restatement_on_known_histograms():
    assert lr.otsu_of(np.full((4, 4), 9, np.uint8)) == 0, "a uniform rectangle: no class split, threshold 0"
    two = np.array([[10] * 8 + [200] * 8], np.uint8)
    assert lr.otsu_of(two) == 10, "two levels: the first index of the largest between-class variance"
    assert lr.rect_otsu(np.full((4, 4), 0, np.uint8), [(0, 0, 4, 4)])[0].max() == 0, "a black uniform rectangle is painted (p <= 0)"
    assert lr.rect_otsu(np.full((4, 4), 9, np.uint8), [(0, 0, 4, 4)])[0].min() == 255
    gray = lr.noise(8, 8, 1, 1)
    for mv, black in ((255.0, False), (254.5, True), (254.51, False), (128.0, True), (0.0, True)):
        mask, _ = lr.rect_otsu(gray, [(1, 1, 5, 4)], mv)
        assert (mask[1:5, 1:6] == 0).all() == black, mv
        assert (np.delete(mask, np.s_[1:5], axis=0) == 255).all()


# ---- the external rectangles -----------------------------------------------------------------------------------------------------

def ring(side, wall, blob):
    m = np.zeros((side + 2, side + 2), np.uint8)
    m[1:-1, 1:-1] = 255
    m[1 + wall:-1 - wall, 1 + wall:-1 - wall] = 0
    c = (side + 2) // 2
    m[c - blob // 2:c - blob // 2 + blob, c - blob // 2:c - blob // 2 + blob] = 255
    return m


def hand_made_maps():
    maps = {"empty": np.zeros((7, 9), np.uint8), "1x1 set": np.full((1, 1), 255, np.uint8), "1x1 clear": np.zeros((1, 1), np.uint8)}
    row = np.array([[1, 0, 1, 1, 1, 0, 0, 1, 1, 0, 1, 1, 1, 1]], np.uint8) * 255
    maps["1xN"], maps["Nx1"] = row, np.ascontiguousarray(row.T)
    one = np.zeros((5, 6), np.uint8)
    one[2, 3] = 1
    maps["one pixel"] = one
    two = np.zeros((5, 6), np.uint8)
    two[2, 2:4] = 7
    maps["two-pixel line"] = two
    diag = np.zeros((5, 6), np.uint8)
    diag[1, 1] = diag[2, 2] = 255
    maps["two pixels on a diagonal"] = diag
    maps["thick ring with a blob"] = ring(14, 3, 3)
    maps["thin ring with a blob"] = ring(14, 1, 3)
    maps["thin ring, blob at the wall"] = ring(9, 1, 5)
    edges = np.zeros((12, 15), np.uint8)
    edges[0:2, 0:2] = edges[0:2, -2:] = edges[-2:, 0:2] = edges[-2:, -2:] = 255        # the corners
    edges[0, 6:9] = edges[-1, 5:10] = edges[5:8, 0] = edges[4:7, -1] = 255             # the edges
    edges[0:3, 11] = 255
    maps["on every edge and corner"] = edges
    maps["checkerboard"] = ((np.add.outer(np.arange(9), np.arange(11)) & 1) * 255).astype(np.uint8)
    maps["full page"] = np.full((6, 8), 255, np.uint8)
    nested = np.zeros((20, 20), np.uint8)
    nested[1:19, 1:19] = 255
    nested[3:17, 3:17] = 0
    nested[5:15, 5:15] = 255
    nested[7:13, 7:13] = 0
    nested[9:11, 9:11] = 255
    maps["rings in rings"] = nested
    return maps


def c_rects(prl, m):
    rects, found = prl.externalRects(m)
    return sorted(map(tuple, rects.tolist())), found


def test_external_rects_on_hand_made_maps(prl):
    for name, m in hand_made_maps().items():
        want, found = lr.external_rects(m)
        assert c_rects(prl, m) == (sorted(want), found), name
    maps = hand_made_maps()
    # fewer than 3 points: one contour found, no rectangle kept
    for name in ("1x1 set", "one pixel", "two-pixel line", "two pixels on a diagonal"):
        assert lr.external_rects(maps[name]) == ([], 1), name
    assert lr.external_rects(maps["empty"]) == ([], 0) and lr.external_rects(maps["full page"]) == ([(0, 0, 8, 6)], 1)
    assert lr.external_rects(maps["checkerboard"]) == ([(0, 0, 11, 9)], 1), "one 8-connected component"
    assert lr.external_rects(maps["on every edge and corner"])[1] == 9


def test_the_blob_in_a_thick_ring_is_not_external(prl):
    """the restatement itself: the scan is inside the ring's border when it meets the blob (the pixel at lnbd is a traced pixel
    that is no right end), so the blob is skipped; a scanner that took the outer border of every component (the non-hole contours
    of RETR_CCOMP) would add the blob's rectangle, and that would change the final mask"""
    m = ring(14, 3, 3)
    rects, found = lr.external_rects(m)
    assert (rects, found) == ([(1, 1, 14, 14)], 1)
    loose, loose_found = lr.component_rects(m)
    assert loose_found == 2 and sorted(loose) == [(1, 1, 14, 14), (7, 7, 3, 3)]
    # a gray page on which the blob's own Otsu threshold paints pixels that the ring's rectangle leaves white
    gray = np.full(m.shape, 200, np.uint8)
    gray[1:15, 1:15] = 40                                  # dark ring area: the large rectangle splits 40 | {180, 200}
    gray[4:12, 4:12] = 200
    gray[7:10, 7:10] = np.array([[180, 200, 180], [200, 180, 200], [180, 200, 180]], np.uint8)
    mask, _ = lr.rect_otsu(gray, rects)
    mask_loose, _ = lr.rect_otsu(gray, loose)
    assert (mask[7:10, 7:10] == 255).all() and (mask_loose[7:10, 7:10] == 0).any()
    assert not np.array_equal(mask, mask_loose), "treating the blob as external changes the mask"
    assert c_rects(prl, m) == ([(1, 1, 14, 14)], 1)


def test_external_rects_on_random_maps(prl):
    rng = np.random.default_rng(20)
    for it in range(200):
        h, w = (int(v) for v in rng.integers(1, 41, size=2))
        density = 0.1 + 0.1 * (it % 9)
        m = (rng.random((h, w)) < density).astype(np.uint8) * (1 + it % 255)
        want, found = lr.external_rects(m)
        assert c_rects(prl, m) == (sorted(want), found), (it, h, w, density)


def test_external_rects_entry_with_a_pitch_and_without_room(prl):
    from prlib_amd import _capi

    L = _capi.lib()
    m = np.zeros((12, 32), np.uint8)
    m[:, 20:] = 255                                 # beyond the width: never read
    m[2:6, 3:9] = m[8:11, 12:18] = 255
    found, kept = ctypes.c_int(-1), ctypes.c_int(-1)
    rects = np.full((2, 4), -7, np.int32)
    assert L.prl_hip_external_rects(m.ctypes.data, 32, 19, 12, rects.ctypes.data, 1, ctypes.byref(found), ctypes.byref(kept)) == 0
    assert (found.value, kept.value) == (2, 2) and (rects == -7).all(), "no room: the counts alone"
    assert L.prl_hip_external_rects(m.ctypes.data, 32, 19, 12, rects.ctypes.data, 2, ctypes.byref(found), ctypes.byref(kept)) == 0
    assert sorted(map(tuple, rects.tolist())) == [(3, 2, 6, 4), (12, 8, 6, 3)]


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------

def test_statuses_in_their_order_without_touching_a_device(prl):
    import torch

    from prlib_amd import _capi

    L = _capi.lib()
    E, W, CH, A, N = _capi.PRL_ERR_EMPTY, _capi.PRL_ERR_BAD_WINDOW, _capi.PRL_ERR_BAD_CHANNELS, _capi.PRL_ERR_BAD_ARG, _capi.PRL_ERR_NO_DEVICE
    no_gpu = not torch.cuda.is_available()   # a valid device call on these host arrays must never reach a device
    buf, out = np.zeros(1 << 16, np.uint8), np.zeros(1 << 16, np.uint8)
    s, o = buf.ctypes.data, out.ctypes.data
    nan, inf = float("nan"), float("inf")

    # the host table
    w16 = np.zeros(256, np.uint16)
    k = lambda n, sg=0.0, p=w16.ctypes.data: L.prl_hip_gaussian_kernel_u8(n, sg, p)
    assert k(0) == W and k(-3) == W and k(4) == W and k(257) == W and k(4, nan, None) == W
    assert k(3, nan) == A and k(3, inf) == A and k(3, 0.0, None) == A and k(255) == 0

    # the blur and the explicit-weight filter
    def blur(n=1, c=1, kw=3, kh=3, sx=0.0, sy=0.0, sp=s, ss=64, w=32, h=20, dp=o, ds=64):
        return L.prl_hip_gaussian_blur_u8_batch_device(n, c, kw, kh, sx, sy, sp, ss * h, ss, w, h, dp, ds * h, ds, None)

    def blur_host(c=1, kw=3, kh=3, sx=0.0, sy=0.0, sp=s, ss=64, w=32, h=20, dp=o, ds=64, n=1):
        return L.prl_hip_gaussian_blur_u8_host(c, kw, kh, sx, sy, sp, ss, w, h, dp, ds)

    wx, wy = np.array([64, 128, 64], np.uint16), np.array([100, 56, 100], np.uint16)

    def sep(n=1, c=1, px=wx.ctypes.data, nx=3, py=wy.ctypes.data, ny=3, sp=s, ss=64, w=32, h=20, dp=o, ds=64):
        return L.prl_hip_sep_filter_u8_batch_device(n, c, px, nx, py, ny, sp, ss * h, ss, w, h, dp, ds * h, ds, None)

    for f in (blur, blur_host):
        assert f(w=0, kw=4, c=9) == E and f(h=-1) == E
        assert f(kw=4, c=9) == W and f(kh=0) == W and f(kw=-3) == W and f(kh=257) == W and f(kw=2, sx=nan) == W
        assert f(c=0) == A and f(c=5) == A and f(sx=nan) == A and f(sy=inf) == A
        assert f(sp=None) == A and f(dp=None) == A and f(ss=31) == A and f(c=3, ds=95) == A
        assert f(w=32769, ss=40000, ds=40000) == A
        assert f(dp=s) == A and f(dp=s + 64 * 19 + 31) == A, "source and destination share a byte"
    assert blur(n=-1) == A and blur(n=0) == 0 and blur(n=0, kw=4) == W
    assert sep(w=0, nx=4) == E and sep(nx=4) == W and sep(ny=257) == W and sep(c=5) == A
    assert sep(px=None) == A and sep(py=None) == A
    heavy = np.array([100, 57, 100], np.uint16)
    assert sep(py=heavy.ctypes.data) == A, "a side that sums to 257"
    assert sep(sp=None) == A and sep(n=-1) == A and sep(ss=31) == A and sep(dp=s) == A and sep(n=0) == 0

    # CannyEdgeDetection
    def ced(n=1, c=1, k=19, up=0.15, lo=0.01, it=1, sp=s, ss=64, w=32, h=20, dp=o, ds=64):
        return L.prl_hip_canny_edge_detection_batch_device(n, c, k, up, lo, it, sp, ss * h, ss, w, h, dp, ds * h, ds, None)

    def ced_host(c=1, k=19, up=0.15, lo=0.01, it=1, sp=s, ss=64, w=32, h=20, dp=o, ds=64, n=1):
        return L.prl_hip_canny_edge_detection_host(c, k, up, lo, it, sp, ss, w, h, dp, ds)

    for f in (ced, ced_host):
        assert f(w=0, k=2) == E
        assert f(k=2, c=9) == A and f(k=1) == A and f(k=-5) == A, "size < 3"
        assert f(up=1.5, k=4) == A and f(up=-0.1) == A and f(up=nan) == A and f(lo=1.5) == A and f(lo=nan) == A
        assert f(up=0.2, lo=0.5) == A and f(k=4) == A and f(k=18, c=9) == A, "lower > upper; an even size"
        assert f(k=257, c=9) == W
        assert f(c=0) == CH and f(c=5) == CH and f(c=5, it=300) == CH
        assert f(it=256) == A and f(it=-256) == A and f(sp=None) == A and f(dp=None) == A and f(c=3, ss=95) == A and f(ds=31) == A
        assert f(w=32769, ss=40000, ds=40000) == A and f(dp=s) == A
    assert ced(n=-1) == A and ced(n=0) == 0

    # the external rectangles (host code: a valid call answers PRL_OK with or without a device)
    fk = (ctypes.c_int * 2)(-1, -1)
    rb = np.zeros(16, np.int32)
    ip = ctypes.POINTER(ctypes.c_int)
    f_at, k_at = ctypes.cast(ctypes.addressof(fk), ip), ctypes.cast(ctypes.addressof(fk) + 4, ip)

    def er(mp=s, st=64, w=32, h=20, pr=rb.ctypes.data, mx=4, pf=f_at, pk=k_at):
        return L.prl_hip_external_rects(mp, st, w, h, pr, mx, pf, pk)

    assert er(w=0, mp=None) == E and er(h=-1, st=0) == E and er(w=0, mx=-1, pf=None) == E, "EMPTY comes first"
    assert er(mp=None) == A and er(st=31) == A and er(pf=None) == A and er(pk=None) == A and er(mx=-1) == A and er(pr=None) == A
    assert er(w=32769, st=40000) == A and er(h=32769) == A
    assert (fk[0], fk[1]) == (-1, -1), "a refused call writes nothing"
    assert er() == 0 and er(pr=None, mx=0) == 0 and (fk[0], fk[1]) == (0, 0)

    # the per-rectangle Otsu
    off = np.array([0, 1], np.int32)
    rc = np.array([0, 0, 4, 4], np.int32)   # (a host array stands for the device list: no valid call gets as far as reading it)

    def ro(n=1, po=off.ctypes.data, pr=rc.ctypes.data, mv=255.0, sp=s, ss=64, w=32, h=20, dp=o, ds=64):
        return L.prl_hip_rect_otsu_batch_device(n, po, pr, mv, sp, ss * h, ss, w, h, dp, ds * h, ds, None, None)

    assert ro(w=0, mv=300.0) == E
    assert ro(mv=255.5) == A and ro(mv=-1.0) == A and ro(mv=nan) == A
    assert ro(sp=None) == A and ro(dp=None) == A and ro(n=-1) == A and ro(ss=31) == A and ro(ds=31) == A and ro(dp=s) == A
    assert ro(po=None) == A and ro(pr=None) == A
    for bad in ([1, 2], [0, -1]):
        assert ro(po=np.array(bad, np.int32).ctypes.data) == A, bad
    assert ro(n=0, po=None, pr=None) == 0

    # the whole call
    cnt = np.zeros(4, np.int32)

    def lo_(n=1, c=1, mv=255.0, clip=0.0, k=19, up=0.15, low=0.01, it=1, sp=s, ss=64, w=32, h=20, dp=o, ds=64):
        return L.prl_hip_binarize_local_otsu_batch_device(n, c, mv, clip, k, up, low, it, sp, ss * h, ss, w, h, dp, ds * h, ds,
                                                          cnt.ctypes.data, cnt.ctypes.data + 8, None)

    def lo_host(c=1, mv=255.0, clip=0.0, k=19, up=0.15, low=0.01, it=1, sp=s, ss=64, w=32, h=20, dp=o, ds=64, n=1):
        return L.prl_hip_binarize_local_otsu_host(c, mv, clip, k, up, low, it, sp, ss, w, h, dp, ds, cnt.ctypes.data, cnt.ctypes.data + 8)

    for f in (lo_, lo_host):
        assert f(w=0, mv=300.0) == E
        assert f(mv=255.5, k=2, c=2) == A and f(mv=nan) == A
        assert f(k=2, c=2) == A and f(up=1.5, k=4) == A and f(low=2.0) == A and f(up=0.1, low=0.2) == A and f(k=4, c=2) == A
        assert f(k=257, c=2) == W
        assert f(c=2) == CH and f(c=0) == CH and f(c=5) == CH
        assert f(clip=nan) == A and f(it=256) == A and f(sp=None) == A and f(dp=None) == A and f(c=3, ss=95) == A and f(ds=31) == A
        assert f(dp=s) == A and f(w=32769, ss=40000, ds=40000) == A
    assert lo_(n=-1) == A and lo_(n=0) == 0

    if no_gpu:   # every check passed: the device is asked for, and there is none
        assert blur() == N and blur_host() == N and sep() == N and ced() == N and ced_host() == N and lo_() == N and lo_host() == N
        assert blur(c=4, kw=255, kh=1, sx=3.0, ss=128, ds=128) == N and ced(c=4, k=3, up=1.0, lo=1.0, it=-255, ss=128) == N and ro() == N
        assert lo_(c=4, mv=0.0, clip=2.0, k=255, up=0.0, low=0.0, it=0, ss=128) == N
        assert (out == 0).all() and (cnt == 0).all()


def test_exports_maps_and_python(prl):
    from prlib_amd import _capi

    so = os.path.join(ROOT, "prlib_amd", "libprlib_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(ROOT, "include", "prl_hip.h")).read()
    for name in SYMBOLS:
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(_capi.lib(), name)
        assert re.search(r"\bT " + name + r"\b", out), name
        assert re.search(r"^int " + name + r"\(", header, flags=re.M), name
        for m in ("prl_hip.map", "prl_hip_testhooks.map"):
            assert re.search(r"^\s+" + name + ";$", open(os.path.join(ROOT, "prlib_amd", "csrc", m)).read(), flags=re.M), (name, m)
    assert _capi.lib().prl_hip_abi_version() == 4
    for fn in ("binarizeLocalOtsu", "cannyEdgeDetection", "externalRects", "gaussianBlurU8", "gaussianKernelU8", "rectOtsu", "sepFilterU8"):
        assert callable(getattr(prl, fn)) and fn in prl.__all__
    small = int(re.search(r"^#define PRL_RECT_OTSU_SMALL_AREA (\d+)", header, flags=re.M).group(1))
    from prlib_amd import localotsu

    assert small == localotsu.RECT_OTSU_SMALL_AREA and int(re.search(r"^#define PRL_GAUSS_MAX_SIDE (\d+)", header, flags=re.M).group(1)) == lr.MAX_SIDE


def test_python_layer_refuses_before_any_device(prl):
    from prlib_amd import _capi

    img = np.zeros((40, 48, 3), np.uint8)
    for call, status in ((lambda: prl.gaussianBlurU8(img, (4, 3)), _capi.PRL_ERR_BAD_WINDOW),
                         (lambda: prl.cannyEdgeDetection(img, 18), _capi.PRL_ERR_BAD_ARG),
                         (lambda: prl.binarizeLocalOtsu(img, 256.0), _capi.PRL_ERR_BAD_ARG),
                         (lambda: prl.binarizeLocalOtsu(img[:, :, :2]), _capi.PRL_ERR_BAD_CHANNELS),
                         (lambda: prl.gaussianKernelU8(8), _capi.PRL_ERR_BAD_WINDOW)):
        with pytest.raises(_capi.PrlError) as e:
            call()
        assert e.value.status == status
    assert prl.gaussianKernelU8(19).tolist() == TABLES[19] and prl.gaussianKernelU8(19).dtype == np.uint16


# ---- the C++ layer and the stand-alone program ------------------------------------------------------------------------------------

def build_dropin(out_dir):
    """g++ of tests/cpp/test_localotsu_dropin.cpp + prl_host.cpp, with only -I include/prl for the drop-in header."""
    exe = os.path.join(out_dir, "test_localotsu_dropin")
    flags = []
    for pc in ("opencv4", "opencv"):
        r = subprocess.run(["pkg-config", "--cflags", "--libs", pc], capture_output=True, text=True) if shutil.which("pkg-config") else None
        if r is not None and r.returncode == 0:
            flags = r.stdout.split()
            break
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include", "prl"),
           os.path.join(ROOT, "tests", "cpp", "test_localotsu_dropin.cpp"), os.path.join(ROOT, "prlib_amd", "csrc", "prl", "prl_host.cpp"),
           ] + flags + ["-L", os.path.join(ROOT, "prlib_amd"), "-lprlib_hip", "-Wl,-rpath," + os.path.join(ROOT, "prlib_amd"),
                        "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_dropin_header_contract_without_device(prl, tmp_path):
    import torch

    src = open(os.path.join(ROOT, "tests", "cpp", "test_localotsu_dropin.cpp")).read()
    assert '#include "binarizeLocalOtsu.h"' in src, "the reference's include line"
    decl = re.sub(r"\s+", " ", open(os.path.join(ROOT, "prlib_amd", "csrc", "prl", "prl.h")).read())
    assert ("binarizeLocalOtsu(cv::Mat& inputImage, cv::Mat& outputImage, double maxValue = 255.0, double CLAHEClipLimit = 0.0, "
            "int GaussianBlurKernelSize = 19, double CannyUpperThresholdCoeff = 0.15, double CannyLowerThresholdCoeff = 0.01, "
            "int CannyMorphIters = 1)") in decl, "the reference's defaults"
    exe = build_dropin(str(tmp_path))
    if not torch.cuda.is_available():   # (with a device the valid calls of this mode would run: the GPU suite covers them)
        r = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "localotsu dropin cpu: OK" in r.stdout, r.stdout + r.stderr


def test_sanitized_program(tmp_path):
    """tests/cpp/test_localotsu.cpp under AddressSanitizer and UndefinedBehaviorSanitizer: a program of its own on the CPU"""
    exe = str(tmp_path / "test_localotsu")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "test_localotsu.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "localotsu: OK" in r.stdout, r.stdout + r.stderr[-3000:]
