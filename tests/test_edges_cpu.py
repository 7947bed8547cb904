"""cv::pyrDown, cv::Canny, the edge map of prl::documentContour and prl::resize without a device: the two models of
tests/edges_ref.py against each other and against answers worked out by hand, the host routines of the library against the
restatement, every status of the entries, and the exports."""
import ctypes as C
import os
import re
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import edges_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("prl_hip_pyr_down_size", "prl_hip_pyr_down_batch_device", "prl_hip_pyr_down_host", "prl_hip_canny_classes_batch_device",
               "prl_hip_edge_link_batch_device", "prl_hip_canny_batch_device", "prl_hip_canny_host", "prl_hip_document_edges_geometry",
               "prl_hip_document_edges_batch_device", "prl_hip_document_edges_host", "prl_hip_resize_pyramid_levels",
               "prl_hip_resize_replicate_batch_device", "prl_hip_resize_replicate_host")
# the first scan of tests/golden/scans as a colour page (er.colour_from_gray): chosen channel and CRC-32 of its edge map, recorded
# from the restatement (both of its models agree on it, test_recorded_document_edges)
SCAN = os.path.join(ROOT, "tests", "golden", "scans", "0004.npz")
SCAN_RECORD = {"size": (270, 400), "channel": 1, "crc": 0x1DBB82C4}


def blocks_page(h, w, seed, cell=3):
    """saturated 0 / 255 blocks: |dx| up to 1020 and plateaus of equal magnitude"""
    r = np.random.RandomState(seed)
    small = r.randint(0, 2, ((h + cell - 1) // cell, (w + cell - 1) // cell)).astype(np.uint8) * 255
    return np.ascontiguousarray(np.kron(small, np.ones((cell, cell), np.uint8))[:h, :w])


def random_page(h, w, seed, channels=None):
    r = np.random.RandomState(seed)
    return r.randint(0, 256, (h, w) if channels is None else (h, w, channels)).astype(np.uint8)


# ---- the two models ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (2, 9), (9, 2), (3, 8), (8, 3), (4, 4), (5, 6), (11, 13)])
def test_pyr_down_models_agree(shape):
    for ch in (None, 3):
        img = random_page(shape[0], shape[1], 7 + shape[0] * 31 + shape[1], ch)
        got = er.pyr_down(img)
        assert got.shape[:2] == ((shape[0] + 1) // 2, (shape[1] + 1) // 2)
        assert np.array_equal(got, er.pyr_down_loop(img))
    img = random_page(shape[0], shape[1], 3)
    assert np.array_equal(er.pyr_down(img, 2), er.pyr_down_loop(er.pyr_down_loop(img)))


def test_reflection_folds_more_than_once():
    for n in (1, 2, 3, 4, 5, 9):
        idx = np.arange(-12, 3 * n + 12)
        assert [er.reflect101(int(p), n) for p in idx] == er.reflect101_table(idx, n).tolist()
    assert [er.reflect101(p, 2) for p in (-2, -1, 0, 1, 2, 3)] == [0, 1, 0, 1, 0, 1]
    assert [er.reflect101(p, 3) for p in (-2, -1, 3, 4, 5)] == [2, 1, 1, 0, 1]


@pytest.mark.parametrize("thr", [(-1, -1), (0, 0), (25, 50), (50, 25), (2039, 2040), (2040, 2041)])
def test_canny_models_agree(thr):
    pages = [random_page(9, 11, 1), blocks_page(12, 10, 2), blocks_page(7, 13, 3, cell=2), random_page(1, 6, 4), random_page(6, 1, 5),
             (random_page(8, 8, 6) >> 5) << 5, random_page(10, 12, 8) >> 4]   # (the last: magnitudes on both sides of 25 and 50)
    for img in pages:
        cls = er.canny_classes(img, *thr)
        assert np.array_equal(cls, er.canny_classes_loop(img, *thr))
        assert np.array_equal(er.edge_link(cls), er.edge_link_loop(cls))
    assert any((er.canny_classes(p, 25, 50) == 0).any() and (er.canny_classes(p, 25, 50) == 2).any() for p in pages)


def test_edge_link_models_agree_on_hand_made_maps():
    r = np.random.RandomState(5)
    for _ in range(20):
        cls = r.choice(np.array([0, 0, 0, 1, 1, 1, 1, 2, 3], np.uint8), (9, 14))
        assert np.array_equal(er.edge_link(cls), er.edge_link_loop(cls))
    cls = np.ones((3, 6), np.uint8)
    cls[0, 5] = 0   # column W - 1 of row 0 ...
    cls[1, 0] = 2   # ... and column 0 of row 1 are no neighbours
    assert er.edge_link(cls).tolist() == [[0] * 6, [255, 0, 0, 0, 0, 0], [0] * 6]


# ---- known answers ----------------------------------------------------------------------------------------------------------------

def test_pyr_down_by_hand():
    for v in (0, 1, 127, 254, 255):
        assert (er.pyr_down(np.full((7, 10, 3), v, np.uint8)) == v).all()          # the weights sum to 256
        assert er.pyr_down(np.full((1, 1), v, np.uint8)).tolist() == [[v]]
    # 2 x 1 (W = 2, H = 1): the columns -2 .. 2 fold to 0 1 0 1 0, so r = 8 a + 8 b, v = 16 r, dst = (a + b + 1) >> 1
    assert er.pyr_down(np.array([[10, 13]], np.uint8)).tolist() == [[12]]
    assert er.pyr_down(np.array([[255, 254]], np.uint8)).tolist() == [[255]]
    # 5 x 1: r0 = 6 s0 + 8 s1 + 2 s2, r1 = s0 + 4 s1 + 6 s2 + 4 s3 + s4, r2 = 2 s2 + 8 s3 + 6 s4 (column 5 folds to 3, 6 to 2);
    # one row: v = 16 r, dst = (r + 8) >> 4: r = 192, 703, 1978
    assert er.pyr_down(np.array([[0, 16, 32, 48, 255]], np.uint8)).tolist() == [[12, 44, 124]]
    assert er.pyr_down(np.array([[0], [16], [32], [48], [255]], np.uint8)).tolist() == [[12], [44], [124]]


def test_step_edge_by_hand():
    """0 | 255 between columns 3 and 4: both columns have |dx| = 1020; column 3 passes m > left, m >= right, column 4 fails m > left"""
    img = np.zeros((6, 9), np.uint8)
    img[:, 4:] = 255
    want = np.zeros((6, 9), np.uint8)
    want[:, 3] = 255
    assert np.array_equal(er.canny(img, 25, 50), want) and np.array_equal(er.canny_loop(img, 25, 50), want)
    assert np.array_equal(er.canny(img, 1019, 1019), want)       # m = 1020 > 1019
    assert not er.canny(img, 1020, 1020).any()
    # the same edge lying down: the row above the step
    assert np.array_equal(er.canny(np.ascontiguousarray(img.T), 25, 50), want.T)


def test_thresholds_by_hand():
    img = blocks_page(12, 14, 9)
    flat = np.full((5, 7), 93, np.uint8)
    assert not er.canny(img, 0, 2040).any() and not er.canny(img, 2040, 5000).any() and not er.canny(img, 2040, float("inf")).any()
    assert (er.canny_classes(img, 0, 2040) == 0).any()           # candidates, and nothing to start from
    assert not er.canny(flat, -1, -1).any() and not er.canny(flat, -7.5, -3).any()   # no 0 > 0 holds
    assert (er.canny_classes(flat, -1, -1) == 1).all()
    assert np.array_equal(er.canny(img, 50, 25), er.canny(img, 25, 50))
    assert np.array_equal(er.canny(img, 25.9, 50.9), er.canny(img, 25, 50))
    assert er.canny_thresholds(25.9, 50.9) == (25, 50) and er.canny_thresholds(-0.5, 1e30) == (-1, 2041)
    assert er.canny_thresholds(float("-inf"), float("inf")) == (-1, 2041) and er.canny_thresholds(60, 3) == (3, 60)


def gradient_page(dx, dy):
    """5 x 5, base 128: the right neighbour of the centre raised by dx / 2 and the lower one by dy / 2 give the centre exactly dx, dy"""
    assert dx % 2 == 0 and dy % 2 == 0
    img = np.full((5, 5), 128, np.uint8)
    img[2, 3] = 128 + dx // 2
    img[3, 2] = 128 + dy // 2
    return img


def test_direction_boundaries():
    """tg 22.5 deg lies between 12 / 29 and 5 / 12, tg 67.5 deg between 12 / 5 and 29 / 12.  A Sobel pair has an even sum (dx + dy =
    2 (i - a + f - d + h - b) over the 3 x 3 neighbourhood), so no page gives a pixel (29, 12) or (12, 5): the rule itself is held on
    those pairs, and pages are built for the doubled pairs, whose comparisons are the same ones scaled by two."""
    for sx in (1, -1):
        for sy in (1, -1):
            assert er.direction(29 * sx, 12 * sy) == 0 and er.direction(12 * sx, 5 * sy) == 2
            assert er.direction(5 * sx, 12 * sy) == 2 and er.direction(12 * sx, 29 * sy) == 1
            for (dx, dy), want in (((58, 24), 0), ((24, 10), 2), ((10, 24), 2), ((24, 58), 1)):
                img = gradient_page(dx * sx, dy * sy)
                gx, gy, _m = er.gradients(img)
                assert (gx[2, 2], gy[2, 2]) == (dx * sx, dy * sy)
                cls, branch = er.canny_classes(img, 0, 0, with_branch=True)
                assert branch[2, 2] == want
                assert np.array_equal(cls, er.canny_classes_loop(img, 0, 0))


def test_geometry_by_hand(prl):
    want = {(511, 100): (0, 511, 100), (100, 511): (0, 100, 511), (512, 3): (1, 256, 2), (1023, 1023): (2, 256, 256),
            (1024, 700): (2, 256, 175), (2480, 3508): (3, 310, 439), (1, 5000): (4, 1, 313)}
    for (w, h), g in want.items():
        assert er.document_edges_geometry(w, h) == g and prl.document_edges_geometry(w, h) == g
    r = np.random.RandomState(1)
    for w, h in r.randint(1, 9000, (200, 2)):
        assert prl.document_edges_geometry(int(w), int(h)) == er.document_edges_geometry(int(w), int(h))
        for levels in (1, 2, 5):
            sz = er.pyr_down(np.zeros((int(h) % 40 + 1, int(w) % 40 + 1), np.uint8), levels).shape
            assert prl.pyr_down_size(int(w) % 40 + 1, int(h) % 40 + 1, levels) == (sz[1], sz[0])
        ms = int(r.randint(1, 3000))
        assert prl.resize_pyramid_levels(int(w), int(h), ms) == er.resize_pyramid_levels(int(w), int(h), ms)
    assert prl.resize_pyramid_levels(2480, 3508, 1024) == (2, 620, 877) and prl.resize_pyramid_levels(1024, 1024, 1024) == (0, 1024, 1024)


def test_channel_choice():
    g = random_page(20, 30, 3)
    assert er.most_informative_channel(np.stack([g, g, g], axis=2)) == 0          # an exact tie: the first
    assert er.most_informative_channel(np.stack([g >> 1, g, g >> 2], axis=2)) == 1
    assert er.most_informative_channel(np.stack([g >> 1, g >> 2, g, g], axis=2)) == 2
    assert er.most_informative_channel(np.full((4, 4, 3), 9, np.uint8)) == 0
    assert er.most_informative_channel(g) == 0


def test_resize_tables():
    assert er.replicate_table(5, 1).tolist() == [0, 1, 2, 3, 4]
    assert er.replicate_table(3, 2).tolist() == [0, 0, 1, 1, 2, 2]
    assert er.replicate_table(2, 3).tolist() == [0, 0, 0, 1, 1, 1]
    assert 49.0 * (1.0 / 49.0) < 1.0
    t = er.replicate_table(2, 49)
    assert t[:49].tolist() == [0] * 49 and t[49] == 0 and t[50:].tolist() == [1] * 48   # column 49 copies source column 0
    img = random_page(3, 2, 1, 3)
    assert np.array_equal(er.resize(img, 1, 1, 0), img)
    assert np.array_equal(er.resize(img, 2, 3, 0), np.repeat(np.repeat(img, 3, axis=0), 2, axis=1))
    assert np.array_equal(er.resize(img, 0, 3, 2), er.pyr_down(img)) and np.array_equal(er.resize(img, -1, -1, 3), img)


def test_recorded_document_edges():
    gray = np.load(SCAN)["gray"]
    page = er.colour_from_gray(gray)
    edges, ch = er.document_edges(page)
    assert (edges.shape[1], edges.shape[0]) == SCAN_RECORD["size"] == er.document_edges_geometry(gray.shape[1], gray.shape[0])[1:]
    assert ch == SCAN_RECORD["channel"]
    assert zlib.crc32(edges.tobytes()) == SCAN_RECORD["crc"]
    small = np.ascontiguousarray(er.pyr_down(page, 2)[:, :, ch])
    assert np.array_equal(edges, er.edge_link_loop(er.canny_classes(small, 25, 50)))
    crop = np.ascontiguousarray(small[100:148, 60:112])
    assert np.array_equal(er.canny_classes(crop, 25, 50), er.canny_classes_loop(crop, 25, 50))
    assert 0 < (edges == 255).mean() < 0.5


# ---- statuses, exports ---------------------------------------------------------------------------------------------------------------

def test_statuses_without_touching_a_device(prl):
    """every status of every new entry, one wrong field at a time and in the documented order; the arguments that pass them all
    reach the device check"""
    import torch

    from prlib_amd import _capi

    L, E = _capi.lib(), _capi
    src = np.zeros((8, 12, 4), np.uint8)
    dst = np.zeros((64, 64, 4), np.uint8)
    ch = np.zeros(4, np.int32)
    sp, dp = src.ctypes.data, dst.ctypes.data

    def pyr(n=1, c=3, levels=1, s=sp, step=48, w=12, h=8, d=dp, dstep=256):
        return L.prl_hip_pyr_down_batch_device(n, c, levels, s, 0, step, w, h, d, 0, dstep, None)

    def pyr_host(n=1, c=3, levels=1, s=sp, step=48, w=12, h=8, d=dp, dstep=256):
        return L.prl_hip_pyr_down_host(c, levels, s, step, w, h, d, dstep)

    def classes(n=1, c=1, t1=25.0, t2=50.0, s=sp, step=48, w=12, h=8, d=dp, dstep=256):
        return L.prl_hip_canny_classes_batch_device(n, c, t1, t2, s, 0, step, w, h, d, 0, dstep, None)

    def canny(n=1, c=1, t1=25.0, t2=50.0, s=sp, step=48, w=12, h=8, d=dp, dstep=256):
        return L.prl_hip_canny_batch_device(n, c, t1, t2, s, 0, step, w, h, d, 0, dstep, None)

    def canny_host(n=1, c=1, t1=25.0, t2=50.0, s=sp, step=48, w=12, h=8, d=dp, dstep=256):
        return L.prl_hip_canny_host(c, t1, t2, s, step, w, h, d, dstep)

    def link(n=1, c=1, s=sp, step=48, w=12, h=8, d=dp, dstep=256):
        return L.prl_hip_edge_link_batch_device(n, s, 0, step, w, h, d, 0, dstep, None, None)

    def doc(n=1, c=3, s=sp, step=48, w=12, h=8, d=dp, dstep=256, o=ch.ctypes.data):
        return L.prl_hip_document_edges_batch_device(n, c, s, 0, step, w, h, d, 0, dstep, o, None)

    def doc_host(n=1, c=3, s=sp, step=48, w=12, h=8, d=dp, dstep=256, o=ch.ctypes.data):
        return L.prl_hip_document_edges_host(c, s, step, w, h, d, dstep, o)

    def rep(n=1, c=3, fx=2, fy=2, s=sp, step=48, w=12, h=8, d=dp, dstep=256):
        return L.prl_hip_resize_replicate_batch_device(n, c, fx, fy, s, 0, step, w, h, d, 0, dstep, None)

    def rep_host(n=1, c=3, fx=2, fy=2, s=sp, step=48, w=12, h=8, d=dp, dstep=256):
        return L.prl_hip_resize_replicate_host(c, fx, fy, s, step, w, h, d, dstep)

    batch = (pyr, classes, canny, link, doc, rep)
    hosts = (pyr_host, canny_host, doc_host, rep_host)
    for fn in batch + hosts:
        assert fn(w=0) == E.PRL_ERR_EMPTY and fn(h=-1) == E.PRL_ERR_EMPTY and fn(w=0, h=0) == E.PRL_ERR_EMPTY
        assert fn(w=0, c=9, s=None) == E.PRL_ERR_EMPTY                                   # the order of the checks
        assert fn(s=None) == E.PRL_ERR_BAD_ARG and fn(d=None) == E.PRL_ERR_BAD_ARG
        assert fn(w=32769, step=1 << 20, dstep=1 << 20) == E.PRL_ERR_BAD_ARG and fn(h=32769) == E.PRL_ERR_BAD_ARG
    for fn in batch:
        assert fn(n=-1) == E.PRL_ERR_BAD_ARG and fn(n=0) == E.PRL_OK
        assert fn(d=sp) == E.PRL_ERR_BAD_ARG and fn(d=sp + 40) == E.PRL_ERR_BAD_ARG      # in place, and any shared byte
    for fn in (pyr, pyr_host, rep, rep_host):
        assert fn(c=0) == E.PRL_ERR_BAD_CHANNELS and fn(c=5) == E.PRL_ERR_BAD_CHANNELS and fn(c=5, s=None) == E.PRL_ERR_BAD_CHANNELS
        assert fn(step=35) == E.PRL_ERR_BAD_ARG
    for fn in (classes, canny, canny_host):
        for c in (0, 2, 3, 4, 5):
            assert fn(c=c) == E.PRL_ERR_BAD_CHANNELS
        assert fn(c=3, t1=float("nan")) == E.PRL_ERR_BAD_CHANNELS
        assert fn(t1=float("nan")) == E.PRL_ERR_BAD_ARG and fn(t2=float("nan")) == E.PRL_ERR_BAD_ARG
    for fn in (classes, canny, canny_host, link):
        assert fn(step=11) == E.PRL_ERR_BAD_ARG and fn(dstep=11) == E.PRL_ERR_BAD_ARG
    for fn in (doc, doc_host):
        for c in (0, 2, 5):
            assert fn(c=c) == E.PRL_ERR_BAD_CHANNELS
        assert fn(step=35) == E.PRL_ERR_BAD_ARG and fn(dstep=11) == E.PRL_ERR_BAD_ARG and fn(o=None) == E.PRL_ERR_BAD_ARG
        assert fn(w=600, h=2, step=1800, dstep=299) == E.PRL_ERR_BAD_ARG                 # one level: 300 columns
    for fn in (pyr, pyr_host):
        assert fn(levels=0) == E.PRL_ERR_BAD_ARG and fn(levels=-1) == E.PRL_ERR_BAD_ARG and fn(levels=17) == E.PRL_ERR_BAD_ARG
        assert fn(dstep=17) == E.PRL_ERR_BAD_ARG and fn(levels=2, dstep=8) == E.PRL_ERR_BAD_ARG
    for fn in (rep, rep_host):
        assert fn(fx=0) == E.PRL_ERR_BAD_ARG and fn(fy=-2) == E.PRL_ERR_BAD_ARG and fn(dstep=71) == E.PRL_ERR_BAD_ARG
        assert fn(fx=2731, dstep=1 << 20) == E.PRL_ERR_BAD_ARG and fn(fy=4097) == E.PRL_ERR_BAD_ARG   # 12 * 2731, 8 * 4097 > 32768
    i = C.c_int(-7)
    ref = C.byref(i)
    assert L.prl_hip_pyr_down_size(0, 4, 1, ref, ref) == E.PRL_ERR_EMPTY and L.prl_hip_pyr_down_size(4, 4, 0, ref, ref) == E.PRL_ERR_BAD_ARG
    assert L.prl_hip_pyr_down_size(4, 4, 1, None, ref) == E.PRL_ERR_BAD_ARG
    assert L.prl_hip_document_edges_geometry(4, 0, ref, ref, ref) == E.PRL_ERR_EMPTY
    assert L.prl_hip_document_edges_geometry(4, 4, ref, None, ref) == E.PRL_ERR_BAD_ARG
    assert L.prl_hip_resize_pyramid_levels(4, -1, 9, ref, ref, ref) == E.PRL_ERR_EMPTY
    assert L.prl_hip_resize_pyramid_levels(4, 4, 9, None, ref, ref) == E.PRL_ERR_BAD_ARG
    for ms in (0, -1, -(2 ** 31)):
        assert L.prl_hip_resize_pyramid_levels(4, 4, ms, ref, ref, ref) == E.PRL_ERR_BAD_ARG
    assert i.value == -7                                                                  # nothing was written
    with pytest.raises(_capi.PrlError):
        prl.resize(np.zeros((4, 4), np.uint8), 0, 0, 0)
    if not torch.cuda.is_available():   # valid arguments get as far as the device
        for fn in batch + hosts:
            assert fn() == E.PRL_ERR_NO_DEVICE
        assert classes(t1=float("inf"), t2=-float("inf")) == E.PRL_ERR_NO_DEVICE and pyr(c=2, levels=16) == E.PRL_ERR_NO_DEVICE


def build_dropin(out_dir):
    """g++ of tests/cpp/test_resize_dropin.cpp + prl_host.cpp, with only -I include/prl for the drop-in header."""
    exe = os.path.join(out_dir, "test_resize_dropin")
    flags = []
    for pc in ("opencv4", "opencv"):
        r = subprocess.run(["pkg-config", "--cflags", "--libs", pc], capture_output=True, text=True) if shutil.which("pkg-config") else None
        if r is not None and r.returncode == 0:
            flags = r.stdout.split()
            break
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include", "prl"),
           os.path.join(ROOT, "tests", "cpp", "test_resize_dropin.cpp"), os.path.join(ROOT, "prlib_amd", "csrc", "prl", "prl_host.cpp"),
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
    assert os.path.exists(os.path.join(ROOT, "include", "prl", "resize.h"))
    if torch.cuda.is_available():
        pytest.skip("a device is present; the no-device behaviour is checked on the CPU box")
    r = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "resize dropin cpu: OK" in r.stdout, r.stdout + r.stderr


def test_exports_maps_and_python(prl):
    from prlib_amd import _capi

    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "prlib_amd", "libprlib_hip.so")], capture_output=True, text=True,
                         check=True).stdout
    for name in NEW_EXPORTS:
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(_capi.lib(), name)
        assert re.search(r"\bT " + name + r"\b", out), name
        for m in ("prl_hip.map", "prl_hip_testhooks.map"):
            assert re.search(r"^\s+" + name + ";$", open(os.path.join(ROOT, "prlib_amd", "csrc", m)).read(), flags=re.M), (name, m)
    assert _capi.lib().prl_hip_abi_version() == 4
    for fn in ("pyr_down", "pyr_down_size", "canny", "canny_classes", "edge_link", "document_edges", "document_edges_geometry", "resize",
               "resize_pyramid_levels"):
        assert callable(getattr(prl, fn)) and fn in prl.__all__
    for f in ("pyr.hip", "canny.hip", "border.hip"):
        assert f in open(os.path.join(ROOT, "prlib_amd", "csrc", "Makefile")).read()
        assert f[:-4] in re.search(r"set\(PRL_KERNELS ([^)]*)\)", open(os.path.join(ROOT, "CMakeLists.txt")).read()).group(1).split()
