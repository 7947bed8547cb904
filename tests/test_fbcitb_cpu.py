"""prl::binarizeFBCITB's host half without a device: cv::findContours(RETR_TREE) of contour.h against the flood-fill statement of the
topological tree in tests/fbcitb_ref.py (all 65 536 maps of 4 x 4, nested rings, more than 127 borders, seeded random maps), against
the RETR_CCOMP and RETR_EXTERNAL scanners already in the tree, RemoveChildrenContours on hand-built hierarchies, every kept
contour's cut and polarity, the argument that the background list is never empty, the ordered paint as a loop, bilateral.h's loop
against the numpy restatement, the stand-alone program under the address and undefined-behaviour sanitizers, the exports and the
drop-in header.  Every comparison is an equality."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import fbcitb_ref as fr
from test_bilateral_cpu import SENSITIVE, sensitive_page

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("prl_hip_variance_mask_batch_device", "prl_hip_find_contours_tree", "prl_hip_remove_children_contours", "prl_hip_fbcitb_contours",
           "prl_hip_rect_paint_batch_device", "prl_hip_default_fbcitb_params", "prl_hip_binarize_fbcitb_batch_device",
           "prl_hip_binarize_fbcitb_host")


def _tuples(a):
    return [tuple(int(v) for v in p) for p in np.asarray(a).reshape(-1, 2)]


def compare_tree(prl, page, name=""):
    want = fr.contour_tree(page)
    contours, hier, holes = prl.findContoursTree(page)
    assert len(contours) == len(want), (name, len(contours), len(want))
    for k, nd in enumerate(want):
        assert bool(holes[k]) == nd["hole"] and _tuples(contours[k]) == nd["points"], (name, k)
        assert tuple(hier[k].tolist()) == (nd["next"], nd["prev"], nd["child"], nd["parent"]), (name, k, hier[k].tolist(), nd)
    return contours, hier, holes


# ---- the contour tree --------------------------------------------------------------------------------------------------------------

def test_all_maps_of_4_by_4(prl):
    """every 4 x 4 map, each on a cell of its own of one large page (two background pixels between neighbours, so no map touches
    another): one tree of 65 536 independent subtrees, the top level in reverse order of discovery"""
    side, pitch = 256, 6
    page = np.zeros((side * pitch, side * pitch), np.uint8)
    bits = np.arange(65536, dtype=np.uint32)
    for i in range(16):
        on = ((bits >> i) & 1).astype(bool).reshape(side, side)
        page[1 + i // 4::pitch, 1 + i % 4::pitch][:side, :side][on] = 255
    assert (page[1:5, 1:5] == 0).all() and (page[pitch * 255 + 1:pitch * 255 + 5, pitch * 255 + 1:pitch * 255 + 5] == 255).all()
    _contours, hier, holes = compare_tree(prl, page, "4x4")
    assert (hier[:, 3] == -1).sum() >= 65535 - 1 and holes.any()


def test_nested_rings_and_blobs_in_holes(prl):
    for depth in (1, 2, 3):
        page = fr.nested_rings(depth)
        _c, hier, holes = compare_tree(prl, page, "rings%d" % depth)
        assert len(hier) == 2 * depth + 2
        assert hier[:2 * depth, 3].tolist() == list(range(-1, 2 * depth - 1)), "ring, hole, ring, hole ... each the child of the one before"
        assert holes[:2 * depth].tolist() == [False, True] * depth
        assert hier[2 * depth:, 3].tolist() == [2 * depth - 1] * 2, "the two blobs lie in the innermost hole"
    two = np.zeros((9, 20), np.uint8)   # two rings side by side, a blob in the second: siblings come last discovered first
    two[1:8, 1:8] = 255
    two[2:7, 2:7] = 0
    two[1:8, 10:19] = 255
    two[2:7, 11:18] = 0
    two[4, 14] = 255
    _c, hier, holes = compare_tree(prl, two, "two")
    assert holes.tolist() == [False, True, False, False, True] and hier[:, 3].tolist() == [-1, 0, 1, -1, 3]


def test_more_than_127_borders(prl):
    """OpenCV's border numbers have 7 bits; the topological parents do not care: 144 blobs in one hole, and 130 rings in a row"""
    page = np.zeros((30, 30), np.uint8)
    page[0, :] = page[-1, :] = page[:, 0] = page[:, -1] = 255
    page[3:27:2, 3:27:2] = 255
    _c, hier, holes = compare_tree(prl, page, "blobs")
    assert len(hier) == 146 and (hier[2:, 3] == 1).all() and holes.tolist() == [False, True] + [False] * 144
    row = np.zeros((5, 4 * 130 + 1), np.uint8)
    for k in range(130):
        row[1:4, 4 * k + 1:4 * k + 4] = 255
        row[2, 4 * k + 2] = 0
    _c, hier, holes = compare_tree(prl, row, "rings in a row")
    assert len(hier) == 260 and holes.tolist() == [False, True] * 130


def test_seeded_random_maps(prl):
    rng = np.random.default_rng(2024)
    for k in range(400):
        h, w = int(rng.integers(1, 25)), int(rng.integers(1, 32))
        page = np.where(rng.random((h, w)) < rng.choice([0.2, 0.5, 0.7, 0.9]), 255, 0).astype(np.uint8)
        compare_tree(prl, page, "random%d" % k)


def test_agrees_with_the_ccomp_and_external_scanners(prl):
    """the same borders as prl.find_contours (RETR_CCOMP), every outer border followed by the same holes in the same order; and on
    maps without nesting the top level is prl.externalRects' contours, last discovered first"""
    rng = np.random.default_rng(7)
    for k in range(150):
        h, w = int(rng.integers(3, 25)), int(rng.integers(3, 32))
        page = np.where(rng.random((h, w)) < 0.6, 255, 0).astype(np.uint8)
        contours, hier, holes = prl.findContoursTree(page)
        flat = prl.find_contours(page)
        assert sorted((bool(hl), _tuples(c)) for c, hl in zip(contours, holes)) == sorted((hl, _tuples(c)) for c, hl in flat), k
        by_outer, cur = {}, None
        for pts, hole in flat:   # RETR_CCOMP: an outer border, then its component's holes
            if not hole:
                cur = tuple(_tuples(pts))
                by_outer[cur] = []
            else:
                by_outer[cur].append(_tuples(pts))
        for i in range(len(contours)):
            if not holes[i]:
                kids, c = [], int(hier[i, 2])
                while c >= 0:
                    kids.append(_tuples(contours[c]))
                    c = int(hier[c, 0])
                assert kids == by_outer[tuple(_tuples(contours[i]))], (k, i)
    for k in range(60):   # filled rectangles that do not touch: no holes, no nesting
        page = np.zeros((40, 50), np.uint8)
        for _ in range(int(rng.integers(1, 9))):
            x, y, w, h = int(rng.integers(0, 44)), int(rng.integers(0, 34)), int(rng.integers(1, 6)), int(rng.integers(1, 6))
            if not page[max(y - 1, 0):y + h + 1, max(x - 1, 0):x + w + 1].any():
                page[y:y + h, x:x + w] = 255
        contours, hier, holes = prl.findContoursTree(page)
        assert not holes.any() and (hier[:, 3] == -1).all()
        rects, found = prl.externalRects(page)
        assert found == len(contours)
        mine = [(c[:, 0].min(), c[:, 1].min(), np.ptp(c[:, 0]) + 1, np.ptp(c[:, 1]) + 1) for c in contours if len(c) >= 3]
        assert [tuple(int(v) for v in r) for r in mine][::-1] == [tuple(int(v) for v in r) for r in rects], k


# ---- RemoveChildrenContours ----------------------------------------------------------------------------------------------------------

def family(top_points, n_children, grandchildren):
    """contour 0 with n_children children of 4 points, the first of which has `grandchildren` children: (counts, hierarchy)"""
    counts, hier = [top_points], [[-1, -1, 1 if n_children else -1, -1]]
    prev = -1
    for c in range(n_children):
        at = len(hier)
        counts.append(4)
        hier.append([-1, prev, -1, 0])
        if prev >= 0:
            hier[prev][0] = at
        prev = at
        if c == 0:
            gprev = -1
            for _ in range(grandchildren):
                ga = len(hier)
                counts.append(4)
                hier.append([-1, gprev, -1, at])
                if gprev >= 0:
                    hier[gprev][0] = ga
                else:
                    hier[at][2] = ga
                gprev = ga
    return counts, hier


@pytest.mark.parametrize("top, kids, grand, want", [
    (10, 5, 0, [0]),                       # 5 descendants: approved, the direct children ignored
    (10, 6, 0, [1, 2, 3, 4, 5, 6]),        # 6: ignored, the walk descends and approves the childless children
    (10, 3, 2, [0]),                       # 5 over two levels: the grandchildren are never visited, hence not kept
    (10, 2, 7, [2, 3, 4, 5, 6, 7, 8, 9]),  # 9: down; the first child has 7: down again; its sibling has none
    (10, 0, 0, [0]),
    (2, 0, 0, []),                         # fewer than 3 points
])
def test_remove_children_on_hand_built_hierarchies(prl, top, kids, grand, want):
    counts, hier = family(top, kids, grand)
    assert [i for i, ok in enumerate(fr.remove_children(counts, hier)) if ok] == want
    assert np.flatnonzero(prl.removeChildrenContours(counts, hier)).tolist() == want


def test_remove_children_short_contour_at_index_0_and_random_trees(prl):
    counts, hier = family(2, 6, 0)         # contour 0 is short: ignored, its children never visited; its sibling is reached
    counts.append(5)
    hier.append([-1, 0, -1, -1])
    hier[0][0] = 7
    assert np.flatnonzero(prl.removeChildrenContours(counts, hier)).tolist() == [7]
    assert [i for i, ok in enumerate(fr.remove_children(counts, hier)) if ok] == [7]
    assert prl.removeChildrenContours([], np.zeros((0, 4), np.int32)).tolist() == []
    rng = np.random.default_rng(3)
    for _ in range(200):   # random trees in pre-order, from the parents
        n = int(rng.integers(1, 40))
        parent = [-1] + [int(rng.integers(-1, i)) for i in range(1, n)]
        kids = {}
        for i, p in enumerate(parent):
            kids.setdefault(p, []).append(i)
        order = []
        stack = list(reversed(kids.get(-1, [])))
        while stack:
            i = stack.pop()
            order.append(i)
            stack.extend(reversed(kids.get(i, [])))
        pos = {i: k for k, i in enumerate(order)}
        hier = [[-1, -1, -1, -1] for _ in range(n)]
        for p, ks in kids.items():
            for a, i in enumerate(ks):
                hier[pos[i]] = [pos[ks[a + 1]] if a + 1 < len(ks) else -1, pos[ks[a - 1]] if a else -1,
                                pos[kids[i][0]] if i in kids else -1, -1 if p < 0 else pos[p]]
        counts = [int(rng.integers(1, 6)) for _ in range(n)]
        assert prl.removeChildrenContours(counts, hier).tolist() == fr.remove_children(counts, hier)


# ---- the decisions and the paint ---------------------------------------------------------------------------------------------------

def test_cut_and_polarity_per_contour(prl):
    from prlib_amd import synth

    pages = [synth.text_page_numpy(120, 160, 30), synth.text_page_numpy(90, 120, 3)]
    for page in pages:
        for canny, variances in ((False, True), (True, False)):
            _m, counts, st = fr.binarize_fbcitb(page, canny, variances, stages=True)
            want, want_counts = fr.contour_rects(fr.contour_tree(st["map"]), st["gray"])
            assert want_counts == counts and counts[2] >= 5
            rects, got_counts = prl.fbcitbContours(st["map"], st["gray"])
            assert got_counts == counts and [tuple(r) for r in rects.tolist()] == want
            assert {r[5] for r in want} <= {0, 1} and all(0 <= r[4] <= 255 for r in want)
    # a dark frame on a light ground and a light frame on a dark ground: F = 40 < B = 220 keeps p >= 40; F = 200 >= B = 30 keeps p < 200
    for fg, bg, below in ((40, 220, 0), (200, 30, 1)):
        gray = np.full((24, 30), bg, np.uint8)
        cmap = np.zeros((24, 30), np.uint8)
        cmap[8:14, 10:18] = 255
        cmap[9:13, 11:17] = 0
        gray[cmap == 255] = fg
        rects, counts = prl.fbcitbContours(cmap, gray)
        assert counts == (2, 1, 1) and rects.tolist() == [[10, 8, 8, 6, fg, below]]
        assert fr.contour_rects(fr.contour_tree(cmap), gray)[0] == [(10, 8, 8, 6, fg, below)]
    # a mean that is not an integer: points 10, 10, 11 around a triangle give F = 10.333..., cut 11
    gray = np.full((20, 20), 10, np.uint8)
    cmap = np.zeros((20, 20), np.uint8)
    for k in range(5):
        cmap[5 + k, 5:6 + k] = 255
    nodes = fr.contour_tree(cmap)
    gray[nodes[0]["points"][0][1], nodes[0]["points"][0][0]] = 11
    rects, counts = prl.fbcitbContours(cmap, gray)
    assert [tuple(r) for r in rects.tolist()] == fr.contour_rects(nodes, gray)[0] and rects[0, 4] == 11 and rects[0, 5] == 1
    rects, counts = prl.fbcitbContours(cmap, gray, 15.0 / 400)
    assert counts == (1, 1, 0), "area 25 is not below int(15)"


def test_the_background_list_is_never_empty():
    """every rectangle that passes the width and height filters on pages of 1 .. 14 columns and rows has a corner neighbour on the
    page: the filters leave at least two columns outside the rectangle"""
    for W in range(1, 15):
        for H in range(1, 15):
            for w in range(1, W + 1):
                for h in range(1, H + 1):
                    if not (w < int(0.8 * W) and h < int(0.8 * H)):
                        continue
                    assert W - w >= 2 and H - h >= 2
                    for x in range(W - w + 1):
                        for y in range(H - h + 1):
                            assert any(0 <= qx < W and 0 <= qy < H for qx, qy in fr.corner_neighbours(x, y, w, h)), (W, H, x, y, w, h)


def test_the_ordered_paint_as_a_loop():
    gray = fr.noise(30, 40, 1, 4)
    a, b = (5, 5, 20, 15, 128, 0), (15, 10, 20, 15, 128, 1)
    first, second = fr.paint(gray, [a, b]), fr.paint(gray, [b, a])
    over = (slice(10, 20), slice(15, 25))
    assert np.array_equal(first[over], np.where(gray[over] < 128, 255, 0)), "the later rectangle wins where they overlap"
    assert np.array_equal(second[over], np.where(gray[over] >= 128, 255, 0))
    assert not np.array_equal(first, second), "swapping two indices changes the mask"
    assert np.array_equal(first[over] ^ 255, second[over]) and (first[0] == 255).all()
    assert (fr.paint(gray, [(0, 0, 40, 30, 0, 0)]) == 255).all() and (fr.paint(gray, [(0, 0, 40, 30, 0, 1)]) == 0).all()
    assert (fr.paint(gray, [(-1, 0, 3, 3, 0, 1), (38, 0, 3, 3, 0, 1)]) == 255).all(), "not on the page: ignored"


def test_variance_cut_meets_the_float32_map():
    """the mask as integers: the restatement's float32 comparison is monotone in D = 9 sum(p^2) - sum(p)^2"""
    d = np.arange(0, 1 << 17, dtype=np.int64)
    v = d.astype(np.float32) * (np.float32(1) / (np.float32(9) * np.float32(9)))
    v = np.where(v > np.float32(0.01), v, np.float32(0.01))
    assert (np.diff(v) >= 0).all()
    assert int(np.argmax(v > np.float32(200.0))) == 16201 and not (v[:16201] > np.float32(200.0)).any()
    assert (v > np.float32(0.005)).all(), "a threshold below the floor passes every pixel"


# ---- the programs, the exports, the header ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fbcitb") / "test_fbcitb")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "test_fbcitb.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_sanitized_program(sanitized):
    """tests/cpp/test_fbcitb.cpp under AddressSanitizer and UndefinedBehaviorSanitizer: a program of its own on the CPU"""
    r = subprocess.run([sanitized], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fbcitb: OK" in r.stdout, r.stdout + r.stderr[-3000:]


def test_the_header_loop_equals_the_restatement(sanitized, tmp_path):
    """bilateral.h's plain loop, in the sanitized program, on the pages the GPU tests filter"""
    cases = [(sensitive_page(g, s), 5, 150.0, 150.0) for g, s in SENSITIVE]
    cases += [(fr.tie_page(), 3, fr.TIE_SIGMA_COLOR, fr.TIE_SIGMA_SPACE), (fr.noise(2, 3, 1, 3), 9, 50.0, 3.0), (fr.smooth_noise(21, 70, 31), 31, 40.0, 12.4),
              (fr.noise(37, 53, 1, 12), 5, 1.0, 2.0)]
    for k, (page, d, sc, ss) in enumerate(cases):
        src, dst = str(tmp_path / ("in%d.bin" % k)), str(tmp_path / ("out%d.bin" % k))
        page.tofile(src)
        r = subprocess.run([sanitized, "filter", src, str(page.shape[1]), str(page.shape[0]), str(d), repr(sc), repr(ss), dst],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr[-3000:]
        got = np.fromfile(dst, np.uint8).reshape(page.shape)
        assert np.array_equal(got, fr.bilateral(page, d, sc, ss)), k


def test_exports_and_maps(prl):
    from prlib_amd import _capi

    L = _capi.lib()
    for s in SYMBOLS:
        assert s in _capi.EXPORTED_SYMBOLS and hasattr(L, s), s
    r = subprocess.run(["python", os.path.join(ROOT, "tools", "gen_export_map.py"), "--check"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout
    p = _capi.FbcitbParams()
    L.prl_hip_default_fbcitb_params(p)
    assert (p.use_canny, p.use_variances_map, p.use_clahe, p.use_bilateral, p.use_other_colorspace, p.use_morphology, p.use_canny_on_variances) == (1, 1, 1, 1, 0, 1, 1)
    assert (p.variance_map_threshold, p.clahe_clip_limit, p.gaussian_blur_kernel_size, p.canny_upper_threshold_coeff, p.canny_lower_threshold_coeff,
            p.bounding_rectangle_max_area, p.bilateral_kernel_size, p.bilateral_kernel_intensity_sigma, p.bilateral_kernel_spatial_sigma,
            p.bounding_rect_max_area_coeff) == (200.0, 2.0, 9.0, 0.6, 0.4, 0.3, 5, 150.0, 150.0, 0.3)


def test_whole_call_statuses_before_any_device(prl):
    from prlib_amd import _capi

    L = _capi.lib()
    p = _capi.FbcitbParams()
    L.prl_hip_default_fbcitb_params(p)
    buf = np.zeros(256, np.uint8)
    s, d = buf.ctypes.data, buf.ctypes.data + 128
    call = L.prl_hip_binarize_fbcitb_batch_device
    assert call(p, 1, 1, s, 64, 8, 0, 8, d, 64, 8, None, None) == _capi.PRL_ERR_EMPTY
    assert call(p, 1, 4, s, 64, 8, 2, 2, d, 64, 8, None, None) == _capi.PRL_ERR_BAD_CHANNELS
    assert call(None, 1, 1, s, 64, 8, 8, 8, d, 64, 8, None, None) == _capi.PRL_ERR_BAD_ARG
    for field, value, status in (("variance_map_threshold", float("nan"), _capi.PRL_ERR_BAD_ARG), ("bilateral_kernel_size", 33, _capi.PRL_ERR_BAD_ARG),
                                 ("gaussian_blur_kernel_size", 2.0, _capi.PRL_ERR_BAD_ARG), ("gaussian_blur_kernel_size", 8.0, _capi.PRL_ERR_BAD_ARG),
                                 ("canny_lower_threshold_coeff", 0.7, _capi.PRL_ERR_BAD_ARG), ("gaussian_blur_kernel_size", 257.0, _capi.PRL_ERR_BAD_WINDOW)):
        q = _capi.FbcitbParams()
        L.prl_hip_default_fbcitb_params(q)
        setattr(q, field, value)
        assert call(q, 1, 1, s, 64, 8, 8, 8, d, 64, 8, None, None) == status, field
    q = _capi.FbcitbParams()
    L.prl_hip_default_fbcitb_params(q)
    q.use_canny, q.gaussian_blur_kernel_size = 0, 2.0   # variances only: CannyEdgeDetection is not called, its checks do not apply
    assert call(q, 0, 1, s, 64, 8, 8, 8, d, 64, 8, None, None) == 0
    q.use_variances_map = 0                            # both off switches both on: they apply again
    assert call(q, 0, 1, s, 64, 8, 8, 8, d, 64, 8, None, None) == _capi.PRL_ERR_BAD_ARG
    assert call(p, 1, 1, s, 64, 8, 8, 8, s, 64, 8, None, None) == _capi.PRL_ERR_BAD_ARG, "source and destination share bytes"
    assert call(p, 0, 1, s, 64, 8, 8, 8, d, 64, 8, None, None) == 0
    off = np.array([0, 1], np.int32)
    paint = L.prl_hip_rect_paint_batch_device
    assert paint(1, off.ctypes.data, None, s, 64, 8, 8, 8, d, 64, 8, None) == _capi.PRL_ERR_BAD_ARG, "rectangles to read, none given"
    assert paint(1, np.array([1, 1], np.int32).ctypes.data, s, s, 64, 8, 8, 8, d, 64, 8, None) == _capi.PRL_ERR_BAD_ARG
    assert paint(1, None, s, s, 64, 8, 8, 8, d, 64, 8, None) == _capi.PRL_ERR_BAD_ARG
    assert L.prl_hip_variance_mask_batch_device(1, 2, 200.0, s, 64, 16, 8, 8, d, 64, 8, None) == _capi.PRL_ERR_BAD_CHANNELS


def test_drop_in_header_compiles_against_the_declared_opencv_api():
    """include/prl/binarizeFBCITB.h keeps the reference's signature and defaults; syntax only, against the declaration-only headers"""
    import re

    src = open(os.path.join(ROOT, "include", "prl", "binarizeFBCITB.h")).read()
    assert '#include "prl.h"' in src
    decl = re.sub(r"\s+", " ", open(os.path.join(ROOT, "prlib_amd", "csrc", "prl", "prl.h")).read())
    assert ("binarizeFBCITB(cv::Mat& inputImage, cv::Mat& outputImage, bool useCanny = true, bool useVariancesMap = true, bool useCLAHE = true, "
            "bool useBilateral = true, bool useOtherColorspace = false, bool useMorphology = true, bool useCannyOnVariances = true, "
            "double varianceMapThreshold = 200.0, double CLAHEClipLimit = 2.0, double gaussianBlurKernelSize = 9.0, "
            "double cannyUpperThresholdCoeff = 0.6, double cannyLowerThresholdCoeff = 0.4, double boundingRectangleMaxArea = 0.3, "
            "int bilateralKernelSize = 5, double bilateralKernelIntensitySigma = 150.0, double bilateralKernelSpatialSigma = 150.0, "
            "double boundingRectMaxAreaCoeff = 0.3)") in decl, "the reference's defaults"
    code = '#include "binarizeFBCITB.h"\n#include "imageLibCommon.h"\nvoid f(cv::Mat& a, cv::Mat& b) { prl::binarizeFBCITB(a, b); prl::binarizeFBCITB(a, b, false, true); prl::bilateralFilter(a, b, 5, 150.0, 150.0); }\n'
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-DPRL_REQUIRE_OPENCV", "-I" + os.path.join(ROOT, "tests", "cpp", "opencv_api"),
                        "-I" + os.path.join(ROOT, "include", "prl"), "-x", "c++", "-"], input=code, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-DPRL_REQUIRE_OPENCV", "-I" + os.path.join(ROOT, "tests", "cpp", "opencv_api"),
                        os.path.join(ROOT, "prlib_amd", "csrc", "prl", "prl_host.cpp")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]


def build_dropin(out_dir):
    """g++ of tests/cpp/test_fbcitb_dropin.cpp + prl_host.cpp, with only -I include/prl for the drop-in header."""
    exe = os.path.join(out_dir, "test_fbcitb_dropin")
    flags = []
    for pc in ("opencv4", "opencv"):
        r = subprocess.run(["pkg-config", "--cflags", "--libs", pc], capture_output=True, text=True) if shutil.which("pkg-config") else None
        if r is not None and r.returncode == 0:
            flags = r.stdout.split()
            break
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include", "prl"),
           os.path.join(ROOT, "tests", "cpp", "test_fbcitb_dropin.cpp"), os.path.join(ROOT, "prlib_amd", "csrc", "prl", "prl_host.cpp"),
           ] + flags + ["-L", os.path.join(ROOT, "prlib_amd"), "-lprlib_hip", "-Wl,-rpath," + os.path.join(ROOT, "prlib_amd"),
                        "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_dropin_caller_contract_without_device(prl, tmp_path):
    """the reference's exceptions in its order, and the side effect on a gray Mat, which happens before any later check can fail"""
    src = open(os.path.join(ROOT, "tests", "cpp", "test_fbcitb_dropin.cpp")).read()
    assert '#include "binarizeFBCITB.h"' in src, "the reference's include line"
    exe = build_dropin(str(tmp_path))
    r = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "fbcitb dropin cpu: OK" in r.stdout, r.stdout + r.stderr
