"""The quad search of prl::documentContour without a device: the library's host entries (prl_hip_find_contours,
prl_hip_approx_poly_closed, prl_hip_document_quad, prl_hip_document_quad_finish) against the restatement of tests/contour_ref.py on
hand-made maps and a seeded fuzz, properties that do not come from the same reading of OpenCV, the ordering of the corners, the
stand-alone C++ program under the sanitizers, the exports and the C++ declarations."""
import os
import re
import subprocess

import numpy as np
import pytest

import contour_cases as cc
import contour_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["prl_hip_morphology_ex_batch_device", "prl_hip_morphology_ex_host", "prl_hip_find_contours", "prl_hip_approx_poly_closed",
               "prl_hip_document_quad", "prl_hip_document_quad_finish", "prl_hip_document_contour_batch_device",
               "prl_hip_document_contour_host"]
HAND = cc.hand_made()
N_FUZZ = 300


def _tuples(a):
    return [tuple(int(v) for v in p) for p in np.asarray(a).reshape(-1, 2)]


def _compare(prl, name, page):
    """contour lists, every approximation, the chosen quad; returns the restatement's quad"""
    want = cr.find_contours(page)
    got = prl.find_contours(page)
    assert len(got) == len(want), (name, len(got), len(want))
    for k, ((wp, wh), (gp, gh)) in enumerate(zip(want, got)):
        assert gh == wh and _tuples(gp) == wp, (name, k, wp, _tuples(gp))
        _poly, steps = cr.reduce_polygon(wp)
        cur, eps = np.array(wp, np.int32), 1.0
        for s in steps:
            cur = prl.approx_poly_closed(cur, eps)
            assert _tuples(cur) == s, (name, k, eps)
            eps += 1.0
    wq, gq = cr.document_quad(page), prl.document_quad(page)
    assert (gq is None) == (wq is None), (name, wq, gq)
    if wq is not None:
        assert _tuples(gq) == wq, (name, wq, gq)
    return wq


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_made_maps(prl, name):
    page, expect = HAND[name]
    quad = _compare(prl, name, page)
    print(name, page.shape, quad)
    if expect is not None:
        assert (quad is not None) == expect


def test_hand_made_maps_fail_for_the_reason_they_name():
    poly, _ = cr.reduce_polygon(cr.find_contours(HAND["trapezoid_sides"][0])[0][0])
    assert len(poly) == 4
    s = [cr._norm(poly[i], poly[(i + 1) % 4]) for i in range(4)]
    assert min(s[0], s[2]) / max(s[0], s[2]) < 0.85 or min(s[1], s[3]) / max(s[1], s[3]) < 0.85
    poly, _ = cr.reduce_polygon(cr.find_contours(HAND["angle_below_160"][0])[0][0])
    assert len(poly) == 4
    s = [cr._norm(poly[i], poly[(i + 1) % 4]) for i in range(4)]
    assert min(s[0], s[2]) / max(s[0], s[2]) >= 0.85 and min(s[1], s[3]) / max(s[1], s[3]) >= 0.85
    assert min(cr._angle(poly[0], poly[1], poly[2], poly[3]), cr._angle(poly[1], poly[2], poly[3], poly[0])) < 160.0
    assert cr.document_quad(HAND["angle_below_160"][0]) is None
    poly, _ = cr.reduce_polygon(cr.find_contours(HAND["below_five_percent"][0])[0][0])
    assert len(poly) == 4 and cr.contour_area(poly) < 0.05 * 64 * 64
    # the rectangle's outer and hole border both qualify; the hole border cuts the corners (316 against 352), so the outer one wins
    both = cr.find_contours(HAND["one_pixel_outline"][0])
    assert [h for _p, h in both] == [False, True]
    polys = [cr.reduce_polygon(p)[0] for p, _h in both]
    assert [len(p) for p in polys] == [4, 4] and [cr.contour_area(p) for p in polys] == [352.0, 316.0]
    assert cr.document_quad(HAND["one_pixel_outline"][0]) == polys[0]
    # the diamond's two borders run over the same pixels: a tie in area, resolved by the order through the strict `>`
    both = cr.find_contours(HAND["diamond_outline_tie"][0])
    assert [h for _p, h in both] == [False, True]
    polys = [cr.reduce_polygon(p)[0] for p, _h in both]
    assert cr.contour_area(polys[0]) == cr.contour_area(polys[1]) and polys[0] != polys[1]
    assert cr.document_quad(HAND["diamond_outline_tie"][0]) == polys[0]


def test_fuzz_against_the_restatement(prl):
    pages = [cc.fuzz_map(s) for s in range(N_FUZZ)]
    alone = [cr.document_quad(p) is not None for p in pages]
    assert sum(alone) >= N_FUZZ // 5 and N_FUZZ - sum(alone) >= N_FUZZ // 5, sum(alone)
    for s, page in enumerate(pages):
        assert page.shape[0] <= 64 and page.shape[1] <= 64
        assert (_compare(prl, s, page) is not None) == alone[s]


def _subsequence_cyclic(small, big):
    if not small:
        return True
    n = len(big)
    for start in range(n):
        if big[start] != small[0]:
            continue
        at, ok = start, True
        used = 1
        for p in small[1:]:
            while used < n and big[(at + 1) % n] != p:
                at += 1
                used += 1
            if used >= n:
                ok = False
                break
            at += 1
            used += 1
        if ok:
            return True
    return False


def test_properties_independent_of_the_restatement(prl):
    from scipy import ndimage

    for s in list(range(0, N_FUZZ, 2)) + sorted(HAND):
        page = HAND[s][0] if isinstance(s, str) else cc.fuzz_map(s)
        fg = page != 0
        borders = prl.find_contours(page)
        _lab, n_comp = ndimage.label(fg, structure=np.ones((3, 3), int))
        assert sum(1 for _p, hole in borders if not hole) == n_comp, s
        framed = np.pad(~fg, 1, constant_values=True)
        lab4, n_bg = ndimage.label(framed)   # 4-connected background
        assert sum(1 for _p, hole in borders if hole) == n_bg - 1, s   # all regions but the one that holds the frame
        nb4 = np.pad(fg, 1, constant_values=False)
        for pts, _hole in borders:
            for x, y in _tuples(pts):
                assert fg[y, x] and not nb4[y:y + 3, x:x + 3].all(), (s, x, y)
            cur, eps = _tuples(pts), 1.0
            while len(cur) > 4:
                nxt = _tuples(prl.approx_poly_closed(np.array(cur, np.int32), eps))
                assert _subsequence_cyclic(nxt, cur), (s, eps, cur, nxt)
                cur, eps = nxt, eps + 1.0


def test_finish_is_one_answer_for_every_start_and_orientation(prl):
    quad = [(12, 9), (200, 14), (190, 160), (8, 150)]   # top left, top right, bottom right, bottom left
    want = cr.quad_finish(quad, 256, 192, 2051, 1537)
    assert np.array_equal(want.reshape(4, 2)[0], np.float32([12, 9]) * np.float32([np.float32(2051) / np.float32(256), np.float32(1537) / np.float32(192)]))
    for start in range(4):
        for order in (1, -1):
            q = [quad[(start + order * i) % 4] for i in range(4)]
            got = prl.document_quad_finish(q, (256, 192), (2051, 1537))
            assert np.array_equal(got.reshape(8), want), (start, order)
            assert np.array_equal(cr.quad_finish(q, 256, 192, 2051, 1537), want)
    bowtie = [quad[0], quad[2], quad[1], quad[3]]
    assert np.array_equal(prl.document_quad_finish(bowtie, (256, 192), (2051, 1537)).reshape(8), want)
    # a distance tie: (3, 4) and (4, 3) are equally near; the first of the cycle from the smallest x, then y, stays
    tie = [(3, 4), (4, 3), (40, 30), (30, 40)]
    got = prl.document_quad_finish(tie, (64, 64), (64, 64))
    assert np.array_equal(got.reshape(8), cr.quad_finish(tie, 64, 64, 64, 64)) and tuple(got[0]) == (3.0, 4.0) and tuple(got[1]) == (4.0, 3.0)
    for bad in ([(0, 0), (5, 5), (10, 10), (0, 10)], [(0, 0), (10, 0), (3, 2), (0, 10)]):
        assert cr.quad_finish(bad, 10, 10, 20, 20) is None
        with pytest.raises(prl._capi.PrlError) as e:
            prl.document_quad_finish(bad, (10, 10), (20, 20))
        assert e.value.status == prl._capi.PRL_ERR_BAD_ARG


def test_scale_is_from_the_integer_division_not_from_the_pyramid(prl):
    import edges_ref as er

    levels, mw, mh = er.document_edges_geometry(1027, 771)
    assert (levels, mw, mh) == (2, 257, 193) and (1027 >> levels, 771 >> levels) == (256, 192)
    assert prl.document_edges_geometry(1027, 771) == (levels, mw, mh)
    page = cc.outline(mw, mh, [(20, 15), (236, 15), (236, 177), (20, 177)])
    quad = cr.document_quad(page)
    assert quad is not None
    want, tries = cr.contour_from_map(page, 1027, 771)
    got = prl.document_quad_finish(quad, (256, 192), (1027, 771))
    assert tries == 0 and np.array_equal(got.reshape(8), want)
    assert not np.array_equal(got, prl.document_quad_finish(quad, (mw, mh), (1027, 771)))


def test_argument_checks(prl):
    from prlib_amd import _capi

    L = prl._capi.lib()
    m = np.zeros((4, 4), np.uint8)
    q, f = np.zeros(8, np.int32), np.zeros(1, np.int32)
    import ctypes as C

    assert L.prl_hip_document_quad(m.ctypes.data, 4, 0, 4, q.ctypes.data, C.cast(f.ctypes.data, C.POINTER(C.c_int))) == _capi.PRL_ERR_EMPTY
    assert L.prl_hip_document_quad(None, 4, 4, 4, q.ctypes.data, C.cast(f.ctypes.data, C.POINTER(C.c_int))) == _capi.PRL_ERR_BAD_ARG
    assert L.prl_hip_document_quad(m.ctypes.data, 3, 4, 4, q.ctypes.data, C.cast(f.ctypes.data, C.POINTER(C.c_int))) == _capi.PRL_ERR_BAD_ARG
    out = np.zeros(8, np.float32)
    assert L.prl_hip_document_quad_finish(q.ctypes.data, 0, 4, 4, 4, out.ctypes.data) == _capi.PRL_ERR_EMPTY
    assert L.prl_hip_document_quad_finish(None, 4, 4, 4, 4, out.ctypes.data) == _capi.PRL_ERR_BAD_ARG
    # the device entries refuse before any device is touched, in the edge entries' order
    fq, fi = np.zeros(8, np.float32), np.zeros(1, np.int32)
    call = L.prl_hip_document_contour_batch_device
    assert call(1, 3, 1, 0, 12, 0, 4, fq.ctypes.data, fi.ctypes.data, None, None) == _capi.PRL_ERR_EMPTY
    assert call(1, 2, 1, 0, 12, 4, 4, fq.ctypes.data, fi.ctypes.data, None, None) == _capi.PRL_ERR_BAD_CHANNELS
    assert call(1, 3, None, 0, 12, 4, 4, fq.ctypes.data, fi.ctypes.data, None, None) == _capi.PRL_ERR_BAD_ARG
    assert call(-1, 3, 1, 0, 12, 4, 4, fq.ctypes.data, fi.ctypes.data, None, None) == _capi.PRL_ERR_BAD_ARG
    assert call(1, 3, 1, 0, 11, 4, 4, fq.ctypes.data, fi.ctypes.data, None, None) == _capi.PRL_ERR_BAD_ARG
    assert call(1, 3, 1, 0, 12, 4, 4, None, fi.ctypes.data, None, None) == _capi.PRL_ERR_BAD_ARG
    assert call(1, 1, 1, 0, 40000, 40000, 4, fq.ctypes.data, fi.ctypes.data, None, None) == _capi.PRL_ERR_BAD_ARG
    assert call(0, 3, 1, 0, 12, 4, 4, fq.ctypes.data, fi.ctypes.data, None, None) == _capi.PRL_OK
    # morphology_ex: anchor, iterations and the grown rectangle are checked with the element
    mx = L.prl_hip_morphology_ex_batch_device
    ok = (1, 1, 1, 0, 3, 3)                  # n_pages, channels, DILATE, RECT, 3 x 3
    tail = (1, 0, 8, 8, 8, 2, 0, 8, None)    # source, its strides, 8 x 8, destination, its strides, stream
    assert mx(*ok, -1, -1, 1, 1, 0, 8, 0, 8, 2, 0, 8, None) == _capi.PRL_ERR_EMPTY
    for anchor_x, anchor_y, iters in ((3, 0, 1), (-2, 0, 1), (0, 3, 1), (0, 0, 0), (0, 0, 17)):
        assert mx(*ok, anchor_x, anchor_y, iters, *tail) == _capi.PRL_ERR_BAD_ARG, (anchor_x, anchor_y, iters)
    assert mx(1, 1, 1, 0, 128, 1, -1, -1, 3, *tail) == _capi.PRL_ERR_BAD_ARG     # 1 + 3 * 127 > 255
    assert mx(1, 5, 1, 0, 3, 3, -1, -1, 1, *tail) == _capi.PRL_ERR_BAD_CHANNELS
    assert mx(0, 1, 1, 0, 128, 1, -1, -1, 2, *tail) == _capi.PRL_OK               # 255: allowed, and no page to run


def test_sanitized_program(tmp_path):
    """tests/cpp/test_contour.cpp under AddressSanitizer and UndefinedBehaviorSanitizer: a program of its own on the CPU"""
    exe = str(tmp_path / "test_contour")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "test_contour.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "contour: OK" in r.stdout, r.stdout + r.stderr[-3000:]


def test_exports_maps_and_python(prl):
    from prlib_amd import _capi

    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "prlib_amd", "libprlib_hip.so")], capture_output=True, text=True,
                         check=True).stdout
    header = open(os.path.join(ROOT, "include", "prl_hip.h")).read()
    for name in NEW_EXPORTS:
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(_capi.lib(), name)
        assert re.search(r"\bT " + name + r"\b", out), name
        assert re.search(r"^int " + name + r"\(", header, flags=re.M), name
        for m in ("prl_hip.map", "prl_hip_testhooks.map"):
            assert re.search(r"^\s+" + name + ";$", open(os.path.join(ROOT, "prlib_amd", "csrc", m)).read(), flags=re.M), (name, m)
    assert _capi.lib().prl_hip_abi_version() == 4
    assert subprocess.run(["python3", os.path.join(ROOT, "tools", "gen_export_map.py"), "--check"]).returncode == 0
    for fn in ("morphology_ex", "find_contours", "approx_poly_closed", "document_quad", "document_quad_finish", "document_contour",
               "auto_crop"):
        assert callable(getattr(prl, fn)) and fn in prl.__all__
    assert "not provided" not in re.search(r"The edge map of prl::documentContour.*?prl::resize \(resize", header, flags=re.S).group(0)


def test_cpp_declarations_against_opencv_headers():
    """prl::documentContour and prl::autoCrop carry the reference's signatures: compiled against OpenCV's declared API"""
    cpp = os.path.join(ROOT, "tests", "cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-DPRL_REQUIRE_OPENCV",
                        "-I" + os.path.join(cpp, "opencv_api"), "-I" + os.path.join(ROOT, "include", "prl"),
                        os.path.join(cpp, "autocrop_api.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-DPRL_REQUIRE_OPENCV",
                        "-I" + os.path.join(cpp, "opencv_api"), os.path.join(ROOT, "prlib_amd", "csrc", "prl", "prl_host.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
