"""cv::HoughLines and prl::findHoughLineContour without a device: the geometry, the argument checks of every new entry in their
order, the host quad search (prlib_amd/csrc/houghline.h through prl_hip_hough_line_quad) against the restatement
(tests/houghline_ref.py) bit for bit on constructed line sets, the plain C++ transform of houghline.h against the restatement, the
colour rule's cases, and the C++ drop-in's contract."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import houghline_cases as hc
import houghline_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF_PI = np.float32(90) * ref.THETA
NEW_EXPORTS = ["prl_hip_hough_lines_geometry", "prl_hip_hough_accumulator_batch_device", "prl_hip_hough_lines_batch_device",
               "prl_hip_hough_lines_host", "prl_hip_hough_edges_batch_device", "prl_hip_hough_edges_host", "prl_hip_hough_line_quad",
               "prl_hip_hough_line_contour_batch_device", "prl_hip_hough_line_contour_host"]


def test_geometry(prl):
    from prlib_amd import _capi

    for w, h in ((1, 1), (7, 1), (64, 48), (2480, 3508), (32768, 32768), (6140, 3)):
        assert prl.hough_lines_geometry(w, h) == ref.geometry(w, h) == (180, 2 * (w + h) + 1)
    assert prl.hough_lines_geometry(2480, 3508)[1] == 11977
    L = _capi.lib()
    a, r = C.c_int(0), C.c_int(0)
    assert L.prl_hip_hough_lines_geometry(0, 4, C.byref(a), C.byref(r)) == _capi.PRL_ERR_EMPTY
    assert L.prl_hip_hough_lines_geometry(4, 4, None, C.byref(r)) == _capi.PRL_ERR_BAD_ARG
    assert L.prl_hip_hough_lines_geometry(32769, 4, C.byref(a), C.byref(r)) == _capi.PRL_ERR_BAD_ARG
    # cvRound(CV_PI / theta) with theta = (float)(CV_PI / 180): 180, not the 181 of floor + 1
    assert round(math.pi / float(ref.THETA)) == 180 and math.floor(math.pi / float(ref.THETA)) + 1 == 181


def test_table_has_no_denormal_products():
    """what include/prl_hip.h says about the denormal mode: one zero entry, the smallest other magnitude is tabCos[90]"""
    c, s = ref.trig_table()
    both = np.concatenate([c, s])
    assert (both == 0).sum() == 1 and s[0] == 0
    nz = np.abs(both[both != 0])
    assert nz.min() == abs(c[90]) and 1.1e-6 < float(nz.min()) < 1.2e-6
    assert float(nz.min()) > 1e30 * float(np.finfo(np.float32).tiny)


def test_argument_checks(prl):
    from prlib_amd import _capi

    L = _capi.lib()
    E, CH, A, OK = _capi.PRL_ERR_EMPTY, _capi.PRL_ERR_BAD_CHANNELS, _capi.PRL_ERR_BAD_ARG, _capi.PRL_OK
    lines, counts, acc = np.zeros(16, np.float32), np.zeros(2, np.int32), np.zeros(182 * 19, np.int32)
    lp, cp, ap = lines.ctypes.data, counts.ctypes.data, acc.ctypes.data
    m = np.zeros((4, 4), np.uint8)
    acc_bytes = 182 * (2 * 8 + 3) * 4
    # the voting stage: n_pages, map, page stride, step, width, height, accumulators, their page stride, stream
    f = L.prl_hip_hough_accumulator_batch_device
    assert f(1, None, 0, 4, 0, 4, None, 0, None) == E                     # EMPTY comes before everything
    assert f(1, None, 0, 4, 4, 4, ap, acc_bytes, None) == A
    assert f(-1, 1, 0, 4, 4, 4, ap, acc_bytes, None) == A
    assert f(1, 1, 0, 3, 4, 4, ap, acc_bytes, None) == A
    assert f(1, 1, 0, 40000, 40000, 4, ap, 1 << 30, None) == A
    assert f(1, 1, 0, 4, 4, 4, None, acc_bytes, None) == A
    assert f(1, 1, 0, 4, 4, 4, ap, acc_bytes - 4, None) == A
    assert f(1, 1, 0, 4, 4, 4, ap, acc_bytes + 2, None) == A
    assert f(0, 1, 0, 4, 4, 4, ap, acc_bytes, None) == OK
    # the lines: ..., threshold, lines, max_lines, n_lines, stream
    f = L.prl_hip_hough_lines_batch_device
    assert f(1, None, 0, 4, 4, 0, -1, None, -1, None, None) == E
    assert f(1, None, 0, 4, 4, 4, 0, lp, 8, cp, None) == A
    assert f(-1, 1, 0, 4, 4, 4, 0, lp, 8, cp, None) == A
    assert f(1, 1, 0, 3, 4, 4, 0, lp, 8, cp, None) == A
    assert f(1, 1, 0, 32769, 32769, 4, 0, lp, 8, cp, None) == A
    assert f(1, 1, 0, 4, 4, 4, -1, lp, 8, cp, None) == A
    assert f(1, 1, 0, 4, 4, 4, 0, None, 8, cp, None) == A
    assert f(1, 1, 0, 4, 4, 4, 0, lp, -1, cp, None) == A
    assert f(1, 1, 0, 4, 4, 4, 0, lp, 8, None, None) == A
    assert f(0, 1, 0, 4, 4, 4, 0, None, 0, cp, None) == OK
    f = L.prl_hip_hough_lines_host
    assert f(m.ctypes.data, 4, 4, 0, 0, lp, 8, cp) == E
    assert f(None, 4, 4, 4, 0, lp, 8, cp) == A
    assert f(m.ctypes.data, 3, 4, 4, 0, lp, 8, cp) == A
    assert f(m.ctypes.data, 4, 4, 4, -5, lp, 8, cp) == A
    assert f(m.ctypes.data, 4, 4, 4, 0, lp, 8, None) == A
    # the edge map: n_pages, channels, source, strides, width, height, destination, strides, stream
    f = L.prl_hip_hough_edges_batch_device
    assert f(1, 2, None, 0, 12, 0, 4, None, 0, 4, None) == E
    assert f(1, 2, 1, 0, 12, 4, 4, 4096, 0, 4, None) == CH                # BAD_CHANNELS comes before BAD_ARG
    assert f(1, 2, None, 0, 12, 4, 4, None, 0, 4, None) == CH
    assert f(1, 3, None, 0, 12, 4, 4, 4096, 0, 4, None) == A
    assert f(1, 3, 1, 0, 12, 4, 4, None, 0, 4, None) == A
    assert f(-1, 3, 1, 0, 12, 4, 4, 4096, 0, 4, None) == A
    assert f(1, 3, 1, 0, 11, 4, 4, 4096, 0, 4, None) == A
    assert f(1, 4, 1, 0, 16, 4, 4, 4096, 0, 3, None) == A
    assert f(1, 1, 1, 0, 40000, 40000, 4, 1 << 40, 0, 40000, None) == A
    assert f(2, 1, 4096, 16, 4, 4, 4, 4096 + 8, 16, 4, None) == A         # source and destination share bytes
    assert f(0, 3, 1, 0, 12, 4, 4, 4096, 0, 4, None) == OK
    f = L.prl_hip_hough_edges_host
    img, dst = np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4), np.uint8)
    assert f(3, img.ctypes.data, 12, 4, 0, dst.ctypes.data, 4) == E
    assert f(5, img.ctypes.data, 12, 4, 4, dst.ctypes.data, 4) == CH
    assert f(3, None, 12, 4, 4, dst.ctypes.data, 4) == A
    assert f(3, img.ctypes.data, 12, 4, 4, dst.ctypes.data, 3) == A
    # the quad search: host code
    f = L.prl_hip_hough_line_quad
    q, found = np.zeros(8, np.int32), C.c_int(0)
    assert f(lp, 4, 0, 4, q.ctypes.data, C.byref(found)) == E
    assert f(None, 4, 4, 4, q.ctypes.data, C.byref(found)) == A
    assert f(lp, -1, 4, 4, q.ctypes.data, C.byref(found)) == A
    assert f(lp, 4, 4, 4, None, C.byref(found)) == A
    assert f(lp, 4, 4, 4, q.ctypes.data, None) == A
    assert f(lp, 4, 40000, 4, q.ctypes.data, C.byref(found)) == A
    assert f(None, 0, 4, 4, q.ctypes.data, C.byref(found)) == OK and found.value == 0
    # the whole function: ..., quads, found, out_lines, stream
    f = L.prl_hip_hough_line_contour_batch_device
    qi, fi = np.zeros(8, np.int32), np.zeros(1, np.int32)
    assert f(1, 2, None, 0, 12, 0, 4, None, None, None, None) == E
    assert f(1, 2, 1, 0, 12, 4, 4, qi.ctypes.data, fi.ctypes.data, None, None) == CH
    assert f(1, 3, None, 0, 12, 4, 4, qi.ctypes.data, fi.ctypes.data, None, None) == A
    assert f(-1, 3, 1, 0, 12, 4, 4, qi.ctypes.data, fi.ctypes.data, None, None) == A
    assert f(1, 3, 1, 0, 11, 4, 4, qi.ctypes.data, fi.ctypes.data, None, None) == A
    assert f(1, 1, 1, 0, 40000, 40000, 4, qi.ctypes.data, fi.ctypes.data, None, None) == A
    assert f(1, 3, 1, 0, 12, 4, 4, None, fi.ctypes.data, None, None) == A
    assert f(1, 3, 1, 0, 12, 4, 4, qi.ctypes.data, None, None, None) == A
    assert f(0, 3, 1, 0, 12, 4, 4, qi.ctypes.data, fi.ctypes.data, None, None) == OK
    f = L.prl_hip_hough_line_contour_host
    assert f(3, img.ctypes.data, 12, 0, 4, qi.ctypes.data, fi.ctypes.data, None) == E
    assert f(2, img.ctypes.data, 12, 4, 4, qi.ctypes.data, fi.ctypes.data, None) == CH
    assert f(3, None, 12, 4, 4, qi.ctypes.data, fi.ctypes.data, None) == A
    assert f(3, img.ctypes.data, 11, 4, 4, qi.ctypes.data, fi.ctypes.data, None) == A
    assert f(3, img.ctypes.data, 12, 4, 4, None, fi.ctypes.data, None) == A


def _line(rho, deg):
    return (np.float32(rho), np.float32(deg) * ref.THETA)


def line_sets():
    """name -> (lines K x 2, width, height, is a quad expected)"""
    rect = [_line(10, 0), _line(20, 90), _line(100, 0), _line(80, 90)]
    sets = {"rectangle": (rect, 120, 100, True), "three": (rect[:3], 120, 100, False),
            "parallel": ([_line(10, 0), _line(30, 0), _line(50, 0), _line(70, 0)], 120, 100, False),
            "two_pairs_parallel_in_a_row": ([_line(10, 0), _line(100, 0), _line(20, 90), _line(80, 90), _line(50, 0)], 120, 100, True),
            "corner_on_the_width": (rect, 100, 100, True), "corner_beyond_the_width": (rect, 99, 100, False),
            "corner_on_the_height": (rect, 120, 80, True), "corner_beyond_the_height": (rect, 120, 79, False)}
    # 25 lines, near-doubles of a leaning quadrilateral's sides: the first round (5 pixels) leaves 21, the second fewer
    many = []
    for rho, deg in ((40, 3), (300, 2), (60, 92), (260, 91)):
        many += [_line(rho + d, deg) for d in (0, 3, 14, 21, 28, 35)]
    many.append(_line(170, 45))
    sets["two_rounds"] = (many, 400, 340, True)
    # 24 lines in three tight bundles: the first round keeps three, the filter gives up and keeps the first 20 of its input.
    # Those are all parallel in the first set; in the second they hold both directions, and a sliver of a quad is found
    bundle = lambda rho, deg, n: [_line(rho + 0.5 * i, deg) for i in range(n)]
    sets["resize_exit"] = (bundle(50, 0, 10) + bundle(200, 0, 10) + bundle(90, 90, 4), 300, 300, False)
    sets["resize_exit_quad"] = (bundle(50, 0, 8) + bundle(200, 0, 8) + bundle(90, 90, 8), 300, 300, True)
    # quads of equal area: a square's eight enumerations (four starting lines, two directions) have exactly the same area, and the
    # first in the loops' order, (0, 1, 2, 3), stays: its corners are lines 1 x 0, 2 x 1, 3 x 2, 0 x 3
    sets["equal_areas"] = ([_line(10, 0), _line(10, 90), _line(70, 0), _line(70, 90)], 200, 200, True)
    return sets


def test_quad_search_against_the_restatement(prl):
    found, missed = 0, 0
    for name, (lines, w, h, expect) in line_sets().items():
        ln = np.array(lines, np.float32).reshape(-1, 2)
        want = ref.hough_line_quad(ln, w, h)
        got = prl.hough_line_quad(ln, w, h)
        assert (want is not None) == expect, (name, want)
        assert (got is None) == (want is None), (name, got, want)
        if want is not None:
            assert got.dtype == np.int32 and np.array_equal(got, want), (name, got.tolist(), want.tolist())
            found += 1
        else:
            missed += 1
    assert found >= 4 and missed >= 4   # the restatement alone puts cases in both classes


def test_filter_rounds_and_the_resize_exit():
    """the constructed sets take the paths they are named after, in the restatement"""
    sets = line_sets()
    many = np.array(sets["two_rounds"][0], np.float32)
    seg = ref.from_vec2f(many)
    assert len(many) == 25 and seg.dtype == np.float32 and np.array_equal(seg, np.rint(seg))
    assert len(ref.delete_similar_lines(many, max_lines=24)) == 21              # what the first round leaves: one round is not enough
    assert 4 <= len(ref.delete_similar_lines(many)) <= 20
    for name in ("resize_exit", "resize_exit_quad"):
        few = np.array(sets[name][0], np.float32)
        kept = ref.delete_similar_lines(few)
        assert len(few) == 24 and len(kept) == 20 and np.array_equal(kept, few[:20])   # the exit: the input's first 20, not the three survivors
    eq = np.array(sets["equal_areas"][0], np.float32)
    q = ref.hough_line_quad(eq, 200, 200)
    assert q.tolist() == [[10, 10], [70, 10], [70, 70], [10, 70]]


def test_colour_rule_cases_are_exercised():
    """the edge-map pages of the GPU test: on the blurred colour pages every channel gives some pixel its gradient, and somewhere
    two channels tie on a magnitude that is not zero"""
    for w, h in ((65, 63), (300, 200)):
        for kind in ("random", "stroke"):
            for ch in (3, 4):
                img = ref.blurred(hc.edge_page(w, h, kind, ch, seed=5))
                _dx, _dy, mp, best, tied = ref.colour_gradients(img)
                assert set(np.unique(best)) == set(range(ch)), (w, h, kind, ch, np.unique(best))
                assert (tied & (mp[1:-1, 1:-1] > 0)).any(), (w, h, kind, ch)


def _build_program(tmp_path):
    exe = str(tmp_path / "test_houghline")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "test_houghline.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_plain_cpp_transform_and_search(tmp_path):
    """tests/cpp/test_houghline.cpp (houghline.h alone, under AddressSanitizer and UndefinedBehaviorSanitizer, a program of its own
    on the CPU): its hand-made facts, then the plain C++ transform and the search against the restatement"""
    exe = _build_program(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "houghline: OK" in r.stdout, r.stdout + r.stderr[-3000:]
    maps = dict(hc.designed_maps())
    maps["sparse"] = hc.sparse_map(65, 63, 3)
    maps["corners"] = hc.corner_map(31, 17)
    for name, m in maps.items():
        for thr in (0, 1, 50):
            path = tmp_path / "map.raw"
            path.write_bytes(np.ascontiguousarray(m).tobytes())
            r = subprocess.run([exe, "lines", str(m.shape[1]), str(m.shape[0]), str(thr), str(path)], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stdout + r.stderr[-3000:]
            acc = ref.accumulator(m)
            hash_ = 2166136261
            for b in acc.astype("<i4").tobytes():
                hash_ = ((hash_ ^ b) * 16777619) & 0xFFFFFFFF
            head = r.stdout.splitlines()[0].split()
            assert head == ["cells", str(acc.size), "sum", str(int(acc.sum())), "hash", str(hash_)], (name, head)
            got = np.array([[int(v) for v in ln.split()[1:]] for ln in r.stdout.splitlines()[1:]], np.uint32).reshape(-1, 2)
            want = ref.hough_lines(m, thr).view(np.uint32).reshape(-1, 2)
            assert np.array_equal(got, want), (name, thr, len(got), len(want))
    for name, (lines, w, h, _expect) in line_sets().items():
        ln = np.array(lines, np.float32).reshape(-1, 2)
        path = tmp_path / "lines.raw"
        path.write_bytes(ln.tobytes())
        r = subprocess.run([exe, "quad", str(w), str(h), str(len(ln)), str(path)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr[-3000:]
        want = ref.hough_line_quad(ln, w, h)
        out = r.stdout.splitlines()
        assert out[0] == f"found {0 if want is None else 1}", (name, out)
        if want is not None:
            assert [int(v) for v in out[1].split()[1:]] == want.reshape(8).tolist(), name


def test_photographs_fall_in_both_classes_with_few_lines():
    """the pages of the GPU contour test: both classes, and line counts that keep the Python filter quick"""
    found = 0
    for w, h in ((511, 300),):
        for kind in ("found", "broken", "flat", "stripes"):
            quad, n_lines = ref.hough_line_contour(hc.photo(w, h, kind, 1))
            print(w, h, kind, "lines", n_lines, "quad", None if quad is None else quad.tolist())
            assert n_lines < 500
            assert (quad is not None) == (kind in ("found", "broken")), (kind, quad)
            found += quad is not None
            if kind == "stripes":
                assert n_lines >= 4   # not the early return: the search itself finds nothing
    assert found == 2


def build_dropin(out_dir):
    """g++ of tests/cpp/test_houghline_dropin.cpp + prl_host.cpp, with only -I include/prl for the drop-in header."""
    exe = os.path.join(out_dir, "test_houghline_dropin")
    flags = []
    for pc in ("opencv4", "opencv"):
        r = subprocess.run(["pkg-config", "--cflags", "--libs", pc], capture_output=True, text=True) if shutil.which("pkg-config") else None
        if r is not None and r.returncode == 0:
            flags = r.stdout.split()
            break
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include", "prl"),
           os.path.join(ROOT, "tests", "cpp", "test_houghline_dropin.cpp"), os.path.join(ROOT, "prlib_amd", "csrc", "prl", "prl_host.cpp"),
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
    assert r.returncode == 0 and "houghline dropin cpu: OK" in r.stdout, r.stdout + r.stderr


def test_cpp_declaration_against_opencv_headers():
    """prl::findHoughLineContour carries the reference's signature: the drop-in program compiles against OpenCV's declared API"""
    cpp = os.path.join(ROOT, "tests", "cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-DPRL_REQUIRE_OPENCV",
                        "-I" + os.path.join(cpp, "opencv_api"), "-I" + os.path.join(ROOT, "include", "prl"),
                        os.path.join(cpp, "test_houghline_dropin.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-DPRL_REQUIRE_OPENCV",
                        "-I" + os.path.join(cpp, "opencv_api"), os.path.join(ROOT, "prlib_amd", "csrc", "prl", "prl_host.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


def test_exports_maps_python_and_documents(prl):
    from prlib_amd import _capi

    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "prlib_amd", "libprlib_hip.so")], capture_output=True, text=True,
                         check=True).stdout
    header = open(os.path.join(ROOT, "include", "prl_hip.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_EXPORTS:
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(_capi.lib(), name)
        assert re.search(r"\bT " + name + r"\b", out), name
        assert re.search(r"^int " + name + r"\(", header, flags=re.M), name
        assert name in integration, name
        for m in ("prl_hip.map", "prl_hip_testhooks.map"):
            assert re.search(r"^\s+" + name + ";$", open(os.path.join(ROOT, "prlib_amd", "csrc", m)).read(), flags=re.M), (name, m)
    assert _capi.lib().prl_hip_abi_version() == 4
    for fn in ("hough_lines_geometry", "hough_accumulator", "hough_lines", "hough_edges", "hough_line_quad", "hough_line_contour"):
        assert callable(getattr(prl, fn)) and fn in prl.__all__
    assert "hough.hip" in open(os.path.join(ROOT, "prlib_amd", "csrc", "Makefile")).read()
    assert "hough" in re.search(r"set\(PRL_KERNELS ([^)]*)\)", open(os.path.join(ROOT, "CMakeLists.txt")).read()).group(1).split()
    section = re.search(r"---- Hough lines.*", header, flags=re.S).group(0)
    assert "[upstream]" in section and "181" in section and "not pinned" in section and "imwrite" in section
