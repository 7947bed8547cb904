"""Rule R without a device: the equivalence the device labeller rests on.  The library's host scan prl_hip_external_rects (the
literal raster scan of cv::findContours(RETR_EXTERNAL), contour.h) must equal the topological restatement tests/components_ref.py
as an ordered list, with `found`, on every 4 x 4 map, every 1 x 12 and 12 x 1 map, 20 000 seeded random maps raw and dilated one to
three times, rings with components in their holes and nested rings; components.h (the plain loops beside the kernels) equals the
restatement on the same maps, in a stand-alone program under the address and undefined-behaviour sanitizers.  Then the statuses of
the two device entries before any device is touched, the exports and the Python mirror.  Every comparison is an equality."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import components_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["prl_hip_connected_components_batch_device", "prl_hip_external_rects_batch_device"]
N_RANDOM = 20000


def host_rects(L, m, buf):
    """prl_hip_external_rects on one map: ([(x, y, w, h), ...], found)"""
    h, w = m.shape
    found, kept = ctypes.c_int(0), ctypes.c_int(0)
    st = L.prl_hip_external_rects(m.ctypes.data, m.strides[0], w, h, buf.ctypes.data, len(buf) // 4, ctypes.byref(found), ctypes.byref(kept))
    assert st == 0 and kept.value <= len(buf) // 4
    return [tuple(r) for r in buf[:4 * kept.value].reshape(-1, 4).tolist()], found.value


def show(m):
    return "\n".join("".join("#" if v else "." for v in row) for row in np.asarray(m))


def compare_batch(L, maps, name, buf):
    """the host scan against the restatement on N x H x W maps; returns the restatement's answers"""
    maps = np.ascontiguousarray(maps)
    want = cr.external_rects_batch(maps)
    for m, (rects, found) in zip(maps, want):
        got = host_rects(L, m, buf)
        if got != (rects, found):
            raise AssertionError(f"{name}: the scan gives {got}, rule R {(rects, found)} on\n{show(m)}")
    return want


@pytest.fixture(scope="module")
def scan(prl):
    from prlib_amd import _capi

    return _capi.lib(), np.zeros(4 * 24 * 24, np.int32)


@pytest.fixture(scope="module")
def cases():
    """(name, maps N x H x W) of every family, made once"""
    out = [("4 x 4", cr.all_maps(4, 4)), ("1 x 12", cr.all_maps(1, 12)), ("12 x 1", cr.all_maps(12, 1))]
    for (h, w), maps in sorted(cr.random_maps(2024, N_RANDOM).items()):
        out.append((f"random {h} x {w}", maps))
        d = maps
        for t in (1, 2, 3):
            d = np.stack([cr.dilate(m, 1) for m in d])
            out.append((f"random {h} x {w} dilated {t}", d))
    return out


def ring_maps():
    blob, line, dot = np.full((3, 3), 255, np.uint8), np.full((1, 3), 255, np.uint8), np.full((1, 1), 255, np.uint8)
    lshape = np.array([[255, 0], [255, 255]], np.uint8)
    out = {}
    for wall in (1, 2, 3, 7):
        for name, inner in (("empty", None), ("blob", blob), ("line", line), ("dot", dot), ("L", lshape)):
            size = 2 * wall + 9
            out[f"ring wall {wall} {name}"] = cr.framed(cr.ring(size, wall, inner), 2)
            out[f"ring wall {wall} {name} on the border"] = cr.ring(size, wall, inner)
        for depth in (1, 2, 3):
            out[f"nested {depth} wall {wall}"] = cr.framed(cr.nested_rings(depth, wall))
            out[f"nested {depth} wall {wall} on the border"] = cr.nested_rings(depth, wall)
            out[f"nested {depth} wall {wall} gap 1"] = cr.framed(cr.nested_rings(depth, wall, gap=1))
    cut = cr.framed(cr.ring(9, 1, np.full((1, 1), 255, np.uint8)), 1)
    cut[1, 1] = 0   # a cut corner: the hole touches the outside diagonally only, and stays a hole
    out["cut corner"] = cut
    return out


def test_the_restatement_on_hand_made_maps():
    assert cr.external_rects(np.zeros((3, 5), np.uint8)) == ([], 0)
    assert cr.external_rects(np.full((3, 5), 255, np.uint8)) == ([(0, 0, 5, 3)], 1)
    assert cr.external_rects(np.full((1, 1), 255, np.uint8)) == ([], 1), "a single pixel is found and not kept"
    diag = np.eye(4, dtype=np.uint8) * 255
    assert cr.external_rects(diag) == ([], 1) and cr.external_rects(diag[::-1]) == ([], 1), "a diagonal is a straight line"
    assert cr.external_rects(np.array([[255, 0], [255, 255]], np.uint8)) == ([(0, 0, 2, 2)], 1), "an L of 3 pixels is kept"
    m = cr.framed(cr.nested_rings(3, 1))
    rects, found = cr.external_rects(m)
    assert found == 1 and rects == [(1, 1, m.shape[1] - 2, m.shape[0] - 2)], "only the outermost ring is reported"
    cut = ring_maps()["cut corner"]
    assert cr.external_rects(cut) == ([(1, 1, 9, 9)], 1), "4-connected background: the blob in the pocket is not external"
    labels, stats = cr.components(np.array([[255, 0, 255], [0, 255, 0]], np.uint8), 8)
    assert labels.tolist() == [[1, 0, 1], [0, 1, 0]] and stats.tolist() == [[0, 0, 3, 2, 3]]
    labels, stats = cr.components(np.array([[255, 0, 255], [0, 255, 0]], np.uint8), 4)
    assert labels.tolist() == [[1, 0, 2], [0, 3, 0]] and stats.tolist() == [[0, 0, 1, 1, 1], [2, 0, 1, 1, 1], [1, 1, 1, 1, 1]]


def test_the_scan_equals_rule_r_on_every_small_map(scan):
    L, buf = scan
    for name, maps in (("4 x 4", cr.all_maps(4, 4)), ("1 x 12", cr.all_maps(1, 12)), ("12 x 1", cr.all_maps(12, 1))):
        want = compare_batch(L, maps, name, buf)
        print(name, len(maps), "maps;", sum(f for _r, f in want), "found,", sum(len(r) for r, _f in want), "kept")


def test_the_scan_equals_rule_r_on_random_maps_raw_and_dilated(scan, cases):
    L, buf = scan
    n = found = kept = 0
    for name, maps in cases[3:]:
        want = compare_batch(L, maps, name, buf)
        n += len(maps)
        found += sum(f for _r, f in want)
        kept += sum(len(r) for r, _f in want)
    assert n == 4 * N_RANDOM
    print(n, "maps;", found, "found,", kept, "kept")


def test_the_scan_equals_rule_r_on_rings(scan):
    L, buf = scan
    big = np.zeros(4 * 64 * 64, np.int32)
    for name, m in ring_maps().items():
        want = cr.external_rects(m)
        assert host_rects(L, np.ascontiguousarray(m), big) == want, (name, want)
        if "nested" in name and "gap" not in name:
            assert want[1] == 1 and len(want[0]) == 1, name


def _write_cases(path, groups, every):
    """the case file of tests/cpp/test_components.cpp: every map with rule R's answer, every `every`-th with labels and statistics"""
    count = 0
    with open(path, "wb") as f:
        f.write(struct.pack("<i", 0))
        for _name, maps in groups:
            want = cr.external_rects_batch(maps)
            for m, (rects, found) in zip(maps, want):
                h, w = m.shape
                f.write(struct.pack("<ii", w, h))
                f.write(np.ascontiguousarray(m).tobytes())
                f.write(struct.pack("<ii", found, len(rects)))
                f.write(np.asarray(rects, "<i4").tobytes())
                full = count % every == 0
                f.write(struct.pack("<i", int(full)))
                if full:
                    for conn in (8, 4):
                        labels, stats = cr.components(m, conn)
                        f.write(struct.pack("<i", len(stats)))
                        f.write(stats.astype("<i4").tobytes())
                        f.write(labels.astype("<i4").tobytes())
                count += 1
        f.seek(0)
        f.write(struct.pack("<i", count))
    return count


def test_components_h_under_the_sanitizers(tmp_path, cases):
    """tests/cpp/test_components.cpp under AddressSanitizer and UndefinedBehaviorSanitizer, a program of its own on the CPU: its own
    families against the literal scan of contour.h, then the maps of this file against the restatement's values"""
    exe = str(tmp_path / "test_components")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "test_components.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "components: OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    groups = list(cases) + [(name, m[None]) for name, m in ring_maps().items()]
    path = str(tmp_path / "cases.bin")
    n = _write_cases(path, groups, 16)
    assert n == 65536 + 2 * 4096 + 4 * N_RANDOM + len(ring_maps())
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "components: OK" in r.stdout and f"{n} maps" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_statuses_before_any_device(prl):
    from prlib_amd import _capi

    L = _capi.lib()
    n4 = np.zeros(4, np.int32)
    cnt, off = n4.ctypes.data, np.zeros(5, np.int32).ctypes.data
    cc, er = L.prl_hip_connected_components_batch_device, L.prl_hip_external_rects_batch_device

    def components(n=1, conn=8, mp=1, stride=64, step=8, w=8, h=8, lab=16, lstride=256, lstep=32, counts=cnt, stats=None, room=0):
        return cc(n, conn, mp, stride, step, w, h, lab, lstride, lstep, counts, stats, room, None)

    def rects(n=1, mp=1, stride=64, step=8, w=8, h=8, out=None, room=0, offsets=off, found=cnt, kept=cnt):
        return er(n, mp, stride, step, w, h, out, room, offsets, found, kept, None)

    assert components(w=0) == _capi.PRL_ERR_EMPTY and components(h=-1) == _capi.PRL_ERR_EMPTY
    assert components(w=0, conn=5) == _capi.PRL_ERR_EMPTY, "EMPTY comes first"
    for bad in (dict(conn=5), dict(conn=0), dict(mp=None), dict(n=-1), dict(step=7), dict(w=32769, step=40000, lstep=4 * 32769),
                dict(counts=None), dict(room=-1), dict(room=3), dict(lstep=28), dict(lab=18), dict(lstep=34)):
        assert components(**bad) == _capi.PRL_ERR_BAD_ARG, bad
    assert components(n=0) == _capi.PRL_OK and components(n=0, lab=None) == _capi.PRL_OK
    assert rects(w=0) == _capi.PRL_ERR_EMPTY
    for bad in (dict(mp=None), dict(n=-1), dict(step=7), dict(h=32769), dict(offsets=None), dict(found=None), dict(kept=None),
                dict(room=-1), dict(room=2)):
        assert rects(**bad) == _capi.PRL_ERR_BAD_ARG, bad
    assert rects(n=0) == _capi.PRL_OK


def test_exports_maps_and_python(prl):
    from prlib_amd import _capi, components

    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "prlib_amd", "libprlib_hip.so")], capture_output=True, text=True,
                         check=True).stdout
    header = open(os.path.join(ROOT, "include", "prl_hip.h")).read()
    for name in NEW_EXPORTS:
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(_capi.lib(), name)
        assert re.search(r"\bT " + name + r"\b", out), name
        assert re.search(r"^int " + name + r"\(", header, flags=re.M), name
        for m in ("prl_hip.map", "prl_hip_testhooks.map"):
            assert re.search(r"^\s+" + name + ";$", open(os.path.join(ROOT, "prlib_amd", "csrc", m)).read(), flags=re.M), (name, m)
    assert subprocess.run(["python3", os.path.join(ROOT, "tools", "gen_export_map.py"), "--check"]).returncode == 0
    assert "Rule R" in header and "straight one-pixel line" in header
    for fn in ("connectedComponents", "externalRects", "externalRectsDevice"):
        assert callable(getattr(components, fn))
    assert callable(prl.connectedComponents) and "connectedComponents" in prl.__all__
    assert prl.externalRects.__module__ == "prlib_amd.localotsu", "the host scan on numpy maps stays where it was"
    assert components.TILE == 32 and "constexpr int kCcTile = 32;" in open(os.path.join(ROOT, "prlib_amd", "csrc", "components.h")).read()
    for lists in ("prlib_amd/csrc/Makefile", "CMakeLists.txt"):
        assert "components" in open(os.path.join(ROOT, lists)).read(), lists
