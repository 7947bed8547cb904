"""cv::CLAHE, cv::equalizeHist and EnhanceLocalContrastByCLAHE without a device: tests/clahe_ref.py against an independent float64
evaluation of its blend within a derived distance, its invariants and OpenCV's quirks each by name, the three host-only C entries
against it bit for bit, clahe.h's plain loops (a stand-alone g++ program, once more under the address and undefined-behaviour
sanitizers) against vectors it dumped into tests/golden/ and against fresh pages, the C ABI's statuses in their documented order,
the exports, and the drop-in header's C++ contract."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import clahe_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "clahe_vectors.bin")
SYMBOLS = ("prl_hip_clahe_geometry", "prl_hip_clahe_tile_lut", "prl_hip_equalize_hist_lut", "prl_hip_clahe_luts_batch_device",
           "prl_hip_clahe_batch_device", "prl_hip_clahe_host", "prl_hip_equalize_hist_batch_device", "prl_hip_equalize_hist_host",
           "prl_hip_enhance_local_contrast_batch_device", "prl_hip_enhance_local_contrast_host")


# ---- the restatement itself --------------------------------------------------------------------------------------------------

def test_ref_against_float64():
    """The blend of four table entries in float64, from the same tables and the same float32 weights xa, ya taken as exact numbers.
    The float32 evaluation makes 11 roundings (xa1, ya1, six products, three sums) of values of at most 255, each within 2^-24
    relative: it is within 11 * 2^-24 * 255 = 1.7e-4 of the float64 value (whose own error is 1e-13).  So the rounded bytes must be
    equal wherever the float64 value is farther than 1e-3 from a half-integer, and within one grey level everywhere."""
    worst, ties = 0.0, 0
    for h, w, tiles, clip in ((67, 130, (8, 8), 40.0), (40, 33, (8, 8), 2.0), (64, 90, (3, 5), 0.0), (17, 16, (8, 8), 3.0), (9, 9, (8, 8), 40.0),
                              (130, 67, (64, 64), 1e6), (50, 70, (1, 8), 0.5), (301, 257, (8, 8), 2.0)):
        for page in (cr.noise(h, w, 1, 3), cr.gradient(h, w), cr.paper(h, w, 1, 2)):
            got = cr.clahe(page, clip, tiles).astype(np.int64)
            exact = cr.plane_blend64(page, clip, tiles)
            assert exact.min() >= 0.0 and exact.max() <= 255.0
            decided = np.abs(exact - np.floor(exact) - 0.5) > 1e-3
            ties += int((~decided).sum())
            want = np.rint(exact).astype(np.int64)
            assert np.array_equal(got[decided], want[decided]), (h, w, tiles, clip)
            assert np.abs(got - exact).max() <= 1.0, (h, w, tiles, clip)
            worst = max(worst, float(np.abs(got - exact)[decided].max()))
    print("float64 distance of the rounded bytes where decided:", worst, "undecided pixels:", ties)
    assert worst <= 0.5 + 1e-3
    assert 11 * 2.0 ** -24 * 255 < 1e-3


def test_tables_are_monotone_and_end_at_255():
    for seed, (h, w, tiles) in enumerate(((67, 130, (8, 8)), (13, 16, (8, 8)), (33, 20, (3, 5)), (5, 5, (64, 64)))):
        for clip in (0.0, 0.5, 2.0, 40.0, 1e6):
            L = cr.plane_luts(cr.noise(h, w, 1, seed), clip, tiles).astype(int)
            assert (np.diff(L, axis=-1) >= 0).all() and (L[..., 255] == 255).all(), (h, w, tiles, clip)


def test_redistribution_preserves_the_bin_total():
    rng = np.random.default_rng(5)
    for clip in (1, 2, 3, 17, 100, 5000):
        hist = rng.integers(0, 400, size=(32, 256))
        hist[::3] = np.where(rng.random((11, 256)) < 0.9, 0, hist[::3] * 9)
        out = cr.redistribute(hist, clip)
        assert np.array_equal(out.sum(axis=1), hist.sum(axis=1))
        for t in range(0, 32, 5):
            assert np.array_equal(out[t], cr.redistribute_loop(hist[t], clip)), (clip, t)   # the slice form == the loop as written


def test_clip_of_one_gives_a_near_linear_table():
    """clip = 1 with a tile of `area` pixels: every bin holds min(h, 1) + area' / 256 (+ 1), so the table rises by a constant slope
    within (bins' spread of at most 2) * 255 / area per entry"""
    page = cr.noise(64, 64, 1, 9)
    tw, th, _, _, clip = cr.geometry(64, 64, (1, 1), 0.01)
    assert clip == 1
    L = cr.plane_luts(page, 0.01, (1, 1))[0, 0].astype(float)
    line = 255.0 * (np.arange(256) + 1) / 256
    assert np.abs(L - line).max() <= 2 * 255.0 * 256 / (tw * th) + 0.5


def test_equalize_flat_and_two_valued():
    for v in (0, 7, 255):
        page = cr.flat(9, 11, v)
        assert np.array_equal(cr.equalize(page), page)                 # a flat page comes back unchanged
    page = cr.two_valued(20, 31, 40, 200)
    out = cr.equalize(page)
    assert set(np.unique(out)) == {0, 255} and np.array_equal(out == 0, page == 40)
    one = cr.flat(10, 10, 90)
    one[3, 4] = 91                                                       # the first non-empty bin holds all but one pixel
    out = cr.equalize(one)
    assert out[3, 4] == 255 and (np.delete(out.ravel(), 34) == 0).all()
    lut = cr.equalize_lut(cr.histogram(cr.noise(40, 50, 1, 1)))
    assert (np.diff(lut.astype(int)) >= 0).all() and lut[255] == 255


# ---- the quirks, by name ------------------------------------------------------------------------------------------------------------

def test_quirk_a_divisible_side_grows_by_a_whole_tiles():
    assert cr.geometry(16, 13)[:4] == (3, 2, 24, 16)      # 16 % 8 == 0 and still 16 -> 24
    assert cr.geometry(16, 16)[:4] == (2, 2, 16, 16)
    assert cr.geometry(13, 16)[:4] == (2, 3, 16, 24)
    page = cr.noise(13, 16, 1, 1)
    assert cr.extended(page, (8, 8)).shape == (16, 24)
    assert np.array_equal(cr.extended(page, (8, 8))[:13, 16:], page[:, [14, 13, 12, 11, 10, 9, 8, 7]])


def test_quirk_a_side_of_one():
    assert cr.reflect101(np.arange(9), 1).tolist() == [0] * 9
    page = cr.noise(1, 5, 1, 2)
    ext = cr.extended(page, (8, 8))
    assert ext.shape == (8, 8) and (ext == ext[0]).all()
    out = cr.clahe(cr.noise(1, 1, 1, 3), 40.0)
    assert out.shape == (1, 1) and out[0, 0] == 255        # one value per tile: every table is 255 from that value on


def test_quirk_a_pad_longer_than_the_side():
    assert cr.reflect101(np.arange(3, 11), 3).tolist() == [1, 0, 1, 2, 1, 0, 1, 2]   # side 3, pad 5: the index turns round twice
    assert cr.reflect101(np.arange(2, 8), 2).tolist() == [0, 1, 0, 1, 0, 1]
    page = cr.noise(3, 3, 1, 4)
    ext = cr.extended(page, (8, 8))
    assert ext.shape == (8, 8) and np.array_equal(ext[:, 3:], ext[:, [1, 0, 1, 2, 1]]) and np.array_equal(ext[3:], ext[[1, 0, 1, 2, 1]])
    assert cr.geometry(130, 67, (64, 64))[:4] == (3, 2, 192, 128)   # a pad of 62 and 61 on the issue's grid


def test_quirk_the_stepped_residual_is_not_the_2_4_rule():
    hist = np.zeros(256, np.int64)
    hist[7], hist[100] = 310, 90                            # clip 10: clipped = 380, batch 1, residual 124, step 2
    new, old = cr.redistribute(hist, 10), cr.redistribute_v24(hist, 10)
    assert new.sum() == old.sum() == 400 and not np.array_equal(new, old)
    want = np.ones(256, np.int64)
    want[0:248:2] += 1
    want[7] += 10
    want[100] += 10
    assert np.array_equal(new, want)
    assert old[:124].sum() - new[:124].sum() == 62          # 2.4 puts all 124 into the first 124 bins, 3.4 half of them
    assert not np.array_equal(cr.tile_lut(hist, 10, 400), cr.sat_u8(np.cumsum(old).astype(np.float32) * (np.float32(255) / np.float32(400))))


def test_quirk_ties_round_to_even():
    """tile_w of 1 or 2 makes xa exactly 0.5 (tile_w 1: every column; 2: the even ones), so res lands on k + 0.5"""
    for w, tile in ((8, 1), (16, 2)):
        _, _, xa, xa1 = cr.axis(w, tile, 8)
        assert (xa[::tile] == 0.5).all() and (xa1[::tile] == 0.5).all()
    found = 0
    for seed in range(4):
        page = cr.noise(8, 8, 1, seed)
        exact = cr.plane_blend64(page, 0.0)
        tie = exact - np.floor(exact) == 0.5
        found += int(tie.sum())
        got = cr.clahe(page, 0.0)
        assert (got[tie] % 2 == 0).all() and np.array_equal(got[tie], np.rint(exact[tie]).astype(np.uint8))
    assert found > 20


# ---- the host-only C entries -------------------------------------------------------------------------------------------------------

def test_geometry_entry_equals_the_restatement(prl):
    for w in list(range(1, 20)) + [64, 127, 130, 2480, 32768]:
        for h in (1, 2, 7, 8, 13, 16, 67, 3508, 32768):
            for tiles in ((8, 8), (1, 1), (3, 5), (64, 64), (1, 8)):
                for clip in (0.0, -1.0, 0.5, 2.0, 40.0, 1e6, 1e300, float("inf")):
                    assert prl.claheGeometry(w, h, tiles, clip) == cr.geometry(w, h, tiles, clip), (w, h, tiles, clip)
    assert prl.claheGeometry(2480, 3508, (8, 8), 2.0) == (311, 439, 2488, 3512, 1066)
    assert prl.claheGeometry(16, 13) == (3, 2, 24, 16, 1)


def test_tile_lut_entry_equals_the_restatement(prl):
    rng = np.random.default_rng(11)
    for k in range(60):
        area = int(rng.integers(1, 5000))
        bins = np.bincount(rng.integers(0, 256 if k % 3 else 9, area), minlength=256).astype(np.uint32)
        for clip in (0, 1, 2, 3, 40, area):
            assert np.array_equal(prl.claheTileLut(bins, clip), cr.tile_lut(bins, clip, area)), (k, clip)
    big = np.zeros(256, np.uint32)
    big[200] = 32832 * 32832                                # the largest tile: one tile on the largest page
    assert np.array_equal(prl.claheTileLut(big, 1), cr.tile_lut(big, 1, int(big[200])))


def test_equalize_lut_entry_equals_the_restatement(prl):
    rng = np.random.default_rng(12)
    for k in range(40):
        n = int(rng.integers(1, 9000))
        bins = np.bincount(rng.integers(k % 7, 256 if k % 2 else 20, n), minlength=256).astype(np.uint32)
        assert np.array_equal(prl.equalizeHistLut(bins), cr.equalize_lut(bins)), k
    one = np.zeros(256, np.uint32)
    one[77] = (1 << 30) - 1                                  # with the next line: the largest page
    assert np.array_equal(prl.equalizeHistLut(one), np.arange(256, dtype=np.uint8))
    one[255] = 1
    assert prl.equalizeHistLut(one).tolist() == [0] * 255 + [255]


# ---- clahe.h on the CPU ------------------------------------------------------------------------------------------------------------

def _build(tmp, name, extra):
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    exe = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-ffp-contract=off"] + extra +
                       [os.path.join(ROOT, "tests", "cpp", "test_clahe.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def clahe_exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("clahe"), "test_clahe", [])


def test_golden_vectors_are_the_restatements():
    assert open(GOLDEN, "rb").read() == cr.golden_bytes()
    assert os.path.getsize(GOLDEN) < 16 * 1024


def test_header_self_check_and_golden_vectors(clahe_exe):
    r = subprocess.run([clahe_exe, "self"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "clahe self: OK" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([clahe_exe, "golden", GOLDEN], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "clahe golden: OK (%d records)" % (len(cr.GOLDEN_PAGES) + len(cr.GOLDEN_TILES)) in r.stdout, r.stdout + r.stderr


def _run(exe, page, tiles, clip, with_clahe, eq, tmp_path, pad=0):
    p3 = page if page.ndim == 3 else page[:, :, None]
    h, w, c = p3.shape
    buf = np.full((h, w * c + pad), 0xAB, np.uint8)
    buf[:, :w * c] = p3.reshape(h, w * c)
    src, out = os.path.join(str(tmp_path), "page.raw"), os.path.join(str(tmp_path), "out.raw")
    buf.tofile(src)
    r = subprocess.run([exe, "run", str(h), str(w), str(c), str(tiles[0]), str(tiles[1]), repr(clip), str(int(with_clahe)), str(int(eq)),
                        str(w * c + pad), src, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    return np.fromfile(out, np.uint8).reshape(page.shape)


@pytest.mark.parametrize("channels", (1, 2, 3, 4))
def test_plain_loop_equals_ref(clahe_exe, tmp_path, channels):
    for i, (h, w) in enumerate(((1, 1), (1, 7), (7, 1), (2, 3), (13, 16), (16, 16), (17, 9), (40, 33), (67, 130))):
        page = cr.noise(h, w, channels, 5) if i % 2 else cr.paper(h, w, channels, i)
        for tiles, clip in (((8, 8), 40.0), ((8, 8), 0.0), ((8, 8), 0.5), ((3, 5), 2.0), ((64, 64), 3.0), ((1, 1), 1e6)):
            got = _run(clahe_exe, page, tiles, clip, True, False, tmp_path, pad=(h + w) % 3)
            assert np.array_equal(got, cr.clahe(page, clip, tiles)), (h, w, channels, tiles, clip)
        assert np.array_equal(_run(clahe_exe, page, (8, 8), 0.0, False, True, tmp_path, pad=1), cr.equalize(page)), (h, w, channels)
        assert np.array_equal(_run(clahe_exe, page, (8, 8), 2.0, True, True, tmp_path), cr.enhance(page, 2.0, True)), (h, w, channels)


def test_plain_loop_under_the_sanitizers(tmp_path):
    """the stand-alone program on pages smaller than the grid, with address and undefined-behaviour checks"""
    # (the runtimes linked statically: the program does not depend on where the loader finds them)
    exe = _build(tmp_path, "test_clahe_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                                              "-static-libubsan"])
    for args in (["narrow"], ["self"], ["golden", GOLDEN]):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "clahe %s: OK" % args[0] in r.stdout, r.stdout + r.stderr[-3000:]


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
    assert re.search(r"#define PRL_CLAHE_MAX_TILES %d\b" % cr.MAX_TILES, header) and prl.contrast.MAX_TILES == cr.MAX_TILES
    for f in ("clahe", "claheLuts", "equalizeHist", "enhanceLocalContrast", "claheGeometry", "claheTileLut", "equalizeHistLut"):
        assert callable(getattr(prl, f)) and f in prl.__all__, f
    r = subprocess.run(["python", os.path.join(ROOT, "tools", "gen_export_map.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    assert os.path.exists(os.path.join(ROOT, "include", "prl", "imageLibCommon.h"))
    assert "prl_hip_enhance_local_contrast_batch_device" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for build_file in ("CMakeLists.txt", os.path.join("prlib_amd", "csrc", "Makefile")):
        assert re.search(r"\bclahe\b", open(os.path.join(ROOT, build_file)).read()), build_file
    kernel_header = open(os.path.join(ROOT, "prlib_amd", "csrc", "clahe.h")).read()
    for name, value in (("kClaheHistBandRows", cr.HIST_BAND_ROWS), ("kClaheHistUnitPx", cr.HIST_UNIT_PX), ("kClaheBlockW", cr.BLOCK_W),
                        ("kClaheBlockH", cr.BLOCK_H), ("kClaheStageTables", cr.STAGE_TABLES), ("kClaheMaxTiles", cr.MAX_TILES)):
        assert re.search(r"constexpr int %s = %d;" % (name, value), kernel_header), name   # the GPU tests take their sizes from these
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
    out = np.zeros(1 << 16, np.uint8)
    s, o = buf.ctypes.data, out.ctypes.data
    E, CH, A = _capi.PRL_ERR_EMPTY, _capi.PRL_ERR_BAD_CHANNELS, _capi.PRL_ERR_BAD_ARG
    nan = float("nan")
    D = dict(n=1, c=1, clip=40.0, tx=8, ty=8, eq=1, src=s, spage=256 * 60, ss=256, w=64, h=60, dst=o, dpage=256 * 60, ds=256)

    def call(name, **kw):
        a = dict(D, **kw)
        page_d = (a["src"], a["spage"], a["ss"], a["w"], a["h"], a["dst"], a["dpage"], a["ds"], None)
        page_h = (a["src"], a["ss"], a["w"], a["h"], a["dst"], a["ds"])
        if name == "clahe_dev":
            return L.prl_hip_clahe_batch_device(a["n"], a["c"], a["clip"], a["tx"], a["ty"], *page_d)
        if name == "clahe_host":
            return L.prl_hip_clahe_host(a["c"], a["clip"], a["tx"], a["ty"], *page_h)
        if name == "luts_dev":
            return L.prl_hip_clahe_luts_batch_device(a["n"], a["c"], a["clip"], a["tx"], a["ty"], a["src"], a["spage"], a["ss"], a["w"], a["h"],
                                                     a["dst"], None)
        if name == "eq_dev":
            return L.prl_hip_equalize_hist_batch_device(a["n"], a["c"], *page_d)
        if name == "eq_host":
            return L.prl_hip_equalize_hist_host(a["c"], *page_h)
        if name == "enh_dev":
            return L.prl_hip_enhance_local_contrast_batch_device(a["n"], a["c"], a["clip"], a["eq"], *page_d)
        return L.prl_hip_enhance_local_contrast_host(a["c"], a["clip"], a["eq"], *page_h)

    for name in ("clahe_dev", "clahe_host", "luts_dev", "eq_dev", "eq_host", "enh_dev", "enh_host"):
        f = lambda **kw: call(name, **kw)  # noqa: E731
        dev, grid, limit, rows_out = name.endswith("_dev"), name in ("clahe_dev", "clahe_host", "luts_dev"), not name.startswith("eq"), name != "luts_dev"
        assert f(w=0) == E and f(h=-1) == E and f(w=0, c=9, src=None, tx=0, clip=nan) == E                      # 1. empty
        for c in (0, 5, -1):                                                                                  # 2. channels
            assert f(c=c) == CH and f(c=c, src=None) == CH and f(c=c, ss=1, tx=99, clip=nan) == CH, c
        assert f(src=None) == A and f(dst=None) == A and f(ss=63) == A and f(c=3, ss=191) == A                  # 3. the rest
        assert f(w=32769, ss=1 << 16, ds=1 << 16) == A and f(h=32769) == A
        if rows_out:
            assert f(ds=63) == A and f(c=4, ds=255) == A
        if grid:
            for t in (0, -1, 65, 1 << 20):
                assert f(tx=t) == A and f(ty=t) == A, t
        if limit:
            assert f(clip=nan) == A
        if dev:
            assert f(n=-1) == A and f(n=0) == _capi.PRL_OK and f(n=0, src=None) == A and f(n=0, c=7) == CH
        if dev and rows_out:
            # exact in place is allowed; any other shared byte is refused
            assert f(dst=s + 1) == A and f(dst=s + 59 * 256 + 63) == A and f(dst=s, ds=512, dpage=512 * 60) == A
            assert f(n=2, dst=s, dpage=256 * 61, spage=256 * 60) == A
            assert f(dst=s + 128, w=16, h=4) == A
        if no_gpu:
            N = _capi.PRL_ERR_NO_DEVICE
            for c in (1, 2, 3, 4):
                assert f(c=c, ss=256, ds=256) == N, (name, c)
            assert f(clip=0.0) == N and f(clip=-5.0) == N and f(clip=float("inf")) == N and f(tx=64, ty=1) == N and f(tx=1, ty=64) == N
            if dev and rows_out:
                assert f(dst=s) == N and f(n=3, dst=s, spage=256 * 60, dpage=256 * 60) == N        # in place
    assert buf.max() == 0 and out.max() == 0
    # the host-only entries
    v = [ctypes.c_int(-5) for _ in range(5)]
    refs = [ctypes.byref(x) for x in v]
    assert L.prl_hip_clahe_geometry(0, 5, 8, 8, 40.0, *refs) == E and L.prl_hip_clahe_geometry(5, 0, 0, 8, nan, *([None] * 5)) == E
    for bad in ((5, 5, 0, 8, 40.0), (5, 5, 8, 65, 40.0), (5, 5, 8, 8, nan), (32769, 5, 8, 8, 40.0), (5, 32769, 8, 8, 40.0)):
        assert L.prl_hip_clahe_geometry(*bad, *refs) == A, bad
    assert L.prl_hip_clahe_geometry(5, 5, 8, 8, 40.0, None, *refs[1:]) == A and [x.value for x in v] == [-5] * 5
    bins = np.zeros(256, np.uint32)
    bins[3] = 10
    lut = np.full(256, 7, np.uint8)
    assert L.prl_hip_clahe_tile_lut(bins.ctypes.data, 1, 0, lut.ctypes.data) == E
    assert L.prl_hip_clahe_tile_lut(None, 1, 10, lut.ctypes.data) == A and L.prl_hip_clahe_tile_lut(bins.ctypes.data, 1, 10, None) == A
    assert L.prl_hip_clahe_tile_lut(bins.ctypes.data, -1, 10, lut.ctypes.data) == A and L.prl_hip_clahe_tile_lut(bins.ctypes.data, 1, 11, lut.ctypes.data) == A
    assert L.prl_hip_equalize_hist_lut(None, lut.ctypes.data) == A and L.prl_hip_equalize_hist_lut(bins.ctypes.data, None) == A
    assert L.prl_hip_equalize_hist_lut(np.zeros(256, np.uint32).ctypes.data, lut.ctypes.data) == E
    assert lut.tolist() == [7] * 256
    assert L.prl_hip_clahe_tile_lut(bins.ctypes.data, 1, 10, lut.ctypes.data) == 0 and lut[255] == 255


def test_valid_call_without_a_device(prl):
    import torch

    from prlib_amd import _capi

    if torch.cuda.is_available():
        pytest.skip("a device is present; the no-device behaviour is checked on the CPU box")
    img = np.zeros((60, 64, 3), np.uint8)
    for call in (lambda: prl.clahe(img), lambda: prl.clahe(img[:, :, 0], 2.0, (3, 5)), lambda: prl.equalizeHist(img),
                 lambda: prl.enhanceLocalContrast(img, 2.0, True), lambda: prl.enhanceLocalContrast(img, 2.0, out=img)):
        with pytest.raises(_capi.PrlError) as e:
            call()
        assert e.value.status == _capi.PRL_ERR_NO_DEVICE
    with pytest.raises(_capi.PrlError) as e:
        prl.clahe(img, 2.0, (0, 8))
    assert e.value.status == _capi.PRL_ERR_BAD_ARG
    with pytest.raises(_capi.PrlError) as e:
        prl.enhanceLocalContrast(img, float("nan"))
    assert e.value.status == _capi.PRL_ERR_BAD_ARG
    with pytest.raises(TypeError):
        prl.clahe(img, out=np.zeros((60, 64), np.uint8))


# ---- the C++ drop-in ---------------------------------------------------------------------------------------------------------------

def build_dropin(out_dir):
    """g++ of tests/cpp/test_clahe_dropin.cpp + prl_host.cpp, with only -I include/prl for the drop-in header."""
    exe = os.path.join(out_dir, "test_clahe_dropin")
    flags = []
    for pc in ("opencv4", "opencv"):
        r = subprocess.run(["pkg-config", "--cflags", "--libs", pc], capture_output=True, text=True) if shutil.which("pkg-config") else None
        if r is not None and r.returncode == 0:
            flags = r.stdout.split()
            break
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include", "prl"),
           os.path.join(ROOT, "tests", "cpp", "test_clahe_dropin.cpp"), os.path.join(ROOT, "prlib_amd", "csrc", "prl", "prl_host.cpp"),
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
    assert r.returncode == 0 and "clahe dropin cpu: OK" in r.stdout, r.stdout + r.stderr


def test_dropin_compiles_against_opencvs_declared_api():
    """the caller and prl_host.cpp against the declaration-only OpenCV headers (tests/cpp/opencv_api): only what OpenCV has is used"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    cpp = os.path.join(ROOT, "tests", "cpp")
    for src in (os.path.join(cpp, "test_clahe_dropin.cpp"), os.path.join(ROOT, "prlib_amd", "csrc", "prl", "prl_host.cpp")):
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-DPRL_REQUIRE_OPENCV",
                            "-I" + os.path.join(cpp, "opencv_api"), "-I" + os.path.join(ROOT, "include", "prl"), src], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
