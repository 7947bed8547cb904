"""prl::removeLines without a device: the restatement (tests/lines_ref.py) against its independent run-length model, the known
answers of the line openings, the numpy emulation of the kernels' word algorithm against both models on every size of the GPU
tests, the C ABI's statuses in their documented order, the exports, and the drop-in header's C++ contract."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import lines_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("prl_hip_remove_lines_batch_device", "prl_hip_remove_lines_host")


@pytest.fixture(scope="module")
def oracle_built(oracle):
    return oracle


def _models_agree(name, page):
    want = lr.remove_lines(page)
    assert np.array_equal(lr.remove_lines_runs(page), want), name
    return want


@pytest.mark.parametrize("size", lr.SIZES, ids=[f"{w}x{h}" for w, h in lr.SIZES])
def test_models_and_word_emulation_agree(oracle_built, size):
    """restatement == run-length model == the kernels' word algorithm, on every family and size the GPU tests use"""
    w, h = size
    for name, page in lr.families(w, h, seed=3):
        want = _models_agree((size, name), page)
        bw, _ = lr.mask_of(page)
        assert np.array_equal(lr.emulate_words(bw), want), (size, name)


def test_word_emulation_on_more_geometries(oracle_built):
    """every L from 1 to 9 and around the word size; heights that put the band seams and the halo at odd places"""
    rng = np.random.default_rng(5)
    for w, h in [(50 * k + r, 50 + 3 * k) for k in (1, 2, 3, 4, 5, 6, 7, 8, 9, 31, 32, 33) for r in (0, 49)] + [(77, 2000), (130, 6143)]:
        bw = rng.random((h, w)) < 0.97
        hor, ver = lr.openings(bw)
        assert np.array_equal(lr.emulate_words(bw), lr.compose(bw, hor, ver)), (w, h)
        g = lr.geometry(w, h)
        assert 2 * (g["TH"] + 2 * (g["Lv"] - 1)) * g["CW"] * 8 <= 61440 and 2 * g["nr"] * g["P"] * 8 <= 61440 and g["TH"] >= 1
    for w, h in ((32768, 32768), (32768, 50), (50, 32768), (2480, 3508)):   # the limits stay inside the LDS budget
        g = lr.geometry(w, h)
        assert 2 * (min(g["TH"], h) + 2 * (g["Lv"] - 1)) * g["CW"] * 8 <= 61440 and 2 * g["nr"] * g["P"] * 8 <= 61440 and g["TH"] >= 1
    assert lr.geometry(2480, 3508)["L"] == 49 and lr.geometry(2480, 3508)["Lv"] == 70 and lr.geometry(2480, 3508)["CW"] == 8


def _line_page(w, h, y, x0, n):
    p = np.full((h, w), lr.PAPER, np.uint8)
    p[y, x0:x0 + n] = lr.INK
    p[h - 10:h - 8, 10:14] = lr.INK   # some ink that is no line (2 x 4 pixels)
    return p


@pytest.mark.parametrize("w", [1050, 1000])
def test_line_known_answers(oracle_built, w):
    """odd L = 21 (width 1050) and even L = 20 (width 1000): a 1-pixel line of L - 1 survives, L and L + 1 are removed"""
    h, y, x0 = 150, 20, 300   # Lv = 3: a 1-pixel line is no vertical run
    L = w // 50
    for n, removed in ((L - 1, False), (L, True), (L + 1, True)):
        out = lr.remove_lines(_line_page(w, h, y, x0, n))
        assert np.array_equal(out, lr.remove_lines_runs(_line_page(w, h, y, x0, n)))
        row = out[y]
        if not removed:
            assert (row[x0:x0 + n] == 0).all() and (row[:x0] == 255).all() and (row[x0 + n:] == 255).all()
        elif L % 2 == 1:
            assert (row == 255).all(), (w, n)
        else:
            # even L: not a true opening - the opening is shifted one pixel to the right, so of a removed run the first pixel
            # survives (and the pixel after the run is flagged, harmlessly)
            assert row[x0] == 0 and (row[x0 + 1:] == 255).all() and (row[:x0] == 255).all()
        assert (out[h - 10:h - 8, 10:14] == 0).all() and (np.delete(out, y, axis=0)[:h - 11] == 255).all()
    if L % 2 == 0:
        bw = np.zeros((h, w), bool)
        bw[y, x0:x0 + L] = True
        hor, _ = lr.openings(bw)
        assert np.flatnonzero(hor[y]).tolist() == list(range(x0 + 1, x0 + L + 1))   # the opening is the run shifted by one


def test_lines_touching_the_borders(oracle_built):
    w, h = 1000, 500   # L = 20, Lv = 10
    for n in (5, 12, 19, 20, 30):
        p = np.full((h, w), lr.PAPER, np.uint8)
        p[100, :n] = lr.INK          # from the left border
        p[200, w - n:] = lr.INK      # to the right border
        p[:n // 2 + 1, 300] = lr.INK     # from the top
        p[h - n // 2 - 1:, 600] = lr.INK  # to the bottom
        p[400:403, 400:403] = lr.INK
        out = lr.remove_lines(p)
        assert np.array_equal(out, lr.remove_lines_runs(p)), n
        bw, _ = lr.mask_of(p)
        assert np.array_equal(lr.emulate_words(bw), out), n
        # taps outside the page are ignored: a run at a border needs only the taps that fall inside.  Left: offsets -10 .. 9, so
        # 10 pixels from column 0 erode at column 0; right: 11 pixels to the last column
        assert (out[100, 0] == 255) == (n >= 10) and (out[200, w - 1] == 255) == (n >= 11), n
        assert (out[100, :n] == 255).all() == (n >= 10)
        assert (out[400:403, 400:403] == 0).all()


def test_small_elements_and_flat_pages(oracle_built):
    rng = np.random.default_rng(2)
    for w, h in ((50, 120), (77, 120), (99, 120), (120, 50), (120, 99)):   # a 1 x 1 element: the opening is bw, all white
        page = lr._page(w, h, rng.random((h, w)) < 0.4)
        assert (lr.remove_lines(page) == 255).all() and (lr.remove_lines_runs(page) == 255).all(), (w, h)
    for v in (0, 255, 128):
        for c in (1, 3):
            flat = np.full((130, 140, c), v, np.uint8)
            assert (lr.remove_lines(flat[:, :, 0] if c == 1 else flat) == 255).all()
    for w, h in ((49, 200), (200, 49), (1, 1)):
        with pytest.raises(ValueError):
            lr.remove_lines(np.zeros((h, w), np.uint8))
    with pytest.raises(ValueError):
        lr.remove_lines(np.zeros((60, 60, 4), np.uint8))


def test_threshold_is_not_the_mirror_of_otsu_on_gray(oracle_built):
    """Otsu runs on the inverted page.  On pages with a tie in the between-class variance the first maximum of the scan over
    inv is not the mirror image of the first maximum over gray: the thresholds differ, and so do the masks."""
    for mid, t_want, t_gray_want, ink in ((4, 105, 100, True), (8, 130, 125, False)):
        page = lr.tie_page(mid)
        half = page == 125
        bw, t = lr.mask_of(page)
        t_gray = oracle_built.otsu(page)[0]
        mirrored = 254 - t_gray                  # gray > t_gray  ==  inv <= 254 - t_gray: what a mirrored scan would give
        assert (t, t_gray) == (t_want, t_gray_want) and t != mirrored, mid
        mirrored_bw = (255 - page) > mirrored
        assert bw[half].all() == ink and bw[half].any() == ink and mirrored_bw[half].all() == (not ink), mid
        out = lr.remove_lines(page)
        # the dark class is one large blob and is opened away; where the half-way pixels are ink, those on the light side
        # stand alone, too short for a line, and are what remains
        lone = half & (np.arange(page.shape[1]) >= page.shape[1] // 2)[None, :]
        assert np.array_equal(out == 0, lone if ink else np.zeros_like(half)), mid
        assert np.array_equal(out, lr.remove_lines_runs(page)) and np.array_equal(lr.emulate_words(bw), out)
    # colour goes through the 14-bit luma
    rng = np.random.default_rng(9)
    bgr = rng.integers(0, 256, size=(64, 80, 3), dtype=np.uint8)
    assert np.array_equal(lr.remove_lines(bgr), lr.remove_lines(oracle_built.bgr2gray(bgr)))


def test_declared_and_exported(prl):
    from prlib_amd import _capi

    header = open(os.path.join(ROOT, "include", "prl_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _capi.EXPORTED_SYMBOLS
        for m in ("prl_hip.map", "prl_hip_testhooks.map"):
            assert re.search(r"\b" + name + r";", open(os.path.join(ROOT, "prlib_amd", "csrc", m)).read()), (name, m)
    assert re.search(r"#define PRL_HIP_ABI_VERSION 4\b", header)
    assert callable(prl.removeLines) and "removeLines" in prl.__all__
    r = subprocess.run(["python", os.path.join(ROOT, "tools", "gen_export_map.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    assert os.path.exists(os.path.join(ROOT, "include", "prl", "removeLines.h"))
    assert "prl_hip_remove_lines_batch_device" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    if shutil.which("nm") is None:
        pytest.skip("binutils not installed")
    for lib in ("libprlib_hip.so", "libprlib_hip_testhooks.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "prlib_amd", lib)], capture_output=True, text=True,
                             check=True).stdout
        for name in SYMBOLS:
            assert re.search(r"\bT " + name + r"\b", out), (lib, name)


def test_statuses_in_their_order_without_touching_a_device(prl):
    from prlib_amd import _capi

    L = _capi.lib()
    src = np.zeros((60, 64 * 3), np.uint8)
    dst = np.zeros((60, 64), np.uint8)
    s, d = src.ctypes.data, dst.ctypes.data
    E, A, CH = _capi.PRL_ERR_EMPTY, _capi.PRL_ERR_BAD_ARG, _capi.PRL_ERR_BAD_CHANNELS

    def dev(n=1, c=1, sp=s, ss=192, w=64, h=60, dp=d, ds=64, spage=192 * 60, dpage=64 * 60):
        return L.prl_hip_remove_lines_batch_device(n, c, sp, spage, ss, w, h, dp, dpage, ds, None)

    def host(n=1, c=1, sp=s, ss=192, w=64, h=60, dp=d, ds=64, **_):
        return L.prl_hip_remove_lines_host(c, sp, ss, w, h, dp, ds)

    for f in (dev, host):
        assert f(w=0) == E and f(h=-1) == E and f(w=0, c=9, sp=None) == E              # empty first
        for c in (0, 2, 4, 5, -1):
            assert f(c=c) == CH, c
        assert f(c=2, w=49) == CH and f(c=4, sp=None) == CH and f(c=0, ss=1) == CH      # channels before everything else
        for w, h in ((49, 60), (64, 49), (1, 1), (49, 49)):
            assert f(w=w, h=h) == A and f(w=w, h=h, c=3) == A, (w, h)
        assert f(sp=None) == A and f(dp=None) == A and f(ss=63) == A and f(ds=63) == A
        assert f(c=3, ss=191) == A and f(c=3, ss=192) != A
        assert f(w=32769, ss=40000, ds=40000) == A and f(h=32769) == A
    assert dev(n=-1) == A and dev(n=0) == _capi.PRL_OK
    # in place only for 1-channel pages at the same strides; any other overlap is refused
    assert dev(n=2, sp=s, dp=s + 64, ss=64, spage=64 * 60) == A
    assert dev(n=1, c=3, sp=s, dp=s) == A
    assert dev(n=1, c=1, sp=s, dp=s, ss=192, ds=64) == A
    assert src.max() == 0 and dst.max() == 0


def test_valid_call_without_a_device(prl):
    import torch

    from prlib_amd import _capi

    if torch.cuda.is_available():
        pytest.skip("a device is present; the no-device behaviour is checked on the CPU box")
    img = np.zeros((60, 64, 3), np.uint8)
    with pytest.raises(_capi.PrlError) as e:
        prl.removeLines(img)
    assert e.value.status == _capi.PRL_ERR_NO_DEVICE
    with pytest.raises(_capi.PrlError) as e:
        prl.removeLines(img[:, :, 0])
    assert e.value.status == _capi.PRL_ERR_NO_DEVICE
    with pytest.raises(_capi.PrlError) as e:
        prl.removeLines(img[:40])
    assert e.value.status == _capi.PRL_ERR_BAD_ARG
    with pytest.raises(_capi.PrlError) as e:
        prl.removeLines(np.zeros((60, 64, 4), np.uint8))
    assert e.value.status == _capi.PRL_ERR_BAD_CHANNELS


def build_dropin(out_dir):
    """g++ of tests/cpp/test_lines_dropin.cpp + prl_host.cpp, with only -I include/prl for the drop-in header."""
    exe = os.path.join(out_dir, "test_lines_dropin")
    flags = []
    for pc in ("opencv4", "opencv"):
        r = subprocess.run(["pkg-config", "--cflags", "--libs", pc], capture_output=True, text=True) if shutil.which("pkg-config") else None
        if r is not None and r.returncode == 0:
            flags = r.stdout.split()
            break
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include", "prl"),
           os.path.join(ROOT, "tests", "cpp", "test_lines_dropin.cpp"), os.path.join(ROOT, "prlib_amd", "csrc", "prl", "prl_host.cpp"),
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
    assert r.returncode == 0 and "lines dropin cpu: OK" in r.stdout, r.stdout + r.stderr
