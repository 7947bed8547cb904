"""The focus measures (LAPM, LAPV, TENG, GLVN) without a device: hand-computed answers, tests/focus_ref.py against an independent
scipy.ndimage.correlate(mode="mirror") model, focus.h's plain loop (a stand-alone g++ program) against focus_ref on the same
pages, prl_hip_focus_from_sums against the reference finalisation bit for bit, the C ABI's statuses in their documented order,
the exports, and the drop-in header's C++ contract."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import focus_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("prl_hip_focus_sums_batch_device", "prl_hip_focus_measures_host", "prl_hip_focus_from_sums")
SMALL = [(1, 1), (1, 2), (2, 1), (1, 7), (7, 1), (2, 2), (3, 3), (5, 4), (9, 13), (40, 33)]   # height x width


# ---- known answers -----------------------------------------------------------------------------------------------------------

def test_known_answers():
    page = np.zeros((5, 5), np.uint8)
    page[2, 2] = 255
    assert fr.sums(page).tolist() == [255, 65025, 0, 1300500, 8160, 1560600]
    assert fr.sums(page, 1).tolist() == [255, 65025, 0, 1300500, 8160, 4 * 65025]
    for h, w in ((1, 1), (5, 5), (3, 70)):
        white = fr.flat(h, w, 255)
        assert fr.sums(white).tolist() == [255 * h * w, 65025 * h * w, 0, 0, 0, 0]
        assert fr.same_bits(fr.measures(white), [0.0, 0.0, 0.0, 0.0]), (h, w)
        black = fr.measures(fr.flat(h, w, 0))
        assert np.isnan(black[fr.GLVN]) and black[:3].tolist() == [0.0, 0.0, 0.0], (h, w)
    # the worst cases reach the stated bounds on interior pixels, and only there
    h = w = 16
    inner = (h - 2) * (w - 2)
    assert fr.sums(fr.stripes4(h, w))[fr.SUM_TENG] >= inner * 1020 * 1020
    assert fr.sums(fr.checkerboard(h, w))[fr.SUM_LAP2] == h * w * fr.MAX_L ** 2      # reflection keeps the parity: every pixel
    assert fr.sums(fr.stripes2(h, w))[fr.SUM_LAPM4] == h * w * fr.MAX_XY
    assert fr.MAX_SIDE ** 2 * fr.MAX_TENG < 2 ** 53


def test_reflect101():
    assert fr.reflect101(np.array([-1, 0, 4, 5]), 5).tolist() == [1, 0, 4, 3]
    assert fr.reflect101(np.array([-1, 0, 1, 2]), 2).tolist() == [1, 0, 1, 0]
    assert fr.reflect101(np.array([-1, 0, 1]), 1).tolist() == [0, 0, 0]


# ---- focus_ref against scipy ---------------------------------------------------------------------------------------------------

def _scipy_sums(p, ksize):
    """An independent model: whole-kernel 2-D correlations with scipy's `mirror` border (d c b | a b c d | c b a: REFLECT_101)."""
    ndi = pytest.importorskip("scipy.ndimage")
    f = p.astype(np.int64)

    def corr(k):
        return ndi.correlate(f, np.array(k, np.int64), mode="mirror")

    lap = corr([[0, 1, 0], [1, -4, 1], [0, 1, 0]])
    x = corr(np.outer([1, 2, 1], [-1, 2, -1]))
    y = corr(np.outer([-1, 2, -1], [1, 2, 1]))
    if ksize == 3:
        gx, gy = corr(np.outer([1, 2, 1], [-1, 0, 1])), corr(np.outer([-1, 0, 1], [1, 2, 1]))
    else:
        gx, gy = corr([[0, 0, 0], [-1, 0, 1], [0, 0, 0]]), corr([[0, -1, 0], [0, 0, 0], [0, 1, 0]])
    return [int(v.sum()) for v in (f, f * f, lap, lap * lap, np.abs(x) + np.abs(y), gx * gx + gy * gy)]


@pytest.mark.parametrize("size", SMALL + [(64, 65), (130, 257)], ids=lambda s: "%dx%d" % s)
def test_ref_equals_the_scipy_model(size):
    h, w = size
    for seed, page in enumerate([fr.noise(h, w, 1, 1), fr.noise(h, w, 1, 2), fr.extremes(h, w, 3), fr.checkerboard(h, w)]):
        for ks in (1, 3):
            assert fr.sums(page, ks).tolist() == _scipy_sums(page, ks), (size, seed, ks)


# ---- focus.h on the CPU ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def focus_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    exe = str(tmp_path_factory.mktemp("focus") / "test_focus")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "test_focus.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _run_loop(exe, page, ks, tmp_path, pad=0):
    """page: H x W [x C]; pad: extra bytes per row (a step above the row bytes) -> (sums [C, 6], measure bits [C, 4])"""
    p3 = page if page.ndim == 3 else page[:, :, None]
    h, w, c = p3.shape
    buf = np.full((h, w * c + pad), 0xAB, np.uint8)
    buf[:, :w * c] = p3.reshape(h, w * c)
    path = os.path.join(str(tmp_path), "page.raw")
    buf.tofile(path)
    r = subprocess.run([exe, str(h), str(w), str(c), str(ks), str(w * c + pad), path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [line.split() for line in r.stdout.strip().splitlines()]
    assert [int(x[0]) for x in rows] == list(range(c))
    return (np.array([[int(v) for v in x[1:7]] for x in rows], np.int64),
            np.array([[int(v, 16) for v in x[7:11]] for x in rows], np.uint64).view(np.float64))


def test_header_self_check(focus_exe):
    r = subprocess.run([focus_exe, "self"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "focus self: OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("channels", (1, 3, 4))
def test_plain_loop_equals_ref(focus_exe, tmp_path, channels):
    for h, w in SMALL + [(70, 261)]:
        for ks in (1, 3):
            page = fr.noise(h, w, channels, 5) if (h + w) % 2 else fr.extremes(h, w * channels, 5).reshape((h, w) if channels == 1 else (h, w, channels))
            got, bits = _run_loop(focus_exe, page, ks, tmp_path, pad=(h + w) % 3)
            want = fr.sums(page, ks).reshape(channels, 6)
            assert np.array_equal(got, want), (h, w, channels, ks)
            assert fr.same_bits(bits, fr.from_sums(want, w, h)), (h, w, channels, ks)
    zero = _run_loop(focus_exe, fr.flat(4, 6, 0), 3, tmp_path)[1]
    assert np.isnan(zero[0, fr.GLVN]) and zero[0, :3].tolist() == [0.0, 0.0, 0.0]


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------

def _c_from_sums(L, s, w, h):
    s = np.ascontiguousarray(s, np.int64)
    m = np.full(4, -7.0)
    assert L.prl_hip_focus_from_sums(s.ctypes.data, w, h, m.ctypes.data) == 0
    return m


def test_from_sums_equals_the_reference_finalisation(prl):
    from prlib_amd import _capi

    L = _capi.lib()
    rng = np.random.default_rng(11)
    cases = []
    for h, w in SMALL + [(70, 261)]:
        for page in (fr.noise(h, w, 1, 8), fr.extremes(h, w, 8), fr.checkerboard(h, w), fr.flat(h, w, 0), fr.flat(h, w, 255), fr.flat(h, w, 1)):
            for ks in (1, 3):
                cases.append((fr.sums(page, ks), w, h))
    # N = 1; zero sums; the bounds on the largest page: every pixel at its largest term
    n_max = fr.MAX_SIDE ** 2
    cases += [(np.array([255, 65025, 0, 0, 0, 0]), 1, 1), (np.zeros(6, np.int64), 1, 1), (np.zeros(6, np.int64), 32768, 32768),
              (np.array([255 * n_max, 65025 * n_max, 0, 0, 0, 0]), 32768, 32768),
              (np.array([127 * n_max, 65025 * n_max // 2, 0, n_max * fr.MAX_L ** 2, n_max * fr.MAX_XY, n_max * fr.MAX_TENG]), 32768, 32768),
              (np.array([1, 1, -1020, 1040400, 1, 1]), 32768, 32768), (np.array([1, 1, 1020 * n_max, n_max * fr.MAX_L ** 2, 3, 7]), 32768, 32768),
              (np.array([3, 9, -5, 25, 2, 1]), 3, 1), (np.array([5, 13, -4, 40, 7, 11]), 1, 3)]
    for _ in range(2000):   # random sums a page could give: S_P2 >= S_P^2 / N is not required of the formula
        w, h = int(rng.integers(1, 32769)), int(rng.integers(1, 32769))
        n = w * h
        cases.append((np.array([rng.integers(0, 255 * n + 1), rng.integers(0, 65025 * n + 1), rng.integers(-fr.MAX_L * n, fr.MAX_L * n + 1),
                                rng.integers(0, fr.MAX_L ** 2 * n + 1), rng.integers(0, fr.MAX_XY * n + 1), rng.integers(0, fr.MAX_TENG * n + 1)]), w, h))
    for s, w, h in cases:
        assert fr.same_bits(_c_from_sums(L, s, w, h), fr.from_sums(s, w, h)), (s, w, h)
    assert fr.same_bits(prl.focusFromSums(np.stack([c[0] for c in cases[:4]]), cases[0][1], cases[0][2]),
                        fr.from_sums(np.stack([c[0] for c in cases[:4]]), cases[0][1], cases[0][2]))
    E, A = _capi.PRL_ERR_EMPTY, _capi.PRL_ERR_BAD_ARG
    s, m = np.zeros(6, np.int64), np.full(4, 5.0)
    assert L.prl_hip_focus_from_sums(s.ctypes.data, 0, 4, m.ctypes.data) == E and L.prl_hip_focus_from_sums(None, 4, -1, None) == E
    assert L.prl_hip_focus_from_sums(None, 4, 4, m.ctypes.data) == A and L.prl_hip_focus_from_sums(s.ctypes.data, 4, 4, None) == A
    assert L.prl_hip_focus_from_sums(s.ctypes.data, 32769, 4, m.ctypes.data) == A and L.prl_hip_focus_from_sums(s.ctypes.data, 4, 32769, m.ctypes.data) == A
    assert m.tolist() == [5.0] * 4


def test_declared_and_exported(prl):
    from prlib_amd import _capi

    header = open(os.path.join(ROOT, "include", "prl_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _capi.EXPORTED_SYMBOLS
        for m in ("prl_hip.map", "prl_hip_testhooks.map"):
            assert re.search(r"\b" + name + r";", open(os.path.join(ROOT, "prlib_amd", "csrc", m)).read()), (name, m)
    assert re.search(r"#define PRL_HIP_ABI_VERSION 4\b", header)
    for bound in ("1020", "2040", "2 * 1020^2", "2^53"):
        assert bound in header, bound
    for f in ("focusSums", "focusMeasures", "focusFromSums"):
        assert callable(getattr(prl, f)) and f in prl.__all__, f
    r = subprocess.run(["python", os.path.join(ROOT, "tools", "gen_export_map.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    assert os.path.exists(os.path.join(ROOT, "include", "prl", "blurDetection.h"))
    assert "prl_hip_focus_sums_batch_device" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for build_file in ("CMakeLists.txt", os.path.join("prlib_amd", "csrc", "Makefile")):
        assert re.search(r"\bfocus\b", open(os.path.join(ROOT, build_file)).read()), build_file
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
    src = np.zeros((60, 64 * 4), np.uint8)
    sums = np.zeros((4, 4, 6), np.int64)
    meas = np.zeros((4, 4), np.float64)
    s, sp, mp = src.ctypes.data, sums.ctypes.data, meas.ctypes.data
    E, A, CH = _capi.PRL_ERR_EMPTY, _capi.PRL_ERR_BAD_ARG, _capi.PRL_ERR_BAD_CHANNELS

    def dev(n=1, c=1, ks=3, src_p=s, ss=256, w=64, h=60, out=sp, spage=256 * 60):
        return L.prl_hip_focus_sums_batch_device(n, c, ks, src_p, spage, ss, w, h, out, None)

    def host(n=1, c=1, ks=3, src_p=s, ss=256, w=64, h=60, out=mp, **_):
        return L.prl_hip_focus_measures_host(c, ks, src_p, ss, w, h, out, None)

    for f in (dev, host):
        assert f(w=0) == E and f(h=-1) == E and f(w=0, ks=5, c=9, src_p=None) == E                 # 1. empty
        for ks in (0, 2, 5, 7, -1, -3):
            assert f(ks=ks) == A and f(ks=ks, c=2) == A and f(ks=ks, c=9, src_p=None) == A, ks      # 2. the Sobel size
        for c in (0, 2, 5, -1):
            assert f(c=c) == CH and f(c=c, src_p=None) == CH and f(c=c, ss=1) == CH and f(c=c, out=None) == CH, c   # 3. channels
        assert f(src_p=None) == A and f(out=None) == A and f(ss=63) == A                            # 4. the rest
        assert f(c=3, ss=191) == A and f(c=4, ss=255) == A
        assert f(w=32769, ss=1 << 18) == A and f(h=32769) == A
        if f is dev:
            assert f(n=-1) == A and f(n=0) == _capi.PRL_OK and f(n=0, src_p=None) == A
        if no_gpu:
            for c in (1, 3, 4):
                for ks in (1, 3):
                    assert f(c=c, ks=ks) == _capi.PRL_ERR_NO_DEVICE, (c, ks)
    assert src.max() == 0 and sums.max() == 0 and meas.max() == 0


def test_valid_call_without_a_device(prl):
    import torch

    from prlib_amd import _capi

    if torch.cuda.is_available():
        pytest.skip("a device is present; the no-device behaviour is checked on the CPU box")
    img = np.zeros((60, 64, 3), np.uint8)
    for call in (lambda: prl.focusMeasures(img), lambda: prl.focusMeasures(img[:, :, 0]), lambda: prl.focusMeasures(img, 1)):
        with pytest.raises(_capi.PrlError) as e:
            call()
        assert e.value.status == _capi.PRL_ERR_NO_DEVICE
    with pytest.raises(_capi.PrlError) as e:
        prl.focusMeasures(img[:, :, :2])
    assert e.value.status == _capi.PRL_ERR_BAD_CHANNELS
    with pytest.raises(_capi.PrlError) as e:
        prl.focusMeasures(img, 5)
    assert e.value.status == _capi.PRL_ERR_BAD_ARG


# ---- the C++ drop-in ---------------------------------------------------------------------------------------------------------------

def build_dropin(out_dir):
    """g++ of tests/cpp/test_focus_dropin.cpp + prl_host.cpp, with only -I include/prl for the drop-in header."""
    exe = os.path.join(out_dir, "test_focus_dropin")
    flags = []
    for pc in ("opencv4", "opencv"):
        r = subprocess.run(["pkg-config", "--cflags", "--libs", pc], capture_output=True, text=True) if shutil.which("pkg-config") else None
        if r is not None and r.returncode == 0:
            flags = r.stdout.split()
            break
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include", "prl"),
           os.path.join(ROOT, "tests", "cpp", "test_focus_dropin.cpp"), os.path.join(ROOT, "prlib_amd", "csrc", "prl", "prl_host.cpp"),
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
    assert r.returncode == 0 and "focus dropin cpu: OK" in r.stdout, r.stdout + r.stderr
