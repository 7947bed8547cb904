"""prl::binarizeMokji without a device: the reference's loops against the numpy model on every size and parameter set of the GPU
tests (tests/mokji_ref.py), the integer threshold against the double sequence on random matrices and the extremes, the library's
host helper against both, a hand-computed answer, the C ABI's statuses in their documented order, the exports, and the drop-in
header's C++ contract."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mokji_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("prl_hip_binarize_mokji_batch_device", "prl_hip_binarize_mokji_host", "prl_hip_mokji_thresholds_batch_device",
           "prl_hip_cooccurrence_batch_device", "prl_hip_mokji_threshold")


def _c_threshold(L, matrix, m_min):
    m = np.ascontiguousarray(matrix, np.uint32)
    t = ctypes.c_int(12345)
    assert L.prl_hip_mokji_threshold(m.ctypes.data, m_min, ctypes.byref(t)) == 0
    return t.value


# ---- (a) == (b) ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", mr.SIZES, ids=[f"{w}x{h}" for w, h in mr.SIZES])
def test_loops_equal_the_numpy_model(size):
    w, h = size
    for name, page in mr.families(w, h, seed=3):
        loops = {}   # the interior loop depends on E alone
        for e, m in mr.params_of(size):
            mask_a, t_a, matrix = mr.mokji_loops(page, e, m, matrix=loops.get(e))
            loops[e] = matrix
            mask_b, t_b = mr.mokji(page, e, m)
            assert t_a == t_b and np.array_equal(mask_a, mask_b), (size, name, e, m, t_a, t_b)
            assert np.array_equal(np.array(matrix, np.int64), mr.mokji_matrix(page, e)), (size, name, e)
            assert t_a == mr.threshold_int(matrix, m), (size, name, e, m)
    for c in (3, 4):
        img = mr.colour_page(w, h, 5, c)
        mask_a, t_a, _ = mr.mokji_loops(img, 3, 20)
        mask_b, t_b = mr.mokji(img, 3, 20)
        assert t_a == t_b and np.array_equal(mask_a, mask_b) and mask_a.shape == (h, w), (size, c)


def test_the_two_dilations_agree():
    for w, h in ((64, 64), (203, 117), (9, 300), (300, 5)):
        g = mr.noise_page(w, h, 2)
        for e in (1, 3, 7, 127):
            assert np.array_equal(mr.dilate_shifts(g, e), mr.dilate_windows(g, e)), (w, h, e)
    g = np.zeros((9, 9), np.uint8)
    g[4, 4] = 200
    d = mr.dilate_windows(g, 2)
    assert (d[2:7, 2:7] == 200).all() and int((d == 200).sum()) == 25


def test_cooccurrence_model_properties():
    w, h = 203, 117
    a, b = mr.noise_page(w, h, 1), mr.noise_page(w, h, 2)
    for border in mr.BORDERS:
        full = mr.cooccurrence(a, b, border, 0)
        assert int(full.sum()) == (w - 2 * border) * (h - 2 * border)
        n, m = np.mgrid[0:256, 0:256]
        for md in mr.MIN_DIFFS:
            assert np.array_equal(mr.cooccurrence(a, b, border, md), full if md == 0 else np.where(n - m >= md, full, 0)), (border, md)
        assert np.triu(full, 1).sum() > 0   # pairs with b < a
    assert mr.cooccurrence(a, b, 59, 0).sum() == 0 and mr.cooccurrence(a, b, 0, 256).sum() == 0
    corners = mr.corners_page(w, h, 1)
    mat = mr.mokji_matrix(corners, 3)
    assert mat[0, 0] > 0 and mat[255, 255] > 0 and mat[255, 0] > 0 and np.triu(mat, 1).sum() == 0   # dil >= gray: the lower triangle


def test_kernel_accounting_equals_the_model():
    """the wavefront-uniform shortcut, the flat lanes and the row tails of k_mokji_cooc, emulated lane by lane in numpy, on every
    size and family of the GPU tests (every border; the largest size at border 3)"""
    for w, h in mr.SIZES + [(1100, 9), (259, 5)]:
        pages = [p for _, p in mr.families(w, h, seed=3)]
        for i, a in enumerate(pages):
            for b in (mr.dilate_shifts(a, 1), pages[i - 1]):
                for border in ([3] if (w, h) == mr.BIG else mr.BORDERS):
                    for md in (0, 20):
                        assert np.array_equal(mr.emulate_cooc(a, b, border, md), mr.cooccurrence(a, b, border, md)), (w, h, i, border, md)
    flat = mr.flat_page(1030, 4, 9)
    assert mr.emulate_cooc(flat, flat, 1, 0)[9, 9] == 1028 * 2 and mr.emulate_cooc(flat, flat, 1, 1).sum() == 0


# ---- (c) == the double sequence ------------------------------------------------------------------------------------------------

def _extreme_matrices():
    out = []
    z = np.zeros((256, 256), np.int64)
    for n, m in ((255, 0), (20, 0), (255, 235), (140, 101)):
        one = z.copy()
        one[n, m] = 2 ** 30          # one bin holding a whole page
        out.append((f"bin{n}_{m}", one, 20))
    for big_m in (1, 20, 255):
        diag = z.copy()              # all mass on n - m == M
        for m in range(0, 256 - big_m):
            diag[m + big_m, m] = 1 + (m * 7919) % 4099
        out.append((f"diag{big_m}", diag, big_m))
    odd = z.copy()                   # nom / den odd: 0.5 * nom / den ends in .5
    odd[101, 50] = 3                 # m + n = 151
    out.append(("odd", odd, 20))
    odd2 = z.copy()
    odd2[100, 51] = 2 ** 29
    odd2[200, 100] = 2 ** 29         # (151 + 300) / 2 = 225.5 -> 0.5 * that + 0.5
    out.append(("odd2", odd2, 20))
    one = z.copy()                   # den == 1
    one[255, 0] = 1
    out.append(("den1", one, 20))
    one2 = z.copy()
    one2[21, 0] = 1
    out.append(("den1_low", one2, 20))
    return out


def test_integer_threshold_equals_the_double_sequence(prl):
    from prlib_amd import _capi

    L = _capi.lib()
    rng = np.random.default_rng(7)
    n_checked = 0
    for i in range(10000):
        mat = np.zeros((256, 256), np.int64)
        k = int(rng.integers(1, 40))
        scale = int(rng.choice([2, 1000, 2 ** 20, 2 ** 30 // k]))
        mat[rng.integers(0, 256, k), rng.integers(0, 256, k)] = rng.integers(1, scale + 1, k)
        m_min = int(rng.choice([1, 5, 20, 40, 100, 255]))
        nom, den = mr.nom_den(mat, m_min)
        t_d, t_i = mr.threshold_double_of(nom, den), mr.threshold_int_of(nom, den)
        assert t_d == t_i, (i, nom, den)
        assert _c_threshold(L, mat, m_min) == t_d, (i, nom, den)
        n_checked += den > 0
    assert n_checked > 5000
    for name, mat, m_min in _extreme_matrices():
        nom, den = mr.nom_den(mat, m_min)
        assert den > 0, name
        t_d = mr.threshold_double_of(nom, den)
        assert t_d == mr.threshold_int_of(nom, den) == _c_threshold(L, mat, m_min), (name, nom, den)
    # every odd quotient a pair of bins can give
    for s in range(21, 510, 2):
        assert mr.threshold_double_of(s * 3, 3) == mr.threshold_int_of(s * 3, 3) == (s + 1) // 2, s
    # no pair: an all-zero matrix, M = 256 and above, mass only above or near the diagonal
    full = np.full((256, 256), 5, np.int64)
    assert _c_threshold(L, np.zeros((256, 256)), 20) == -1 and mr.threshold_int(np.zeros((256, 256)), 20) == -1
    for m_min in (256, 257, 100000, 2 ** 31 - 1):
        assert _c_threshold(L, full, m_min) == -1 and mr.threshold_double(full, m_min) == -1, m_min
    assert _c_threshold(L, np.triu(full, -19), 20) == -1 and _c_threshold(L, np.triu(full, -20), 20) >= 0
    assert _c_threshold(L, full, 255) == 128   # the single pair (255, 0): (255 + 1) / 2
    A = _capi.PRL_ERR_BAD_ARG
    t = ctypes.c_int(7)
    m = np.zeros((256, 256), np.uint32)
    assert L.prl_hip_mokji_threshold(None, 20, ctypes.byref(t)) == A and L.prl_hip_mokji_threshold(m.ctypes.data, 20, None) == A
    assert L.prl_hip_mokji_threshold(m.ctypes.data, 0, ctypes.byref(t)) == A and L.prl_hip_mokji_threshold(m.ctypes.data, -3, ctypes.byref(t)) == A
    assert t.value == 7
    assert prl.mokjiThreshold(full, 255) == 128 and prl.mokjiThreshold(np.zeros((256, 256)), 20) == -1


def test_known_answers():
    """a two-level page 50 | 200 with E = 1 and M = 20: the only pairs with an edge are (dil 200, gray 50) in the column left of
    the step, so nom / den = 250 and t = (int)(125 + 0.5) = 125"""
    page = mr.two_level_page(64, 40, 50, 200)
    mask, t, matrix = mr.mokji_loops(page, 1, 20)
    assert t == 125 and matrix[200][50] == 38 and matrix[50][50] == 38 * 30 and matrix[200][200] == 38 * 31
    assert np.array_equal(mask, np.where(page == 200, 255, 0)) and mr.mokji(page, 1, 20)[1] == 125
    # no edge of M: flat pages, and a step lower than M - all 255, t = -1
    for p in (mr.flat_page(40, 30, 0), mr.flat_page(40, 30, 255), mr.two_level_page(40, 30, 100, 119)):
        mask, t = mr.mokji(p, 3, 20)
        assert t == -1 and (mask == 255).all()
    assert mr.mokji(mr.two_level_page(40, 30, 100, 120), 3, 20)[1] == 110
    # no interior: cols <= 2E or rows <= 2E
    for w, h, e in ((257, 3, 2), (6, 40, 3), (64, 64, 128), (64, 64, 32)):
        mask, t, _ = mr.mokji_loops(mr.noise_page(w, h, 1), e, 20)
        assert t == -1 and (mask == 255).all(), (w, h, e)
    assert mr.mokji(mr.noise_page(64, 64, 1), 31, 20)[1] >= 0     # a 2 x 2 interior
    assert mr.mokji(mr.noise_page(64, 64, 1), 3, 256)[1] == -1 and mr.mokji(mr.noise_page(64, 64, 1), 3, 1000)[1] == -1
    with pytest.raises(ValueError, match="maxEdgeWidth"):
        mr.mokji_loops(page, 0, 0)
    with pytest.raises(ValueError, match="minEdgeMagnitude"):
        mr.mokji_loops(page, 1, 0)


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
    for f in ("binarizeMokji", "mokjiThresholds", "mokjiThreshold", "cooccurrence"):
        assert callable(getattr(prl, f)) and f in prl.__all__, f
    r = subprocess.run(["python", os.path.join(ROOT, "tools", "gen_export_map.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    assert os.path.exists(os.path.join(ROOT, "include", "prl", "binarizeMokji.h"))
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in SYMBOLS:
        assert name in integration, name
    for build_file in ("CMakeLists.txt", os.path.join("prlib_amd", "csrc", "Makefile")):
        assert re.search(r"\bmokji\b", open(os.path.join(ROOT, build_file)).read()), build_file
    if shutil.which("nm") is None:
        pytest.skip("binutils not installed")
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
    dst = np.zeros((60, 64), np.uint8)
    thr = np.zeros(4, np.int32)
    cooc = np.zeros((256, 256), np.uint32)
    s, d, tp, cp = src.ctypes.data, dst.ctypes.data, thr.ctypes.data, cooc.ctypes.data
    E, A, CH = _capi.PRL_ERR_EMPTY, _capi.PRL_ERR_BAD_ARG, _capi.PRL_ERR_BAD_CHANNELS

    def dev(n=1, c=1, e=3, m=20, sp=s, ss=256, w=64, h=60, dp=d, ds=64, spage=256 * 60, dpage=64 * 60):
        return L.prl_hip_binarize_mokji_batch_device(n, c, e, m, sp, spage, ss, w, h, dp, dpage, ds, None)

    def host(n=1, c=1, e=3, m=20, sp=s, ss=256, w=64, h=60, dp=d, ds=64, **_):
        return L.prl_hip_binarize_mokji_host(c, e, m, sp, ss, w, h, dp, ds)

    def thrs(n=1, c=1, e=3, m=20, sp=s, ss=256, w=64, h=60, dp=tp, spage=256 * 60, **_):
        return L.prl_hip_mokji_thresholds_batch_device(n, c, e, m, sp, spage, ss, w, h, dp, None)

    for f in (dev, host, thrs):
        assert f(w=0) == E and f(h=-1) == E and f(w=0, e=0, c=9, sp=None) == E                    # 1. empty
        assert f(e=0) == A and f(e=-2) == A and f(m=0) == A and f(m=-1) == A                        # 2. the arguments
        assert f(e=0, c=9) == A and f(m=0, c=2, sp=None) == A
        assert f(e=128, w=300, h=257, ss=1200) == A and f(e=128, w=300, h=257, c=7) == A            #    E > 127 with an interior
        assert f(e=128, w=300, h=256, c=7) == CH and f(e=1 << 30, c=0) == CH                        #    ... without one: not an error
        for c in (0, 2, 5, -1):
            assert f(c=c) == CH and f(c=c, sp=None) == CH and f(c=c, ss=1) == CH, c              # 3. channels
        assert f(sp=None) == A and f(dp=None) == A and f(ss=63) == A                                # 4. the rest
        assert f(c=3, ss=191) == A and f(c=4, ss=255) == A
        assert f(w=32769, ss=1 << 18, ds=1 << 18) == A and f(h=32769) == A
        if f is not host:
            assert f(n=-1) == A and f(n=0) == _capi.PRL_OK
        if no_gpu:
            for c in (1, 3, 4):
                assert f(c=c) not in (E, A, CH), c
            assert f(m=256) not in (E, A, CH) and f(m=2 ** 31 - 1) not in (E, A, CH) and f(e=127) not in (E, A, CH)
            assert f(e=128, w=64, h=60) not in (E, A, CH) and f(e=2 ** 31 - 1) not in (E, A, CH)
    assert dev(ds=63) == A and host(ds=63) == A
    # in place only for 1-channel pages at the same strides; any other overlap is refused
    assert dev(n=2, sp=s, dp=s + 64, ss=64, spage=64 * 60) == A
    assert dev(n=1, c=3, sp=s, dp=s) == A and dev(n=1, c=4, sp=s, dp=s, ds=256, dpage=256 * 60) == A
    assert dev(n=1, c=1, sp=s, dp=s, ss=256, ds=64) == A
    if no_gpu:
        assert dev(n=1, c=1, sp=s, dp=s, ss=256, ds=256, dpage=256 * 60) not in (E, A, CH)

    def co(n=1, border=0, md=0, ap=s, astep=256, bp=s, bstep=256, w=64, h=60, out=cp):
        return L.prl_hip_cooccurrence_batch_device(n, border, md, ap, 256 * 60, astep, bp, 256 * 60, bstep, w, h, out, None)

    assert co(w=0) == E and co(h=0, border=-1, ap=None) == E
    assert co(border=-1) == A and co(md=-1) == A and co(md=257) == A
    assert co(ap=None) == A and co(bp=None) == A and co(out=None) == A and co(astep=63) == A and co(bstep=63) == A
    assert co(n=-1) == A and co(n=0) == _capi.PRL_OK and co(w=32769, astep=40000, bstep=40000) == A and co(h=32769) == A
    if no_gpu:
        assert co(md=256) not in (E, A, CH) and co(border=1000) not in (E, A, CH)
    assert src.max() == 0 and dst.max() == 0 and thr.max() == 0 and cooc.max() == 0


def test_valid_call_without_a_device(prl):
    import torch

    from prlib_amd import _capi

    if torch.cuda.is_available():
        pytest.skip("a device is present; the no-device behaviour is checked on the CPU box")
    img = np.zeros((60, 64, 3), np.uint8)
    for call in (lambda: prl.binarizeMokji(img), lambda: prl.binarizeMokji(img[:, :, 0]), lambda: prl.binarizeMokji(img, 128, 300)):
        with pytest.raises(_capi.PrlError) as e:
            call()
        assert e.value.status == _capi.PRL_ERR_NO_DEVICE
    with pytest.raises(_capi.PrlError) as e:
        prl.binarizeMokji(img[:, :, :2])
    assert e.value.status == _capi.PRL_ERR_BAD_CHANNELS
    with pytest.raises(_capi.PrlError) as e:
        prl.binarizeMokji(img, 0, 20)
    assert e.value.status == _capi.PRL_ERR_BAD_ARG


# ---- the C++ drop-in ---------------------------------------------------------------------------------------------------------------

def build_dropin(out_dir):
    """g++ of tests/cpp/test_mokji_dropin.cpp + prl_host.cpp, with only -I include/prl for the drop-in header."""
    exe = os.path.join(out_dir, "test_mokji_dropin")
    flags = []
    for pc in ("opencv4", "opencv"):
        r = subprocess.run(["pkg-config", "--cflags", "--libs", pc], capture_output=True, text=True) if shutil.which("pkg-config") else None
        if r is not None and r.returncode == 0:
            flags = r.stdout.split()
            break
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include", "prl"),
           os.path.join(ROOT, "tests", "cpp", "test_mokji_dropin.cpp"), os.path.join(ROOT, "prlib_amd", "csrc", "prl", "prl_host.cpp"),
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
    assert r.returncode == 0 and "mokji dropin cpu: OK" in r.stdout, r.stdout + r.stderr
