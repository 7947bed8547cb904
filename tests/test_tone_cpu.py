"""The tone functions without a device: the reference's statements loop for loop against their per-pixel numpy form against the
histogram -> table -> look-up model (tests/tone_ref.py: the factorisation tone.hip rests on), the library's host table builders
against the model on ordinary and degenerate histograms, the gray-world sum over the bins against the raster-order sum, the
clean-background curve's 256 values, the C ABI's statuses in their documented order, the exports, and the drop-in headers' C++
contract."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import tone_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("prl_hip_histogram_batch_device", "prl_hip_lut_batch_device", "prl_hip_gamma_correction_batch_device",
           "prl_hip_gamma_correction_host", "prl_hip_simple_white_balance_batch_device", "prl_hip_simple_white_balance_host",
           "prl_hip_gray_world_batch_device", "prl_hip_gray_world_host", "prl_hip_clean_background_batch_device",
           "prl_hip_clean_background_host", "prl_hip_gamma_lut", "prl_hip_clean_background_lut", "prl_hip_simple_white_balance_luts",
           "prl_hip_gray_world_luts")
BIG = (1031, 517)
SMALL = (23, 17)


@pytest.fixture(scope="module")
def big_pages():
    """the three pages the header's statement about the gray-world sum names, plus the other families; built once"""
    return dict(tr.colour_families(*BIG, seed=1))


def _lib(prl):
    from prlib_amd import _capi

    return _capi.lib(), _capi


def _c_gamma_lut(L, k, gamma):
    out = np.zeros(256, np.uint8)
    assert L.prl_hip_gamma_lut(k, gamma, out.ctypes.data) == 0
    return out


def _c_luts(fn, hist, *args):
    h = np.ascontiguousarray(hist, np.uint32)
    out = np.zeros((3, 256), np.uint8)
    st = fn(*args, h.ctypes.data, out.ctypes.data)
    return st, out


# ---- the factorisation ---------------------------------------------------------------------------------------------------------

def test_loops_equal_the_numpy_literal_and_the_model_on_small_pages():
    w, h = SMALL
    for name, page in tr.colour_families(w, h, seed=4):
        for k in (0.01, 0.25, float("nan")):
            want = tr.swb_loops(page, k)
            assert np.array_equal(tr.swb_literal(page, k), want) and np.array_equal(tr.swb_model(page, k), want), (name, k)
        for p, wm in ((1.0, False), (2.5, True), (6.0, False)):
            want = tr.gw_loops(page, p, wm)
            assert np.array_equal(tr.gw_literal(page, p, wm), want) and np.array_equal(tr.gw_model(page, p, wm), want), (name, p, wm)
    for c in (1, 2, 3, 4):
        page = tr.noise_page(w, h, c, 7 + c)
        for k, gamma in ((1.0, 2.2), (0.5, 0.4), (1.7, 1.0), (1.0 + 5e-8, 2.2)):
            want = tr.gamma_loops(page, k, gamma)
            assert want.shape == (h, w, 3 if c == 4 else c)
            assert np.array_equal(tr.gamma_literal(page, k, gamma), want) and np.array_equal(tr.gamma_model(page, k, gamma), want), (c, k)
    g = tr.noise_page(w, h, 1, 3)[:, :, 0]
    assert np.array_equal(tr.gamma_loops(g, 0.5, 2.2), tr.gamma_model(g, 0.5, 2.2)) and tr.gamma_model(g, 0.5, 2.2).shape == (h, w)


def test_literal_equals_the_table_model_on_every_family(big_pages):
    for name, page in big_pages.items():
        for k in tr.SWB_KS:
            assert np.array_equal(tr.swb_literal(page, k), tr.swb_model(page, k)), (name, k)
        for p in (1.0, 2.0, 3.0):
            for wm in (False, True):
                assert np.array_equal(tr.gw_literal(page, p, wm), tr.gw_model(page, p, wm)), (name, p, wm)
        for gamma in tr.GAMMAS:
            for k in tr.GAMMA_KS:
                assert np.array_equal(tr.gamma_literal(page, k, gamma), tr.gamma_model(page, k, gamma)), (name, k, gamma)
    bgra = tr.noise_page(203, 117, 4, 2)
    for k in tr.GAMMA_KS:
        got = tr.gamma_model(bgra, k, 2.2)
        assert got.shape == (117, 203, 3) and np.array_equal(got, tr.gamma_literal(bgra, k, 2.2))
        assert np.array_equal(got, tr.k_step_lut(k)[bgra[:, :, :3]])   # no gamma, the alpha byte dropped


def test_known_answers_of_the_degenerate_pages():
    w, h = 40, 30
    zero = tr.flat_page(w, h, (0, 0, 0))
    assert (tr.gw_model(zero, 1.0, False) == 255).all() and (tr.gw_literal(zero, 2.0, True) == 255).all()   # NaN -> 255
    zc = tr.noise_page(w, h, 3, 1)
    zc[:, :, 1] = 0
    assert (tr.gw_model(zc, 1.0, False)[:, :, 1] == 255).all()
    for k in (0.0, 0.01, 0.5):
        flat = tr.swb_model(tr.flat_page(w, h, (100, 100, 100)), k)
        assert np.array_equal(flat, tr.swb_literal(tr.flat_page(w, h, (100, 100, 100)), k)) and len(np.unique(flat)) == 1
    for k in (-1.0, float("nan")):   # the identity by the literal comparisons
        page = tr.noise_page(w, h, 3, 2)
        assert np.array_equal(tr.swb_model(page, k), page)
    assert np.array_equal(tr.swb_model(tr.flat_page(w, h, (0, 0, 0)), 0.01), tr.swb_literal(tr.flat_page(w, h, (0, 0, 0)), 0.01))
    for k in (25.0, 1.5):   # the reference's own sample passes k = 25: both scans stop at the array's ends
        page = tr.noise_page(w, h, 3, 3)
        assert np.array_equal(tr.swb_model(page, k), tr.swb_literal(page, k))
    assert np.array_equal(tr.gamma_lut(1.0, 1.0), np.arange(256)) and np.array_equal(tr.gamma_lut(1.0 + 5e-8, 1.0), np.arange(256))
    assert tr.gamma_lut(0.5, 1.0)[[1, 3, 5, 255]].tolist() == [0, 2, 2, 128]   # 0.5, 1.5, 2.5, 127.5: half to even
    assert tr.gamma_lut(1.7, 1.0)[151] == 255 and tr.gamma_lut(1.7, 1.0)[150] == 255 and tr.gamma_lut(1.7, 1.0)[149] == 253


def test_histogram_kernel_accounting_equals_bincount():
    """the wavefront-uniform shortcut of k_tone_hist, emulated lane by lane in numpy, on every size, channel count and family of
    the GPU tests"""
    for w, h in tr.HIST_SIZES:
        for c in (1, 2, 3, 4):
            for name, page in tr.hist_families(w, h, c, seed=3):
                assert np.array_equal(tr.emulate_hist(page), tr.histograms(page)), (w, h, c, name)
    flat = tr.flat_page(1024, 3, (9, 9, 200))
    assert tr.emulate_hist(flat)[2, 200] == 3072 and tr.emulate_hist(flat)[0, 9] == 3072


# ---- the gray-world sum ------------------------------------------------------------------------------------------------------------

def test_gray_world_sum_over_bins_against_the_raster_sum(big_pages):
    """p = 1, 2, 3: the means are bit-identical.  p = 6, 0.5, 2.5 on the three pages the header names: the means may differ in
    their last bits, the output bytes do not (re-verified here on every run)."""
    for name in ("noise", "paper", "gray3"):
        page = big_pages[name]
        hist, total = tr.histograms(page), page.shape[0] * page.shape[1]
        for p in (1.0, 2.0, 3.0):
            a, b = tr.gw_means_hist(p, hist, total), tr.gw_means_raster(page, p)
            assert [float(x).hex() for x in a] == [float(x).hex() for x in b], (name, p)
        for p in (6.0, 0.5, 2.5):
            for wm in (False, True):
                n_bad = int((tr.gw_model(page, p, wm) != tr.gw_literal(page, p, wm)).sum())
                print(f"{name} p = {p} withMax = {wm}: {n_bad} differing bytes against the raster-order literal")
                assert n_bad == 0, (name, p, wm)


# ---- the library's builders ------------------------------------------------------------------------------------------------------

def _degenerate_hists(total=1031 * 517):
    z = np.zeros((3, 256), np.int64)
    out = {}
    for name, fill in (("zero_channels", {0: total}), ("flat255", {255: total}), ("flat100", {100: total}),
                       ("two_valued", {40: total // 3, 215: total - total // 3}), ("ends", {0: total // 2, 255: total - total // 2}),
                       ("one_each_end", {0: 1, 128: total - 2, 255: 1})):
        h = z.copy()
        for v, n in fill.items():
            h[:, v] = n
        out[name] = h
    mixed = z.copy()
    mixed[0, 0] = total          # an all-zero channel beside two ordinary ones
    mixed[1, 10:250] = total // 240
    mixed[1, 10] += total - int(mixed[1].sum())
    mixed[2, 200] = total
    out["mixed"] = mixed
    return out


def test_builders_equal_the_model(prl, big_pages):
    L, _capi = _lib(prl)
    for gamma in tr.GAMMAS + [0.0, -1.0, float("nan")]:
        for k in tr.GAMMA_KS + [0.0, -2.0, 300.0, 1e12, float("nan")]:
            assert np.array_equal(_c_gamma_lut(L, k, gamma), tr.gamma_lut(k, gamma)), (k, gamma)
    hists = {name: tr.histograms(page) for name, page in big_pages.items()}
    hists.update(_degenerate_hists())
    for name, h in hists.items():
        for k in tr.SWB_KS + [1.0, 25.0, 0.999]:
            st, got = _c_luts(L.prl_hip_simple_white_balance_luts, h, k)
            assert st == 0 and np.array_equal(got, tr.swb_luts(k, h)), (name, k)
        for p in tr.GW_PS:
            for wm in (0, 1):
                st, got = _c_luts(L.prl_hip_gray_world_luts, h, p, wm)
                assert st == 0 and np.array_equal(got, tr.gw_luts(p, bool(wm), h)), (name, p, wm)
    # a tiny page: the scans' stops and the +1 below 254
    h = np.zeros((3, 256), np.int64)
    h[:, 3] = 1
    for k in (0.0, 0.5, 1.0):
        st, got = _c_luts(L.prl_hip_simple_white_balance_luts, h, k)
        assert st == 0 and np.array_equal(got, tr.swb_luts(k, h)), k


def test_clean_background_table_has_its_stated_values(prl):
    L, _ = _lib(prl)
    got = np.zeros(256, np.uint8)
    assert L.prl_hip_clean_background_lut(got.ctypes.data) == 0
    assert np.array_equal(got, tr.CLEAN_LUT) and np.array_equal(tr.clean_lut(), tr.CLEAN_LUT)
    assert (got[:71] == 0).all() and (got[170:] == 255).all() and len(set(got.tolist())) == 101
    assert got[70:76].tolist() == [0, 3, 5, 8, 10, 13] and got[168:171].tolist() == [250, 252, 255]


def test_builder_statuses(prl):
    L, _capi = _lib(prl)
    E, A = _capi.PRL_ERR_EMPTY, _capi.PRL_ERR_BAD_ARG
    h = np.zeros((3, 256), np.uint32)
    out = np.zeros((3, 256), np.uint8)
    assert L.prl_hip_gamma_lut(1.0, 1.0, None) == A and L.prl_hip_clean_background_lut(None) == A
    for fn, args in ((L.prl_hip_simple_white_balance_luts, (0.01,)), (L.prl_hip_gray_world_luts, (1.0, 0))):
        assert fn(*args, None, out.ctypes.data) == A and fn(*args, h.ctypes.data, None) == A
        assert fn(*args, h.ctypes.data, out.ctypes.data) == E                       # no pixel
        h2 = h.copy()
        h2[:, 5] = 7
        h2[2, 6] = 1
        assert fn(*args, h2.ctypes.data, out.ctypes.data) == A                      # the channels' sums differ
        h3 = h.copy()
        h3[:, 0] = 2 ** 30
        h3[:, 1] = 1
        assert fn(*args, h3.ctypes.data, out.ctypes.data) == A                      # more pixels than the largest page
    assert out.max() == 0


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
    for f in ("gammaCorrection", "simpleWhiteBalance", "grayWorldWhiteBalance", "cleanBackgroundToWhite", "histogram", "lut"):
        assert callable(getattr(prl, f)) and f in prl.__all__, f
    r = subprocess.run(["python", os.path.join(ROOT, "tools", "gen_export_map.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    for h in ("gammaCorrection.h", "balanceSimpleWhite.h", "balanceGrayWorldWhite.h", "cleanBackgroundToWhite.h"):
        assert os.path.exists(os.path.join(ROOT, "include", "prl", h)), h
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in SYMBOLS:
        assert name in integration, name
    if shutil.which("nm") is None:
        pytest.skip("binutils not installed")
    for lib in ("libprlib_hip.so", "libprlib_hip_testhooks.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "prlib_amd", lib)], capture_output=True, text=True,
                             check=True).stdout
        for name in SYMBOLS:
            assert re.search(r"\bT " + name + r"\b", out), (lib, name)


def test_statuses_in_their_order_without_touching_a_device(prl):
    import torch

    L, _capi = _lib(prl)
    no_gpu = not torch.cuda.is_available()   # a valid device call on these host arrays must never reach a device
    src = np.zeros((60, 64 * 4), np.uint8)
    dst = np.zeros((60, 64 * 4), np.uint8)
    aux = np.zeros(4 * 256 * 4, np.uint8)
    s, d, x = src.ctypes.data, dst.ctypes.data, aux.ctypes.data
    E, A, CH = _capi.PRL_ERR_EMPTY, _capi.PRL_ERR_BAD_ARG, _capi.PRL_ERR_BAD_CHANNELS

    def entries(c_in_args):
        """(name, callable(n, c, sp, spage, ss, w, h, dp, dpage, ds), is a device entry, takes channels)"""
        return [
            ("gamma_dev", lambda n, c, sp, spg, ss, w, h, dp, dpg, ds: L.prl_hip_gamma_correction_batch_device(n, c, 0.5, 2.2, sp, spg, ss, w, h, dp, dpg, ds, None), True, True),
            ("gamma_host", lambda n, c, sp, spg, ss, w, h, dp, dpg, ds: L.prl_hip_gamma_correction_host(c, 0.5, 2.2, sp, ss, w, h, dp, ds), False, True),
            ("clean_dev", lambda n, c, sp, spg, ss, w, h, dp, dpg, ds: L.prl_hip_clean_background_batch_device(n, c, sp, spg, ss, w, h, dp, dpg, ds, None), True, True),
            ("clean_host", lambda n, c, sp, spg, ss, w, h, dp, dpg, ds: L.prl_hip_clean_background_host(c, sp, ss, w, h, dp, ds), False, True),
            ("lut_dev", lambda n, c, sp, spg, ss, w, h, dp, dpg, ds: L.prl_hip_lut_batch_device(n, c, x, 0, sp, spg, ss, w, h, dp, dpg, ds, None), True, True),
            ("swb_dev", lambda n, c, sp, spg, ss, w, h, dp, dpg, ds: L.prl_hip_simple_white_balance_batch_device(n, 0.01, sp, spg, ss, w, h, dp, dpg, ds, None), True, False),
            ("swb_host", lambda n, c, sp, spg, ss, w, h, dp, dpg, ds: L.prl_hip_simple_white_balance_host(0.01, sp, ss, w, h, dp, ds), False, False),
            ("gw_dev", lambda n, c, sp, spg, ss, w, h, dp, dpg, ds: L.prl_hip_gray_world_batch_device(n, 2.5, 1, sp, spg, ss, w, h, dp, dpg, ds, None), True, False),
            ("gw_host", lambda n, c, sp, spg, ss, w, h, dp, dpg, ds: L.prl_hip_gray_world_host(2.5, 1, sp, ss, w, h, dp, ds), False, False),
        ]

    for name, fn, device, has_c in entries(None):
        def f(n=1, c=3, sp=s, spg=256 * 60, ss=256, w=64, h=60, dp=d, dpg=256 * 60, ds=256):
            return fn(n, c, sp, spg, ss, w, h, dp, dpg, ds)

        assert f(w=0) == E and f(h=-1) == E and f(w=0, c=9, sp=None) == E, name                       # empty first
        if has_c:
            bad = (0, 5, -1) + ((2,) if name.startswith("clean") else ())
            for c in bad:
                assert f(c=c) == CH and f(c=c, sp=None) == CH and f(c=c, ss=1) == CH, (name, c)     # channels before the rest
            if not device or no_gpu:
                for c in (1, 3, 4) + (() if name.startswith("clean") else (2,)):
                    assert f(c=c) not in (E, CH, A), (name, c)
        assert f(sp=None) == A and f(dp=None) == A, name
        assert f(ss=64 * 3 - 1) == A and f(ds=64 * 3 - 1) == A, name
        if not device or no_gpu:
            assert f(ss=64 * 3, ds=64 * 3) != A, name
        assert f(w=32769, ss=1 << 18, ds=1 << 18) == A and f(h=32769) == A, name
        if device:
            assert f(n=-1) == A and f(n=0) == _capi.PRL_OK, name
            assert f(n=2, dp=s + 64, spg=192 * 60, dpg=192 * 60) == A, name                           # overlap
            assert f(dp=s, ds=192) == A, name                                                          # same base, other strides
            if no_gpu:
                assert f(dp=s) not in (E, CH, A), name                                                 # in place
            if name in ("gamma_dev", "clean_dev"):
                assert f(c=4, dp=s) == A, name                                                         # 4 -> 3 channels: never in place
    # the histogram has no destination image; its bins and the look-up's tables must be there
    def hist(n=1, c=3, sp=s, spg=256 * 60, ss=256, w=64, h=60, out=x):
        return L.prl_hip_histogram_batch_device(n, c, sp, spg, ss, w, h, out, None)

    assert hist(w=0) == E and hist(c=0) == CH and hist(c=5, sp=None) == CH and hist(sp=None) == A and hist(out=None) == A
    assert hist(ss=191) == A and hist(n=-1) == A and hist(n=0) == _capi.PRL_OK and hist(h=32769) == A
    assert not no_gpu or hist(c=2) not in (E, CH, A)
    assert L.prl_hip_lut_batch_device(1, 3, None, 0, s, 256 * 60, 256, 64, 60, d, 256 * 60, 256, None) == A
    assert src.max() == 0 and dst.max() == 0 and aux.max() == 0


def test_valid_call_without_a_device(prl):
    import torch

    from prlib_amd import _capi

    if torch.cuda.is_available():
        pytest.skip("a device is present; the no-device behaviour is checked on the CPU box")
    img = np.zeros((60, 64, 3), np.uint8)
    for call in (lambda: prl.gammaCorrection(img, 0.5, 2.2), lambda: prl.gammaCorrection(img[:, :, 0], 1.0, 2.2),
                 lambda: prl.simpleWhiteBalance(img, 0.01), lambda: prl.grayWorldWhiteBalance(img, 1.0, False),
                 lambda: prl.grayWorldWhiteBalance(img, 2.5, True), lambda: prl.cleanBackgroundToWhite(img),
                 lambda: prl.cleanBackgroundToWhite(img[:, :, 0])):
        with pytest.raises(_capi.PrlError) as e:
            call()
        assert e.value.status == _capi.PRL_ERR_NO_DEVICE
    for call in (lambda: prl.simpleWhiteBalance(img[:, :, :2], 0.01), lambda: prl.grayWorldWhiteBalance(img[:, :, 0], 1.0, False),
                 lambda: prl.cleanBackgroundToWhite(img[:, :, :2])):
        with pytest.raises(_capi.PrlError) as e:
            call()
        assert e.value.status == _capi.PRL_ERR_BAD_CHANNELS


# ---- the C++ drop-in ---------------------------------------------------------------------------------------------------------------

def build_dropin(out_dir):
    """g++ of tests/cpp/test_tone_dropin.cpp + prl_host.cpp, with only -I include/prl for the drop-in headers."""
    exe = os.path.join(out_dir, "test_tone_dropin")
    flags = []
    for pc in ("opencv4", "opencv"):
        r = subprocess.run(["pkg-config", "--cflags", "--libs", pc], capture_output=True, text=True) if shutil.which("pkg-config") else None
        if r is not None and r.returncode == 0:
            flags = r.stdout.split()
            break
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include", "prl"),
           os.path.join(ROOT, "tests", "cpp", "test_tone_dropin.cpp"), os.path.join(ROOT, "prlib_amd", "csrc", "prl", "prl_host.cpp"),
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
    assert r.returncode == 0 and "tone dropin cpu: OK" in r.stdout, r.stdout + r.stderr
