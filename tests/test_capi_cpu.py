"""CPU-side checks of the drop-in boundary: libprlib_hip.so loads, exports every symbol the public
header declares, validates arguments like the reference, and fails loudly without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbols_are_exported(prl):
    from prlib_amd import _capi

    header = open(os.path.join(ROOT, "include", "prl_hip.h")).read()
    declared = set(re.findall(r"\b(prl_hip_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations found in include/prl_hip.h"
    assert declared == set(_capi.EXPORTED_SYMBOLS), declared ^ set(_capi.EXPORTED_SYMBOLS)
    L = _capi.lib()
    for name in declared:
        assert hasattr(L, name), f"{name} is declared in the header but not exported"
    assert L.prl_hip_abi_version() == 4


def test_struct_layout_matches_header(prl):
    from prlib_amd import _capi

    assert C.sizeof(_capi.BinarizeParams) == 56
    assert _capi.BinarizeParams.k.offset == 8 and _capi.BinarizeParams.feng_alpha1.offset == 24
    assert C.sizeof(_capi.BinarizeGeometry) == 24
    assert C.sizeof(_capi.BinarizeStats) == 64
    from prlib_amd.deskew import DeskewStats   # prl_deskew_stats: 8 x 64-bit

    assert C.sizeof(DeskewStats) == 64 and DeskewStats.min_page_headroom.offset == 48


def test_defaults_are_the_reference_headers(prl):
    # binarizeSauvola.h:43-47, binarizeNiblack.h:43-47, binarizeWolfJolion.h:43-47, binarizeNICK.h:43-47, binarizeFeng.h:46-53
    for m in (prl.SAUVOLA, prl.NIBLACK, prl.WOLFJOLION):
        p = prl.default_params(m)
        assert (p.window_size, p.k, p.morph_iterations) == (101, 0.01, 2)
    p = prl.default_params(prl.NICK)
    assert (p.window_size, p.k, p.morph_iterations) == (21, -0.01, 0)
    p = prl.default_params(prl.FENG)
    assert (p.window_size, p.feng_alpha1, p.feng_k1, p.feng_k2, p.feng_gamma, p.morph_iterations) == (21, 0.75, 0.2, 0.03, 2.0, 2)


@pytest.mark.parametrize("method", range(5))
@pytest.mark.parametrize("w,h,win", [(4096, 4096, 31), (2480, 3508, 101), (100, 100, 101), (60, 80, 101), (33, 200, 15)])
def test_geometry_agrees_with_oracle(prl, oracle, method, w, h, win):
    po = oracle.make_params(method, win, 0.1, 0)
    st_o, go = oracle.geometry(po, w, h)
    pp = prl.make_params(method, win, 0.1, 0)
    from prlib_amd import _capi

    g = _capi.BinarizeGeometry()
    st_p = _capi.lib().prl_hip_binarize_geometry(C.byref(pp), w, h, C.byref(g))
    assert st_p == st_o
    assert (g.w, g.half, g.padded_w, g.padded_h, g.out_w, g.out_h) == (go.w, go.half, go.padded_w, go.padded_h, go.out_w, go.out_h)


def test_reference_quirks_in_geometry(prl):
    # Sauvola/Niblack output (W-1)x(H-1); Wolf/NICK/Feng (W-w)x(H-w)
    g = prl.geometry(prl.make_params(prl.SAUVOLA, 31), 4096, 4096)
    assert (g.out_w, g.out_h, g.padded_w) == (4095, 4095, 4126)
    g = prl.geometry(prl.make_params(prl.NICK, 21), 2480, 3508)
    assert (g.out_w, g.out_h) == (2459, 3487)
    # clamped even window keeps the page size (Appendix D.7)
    g = prl.geometry(prl.make_params(prl.NIBLACK, 101), 100, 100)
    assert (g.w, g.half, g.out_w, g.out_h) == (100, 50, 100, 100)


def test_errors_without_touching_a_device(prl):
    from prlib_amd import _capi

    page = np.zeros((50, 60), np.uint8)
    with pytest.raises(ValueError, match="Window size must satisfy"):
        prl.binarizeSauvola(page, 30)
    with pytest.raises(ValueError, match="empty"):
        prl.binarizeNiblack(np.zeros((0, 0), np.uint8))
    with pytest.raises(_capi.PrlError) as e:
        prl.binarizeFeng(page, 51)
    assert e.value.status == _capi.PRL_ERR_EMPTY_RECT


def test_no_device_means_loud_failure_not_cpu_fallback(prl):
    import torch
    from prlib_amd import _capi

    if torch.cuda.is_available():
        pytest.skip("device present")
    page = np.full((64, 64), 200, np.uint8)
    with pytest.raises(_capi.PrlError) as e:
        prl.binarizeSauvola(page, 15, 0.34, 0)
    assert e.value.status == _capi.PRL_ERR_NO_DEVICE
    with pytest.raises(_capi.PrlError) as e:
        prl.denoise(np.zeros((32, 32, 3), np.uint8))
    assert e.value.status == _capi.PRL_ERR_NO_DEVICE


def test_entry_statuses_without_a_device(prl):
    """The *_host entries, the batch entries on the shared device workspace and the deskew / rotate / find_angle / houghp entries
    check their arguments in a fixed order before they look for a device: one row per rejection class (a few with two faults pin which check comes first), then valid calls,
    which fail with PRL_ERR_NO_DEVICE here (those rows are skipped where a device is visible).  No row reaches the buffers."""
    import torch
    from prlib_amd import _capi as E

    L = E.lib()
    has_device = torch.cuda.is_available()
    buf = np.zeros(1 << 16, np.uint8)
    s, d = buf.ctypes.data, buf.ctypes.data + (1 << 15)
    angles = (C.c_double * 2)(1.0, -2.0)
    ang = C.addressof(angles)
    wh, nseg = (C.c_int32 * 2)(0, 0), (C.c_int32 * 2)(0, 0)   # results of the deskew / find_angle entries: never the page buffer
    whp = C.addressof(wh)
    out_w, out_h, one_angle, one_nseg = C.c_int(0), C.c_int(0), C.c_double(0.0), C.c_int32(0)
    sauvola = prl.make_params(prl.SAUVOLA, 3)   # 12 x 8 page: 11 x 7 output, 14 x 10 padded
    even = prl.make_params(prl.SAUVOLA, 4)
    bad_method = prl.make_params(prl.SAUVOLA, 3)
    bad_method.method = 5
    feng51 = prl.make_params(prl.FENG, 51)   # 12 x 8 page: the window clamps to 8, leaving no output rows
    ps = 384   # page stride of the batch entries
    OK, EMPTY, WIN, CH, RECT, ARG, NODEV = (E.PRL_OK, E.PRL_ERR_EMPTY, E.PRL_ERR_BAD_WINDOW, E.PRL_ERR_BAD_CHANNELS,
                                            E.PRL_ERR_EMPTY_RECT, E.PRL_ERR_BAD_ARG, E.PRL_ERR_NO_DEVICE)
    # (entry, arguments in order, [(changed arguments, status), ...])
    table = [
        (L.prl_hip_binarize_host, dict(p=C.byref(sauvola), src=s, ss=12, w=12, h=8, dst=d, ds=12, pad=None, pad_step=0), [
            (dict(p=None), ARG), (dict(w=0), EMPTY), (dict(h=-1), EMPTY), (dict(p=C.byref(even)), WIN),
            (dict(p=C.byref(bad_method)), ARG), (dict(p=C.byref(feng51)), RECT),
            (dict(src=None), ARG), (dict(dst=None), ARG), (dict(ss=11), ARG), (dict(ds=10), ARG), (dict(pad=d, pad_step=13), ARG),
            (dict(w=0, p=C.byref(even)), EMPTY), (dict(p=C.byref(even), src=None), WIN), (dict(p=C.byref(feng51), src=None), RECT),
            (dict(), NODEV), (dict(ds=11), NODEV), (dict(pad=d, pad_step=14), NODEV)]),
        (L.prl_hip_denoise_host, dict(c=3, strength=10.0, src=s, ss=36, w=12, h=8, dst=d, ds=36), [
            (dict(w=0), EMPTY), (dict(h=0), EMPTY), (dict(c=1), CH), (dict(c=2), CH), (dict(c=5), CH),
            (dict(src=None), ARG), (dict(dst=None), ARG), (dict(ss=35), ARG), (dict(ds=35), ARG), (dict(c=4, ds=48), ARG),
            (dict(w=0, c=1), EMPTY), (dict(c=1, src=None), CH),
            (dict(), NODEV), (dict(c=4, ss=48, ds=48), NODEV), (dict(h=65536), NODEV)]),
        (L.prl_hip_thin_host, dict(m=0, src=s, ss=12, w=12, h=8, dst=d, ds=12), [
            (dict(w=0), EMPTY), (dict(h=0), EMPTY), (dict(src=None), ARG), (dict(dst=None), ARG), (dict(ss=11), ARG),
            (dict(ds=11), ARG), (dict(w=0, src=None), EMPTY),
            (dict(), NODEV), (dict(m=1), NODEV), (dict(m=2), NODEV)]),
        (L.prl_hip_bgnorm_host, dict(c=1, src=s, ss=12, w=12, h=8, dst=d, ds=12), [
            (dict(w=0), EMPTY), (dict(h=0), EMPTY), (dict(src=None), EMPTY), (dict(c=0), CH), (dict(c=2), CH), (dict(c=5), CH),
            (dict(dst=None), ARG), (dict(ss=11), ARG), (dict(ds=11), ARG), (dict(c=3, ss=36, ds=35), ARG),
            (dict(c=4, ss=47, ds=36), ARG), (dict(src=None, c=2), EMPTY), (dict(c=2, dst=None), CH),
            (dict(), NODEV), (dict(c=3, ss=36, ds=36), NODEV), (dict(c=4, ss=48, ds=36), NODEV)]),
        (L.prl_hip_binarize_lv_host, dict(wf=1, coeff=1.0, mv=0, gamma=1.0, src=s, ss=36, w=12, h=8, dst=d, ds=12), [
            (dict(w=0), EMPTY), (dict(h=0), EMPTY), (dict(src=None), EMPTY), (dict(dst=None), ARG), (dict(ss=35), ARG),
            (dict(ds=11), ARG), (dict(src=None, dst=None), EMPTY),
            (dict(), NODEV), (dict(wf=0), NODEV)]),
        (L.prl_hip_bgnorm_batch_device, dict(n=1, c=1, src=s, sps=ps, ss=12, w=12, h=8, dst=d, dps=ps, ds=12, stream=None), [
            (dict(w=0), EMPTY), (dict(c=2), CH), (dict(n=-1), ARG), (dict(src=None), ARG), (dict(dst=None), ARG),
            (dict(ss=11), ARG), (dict(ds=11), ARG), (dict(c=3, ss=36, ds=35), ARG), (dict(h=65536), ARG),
            (dict(w=40951, ss=40951, ds=40951), ARG), (dict(n=0), OK),
            (dict(w=0, c=2), EMPTY), (dict(c=2, n=-1), CH), (dict(n=0, h=65536), ARG),
            (dict(), NODEV), (dict(c=4, ss=48, ds=36), NODEV)]),
        (L.prl_hip_binarize_lv_batch_device, dict(n=1, wf=1, coeff=1.0, mv=0, gamma=1.0, src=s, sps=ps, ss=36, w=12, h=8, dst=d,
                                                  dps=ps, ds=12, stream=None), [
            (dict(w=0), EMPTY), (dict(n=-1), ARG), (dict(src=None), ARG), (dict(dst=None), ARG), (dict(ss=35), ARG),
            (dict(ds=11), ARG), (dict(h=1048561), ARG), (dict(n=0), OK), (dict(w=0, n=-1), EMPTY), (dict(n=0, h=1048561), ARG),
            (dict(w=0, src=None), EMPTY), (dict(), NODEV), (dict(wf=0), NODEV), (dict(h=1048560), NODEV)]),
        (L.prl_hip_thin_batch_device, dict(m=0, n=1, src=s, sps=ps, ss=12, w=12, h=8, dst=d, dps=ps, ds=12, stream=None), [
            (dict(w=0), EMPTY), (dict(m=2), ARG), (dict(m=-1), ARG), (dict(n=-1), ARG), (dict(src=None), ARG),
            (dict(dst=None), ARG), (dict(ss=11), ARG), (dict(ds=11), ARG), (dict(n=0), OK),
            (dict(w=0, m=2), EMPTY), (dict(n=0, m=2), ARG),
            (dict(), NODEV), (dict(m=1), NODEV), (dict(n=32769), NODEV),
            (dict(w=1 << 21, ss=1 << 21, ds=1 << 21, h=1 << 15), NODEV)]),   # (a plane of 2^31 words: refused after the device check)
        (L.prl_hip_morph_batch_device, dict(it=2, n=1, src=s, sps=ps, ss=12, w=12, h=8, dst=d, dps=ps, ds=12, stream=None), [
            (dict(w=0), EMPTY), (dict(h=0), EMPTY), (dict(n=-1), ARG), (dict(src=None), ARG), (dict(dst=None), ARG),
            (dict(dst=s), ARG), (dict(ss=11), ARG), (dict(ds=11), ARG), (dict(n=0), OK),
            (dict(w=0, n=-1), EMPTY), (dict(n=0, dst=s), ARG), (dict(n=0, ss=11), ARG),
            (dict(), NODEV), (dict(it=-8), NODEV), (dict(it=0), NODEV), (dict(it=9), NODEV), (dict(it=-12), NODEV),
            (dict(n=32769), NODEV), (dict(it=9, n=32769), NODEV)]),
        (L.prl_hip_nlm_planes_device, dict(n=1, c=1, h_=10.0, src=s, sps=ps, ss=12, w=12, h=8, dst=d, dps=ps, ds=12, stream=None), [
            (dict(w=0), EMPTY), (dict(c=0), CH), (dict(c=4), CH), (dict(n=-1), ARG), (dict(src=None), ARG), (dict(dst=None), ARG),
            (dict(dst=s), ARG), (dict(ss=11), ARG), (dict(ds=11), ARG), (dict(c=2, ss=23, ds=24), ARG), (dict(n=0), OK),
            (dict(w=0, c=0), EMPTY), (dict(c=0, src=None), CH), (dict(n=0, dst=s), ARG),
            (dict(), NODEV), (dict(c=2, ss=24, ds=24), NODEV), (dict(c=3, ss=36, ds=36), NODEV)]),
        (L.prl_hip_denoise_batch_device, dict(n=1, c=3, strength=10.0, src=s, sps=ps, ss=36, w=12, h=8, dst=d, dps=ps, ds=36,
                                              stream=None), [
            (dict(w=0), EMPTY), (dict(c=1), CH), (dict(c=2), CH), (dict(c=5), CH), (dict(n=-1), ARG), (dict(src=None), ARG),
            (dict(dst=None), ARG), (dict(ss=35), ARG), (dict(ds=35), ARG), (dict(c=4, ss=48), ARG), (dict(h=65536), ARG),
            (dict(n=0), OK), (dict(w=0, c=1), EMPTY), (dict(c=1, n=-1), CH), (dict(n=0, h=65536), OK),
            (dict(), NODEV), (dict(c=4, ss=48, ds=48), NODEV), (dict(n=65536), NODEV)]),
        (L.prl_hip_rotate_batch_device, dict(n=1, c=1, ang=ang, src=s, sps=ps, ss=12, w=12, h=8, dst=d, dps=ps, ds=12, stream=None), [
            (dict(w=0), EMPTY), (dict(c=0), CH), (dict(c=5), CH), (dict(n=-1), ARG), (dict(ang=None), ARG), (dict(src=None), ARG),
            (dict(dst=None), ARG), (dict(dst=s), ARG), (dict(ss=11), ARG), (dict(w=32768, ss=32768), ARG), (dict(h=32768), ARG),
            (dict(n=0), OK), (dict(w=0, c=0), EMPTY), (dict(c=0, ang=None), CH), (dict(n=0, h=32768), ARG),
            (dict(), NODEV), (dict(c=4, ss=48, ds=48), NODEV), (dict(ds=1), NODEV)]),   # (dst_step: checked per chunk, after the device)
        # deskew: a page's result may be max(w, h) wide, so that side bounds dst_step
        (L.prl_hip_deskew_batch_device, dict(n=1, c=1, src=s, sps=ps, ss=12, w=12, h=8, dst=d, dps=ps, ds=12, wh=whp, ang=None,
                                             stream=None), [
            (dict(w=0), EMPTY), (dict(h=0), EMPTY), (dict(c=0), CH), (dict(c=2), CH), (dict(c=5), CH), (dict(n=-1), ARG),
            (dict(src=None), ARG), (dict(dst=None), ARG), (dict(dst=s), ARG), (dict(wh=None), ARG), (dict(ss=11), ARG),
            (dict(ds=11), ARG), (dict(w=8, h=12, ss=8, ds=11), ARG), (dict(h=32768, ds=32768), ARG),
            (dict(w=32768, ss=32768, ds=32768), ARG), (dict(n=0), OK),
            (dict(w=0, c=2), EMPTY), (dict(c=2, n=-1), CH), (dict(c=2, wh=None), CH), (dict(n=0, dst=None), ARG),
            (dict(n=0, h=32768, ds=32768), ARG),
            (dict(), NODEV), (dict(ang=ang), NODEV), (dict(c=3, ss=36, ds=36), NODEV), (dict(c=4, ss=48, ds=48), NODEV),
            (dict(w=8, h=12, ss=8), NODEV), (dict(h=32767, ds=32767), NODEV)]),
        # (dst_step of the two *_host entries below: compared with the result's width after the device stage; their sides are
        # the device stage's to refuse)
        (L.prl_hip_deskew_host, dict(c=1, src=s, ss=12, w=12, h=8, dst=d, ds=12, ow=C.byref(out_w), oh=C.byref(out_h), angle=None), [
            (dict(w=0), EMPTY), (dict(h=0), EMPTY), (dict(src=None), EMPTY), (dict(c=0), CH), (dict(c=2), CH), (dict(c=5), CH),
            (dict(dst=None), ARG), (dict(ow=None), ARG), (dict(oh=None), ARG), (dict(ss=11), ARG),
            (dict(src=None, c=2), EMPTY), (dict(c=2, dst=None), CH),
            (dict(), NODEV), (dict(ds=1), NODEV), (dict(angle=C.byref(one_angle)), NODEV), (dict(c=3, ss=36, ds=36), NODEV),
            (dict(c=4, ss=48, ds=48), NODEV), (dict(h=32768), NODEV)]),
        (L.prl_hip_rotate_host, dict(c=1, angle=3.0, src=s, ss=12, w=12, h=8, dst=d, ds=12), [
            (dict(w=0), EMPTY), (dict(h=0), EMPTY), (dict(src=None), EMPTY), (dict(c=0), CH), (dict(c=5), CH),
            (dict(dst=None), ARG), (dict(ss=11), ARG), (dict(c=3, ss=35), ARG),
            (dict(src=None, c=0), EMPTY), (dict(c=0, dst=None), CH),
            (dict(), NODEV), (dict(ds=1), NODEV), (dict(angle=90.0), NODEV), (dict(c=2, ss=24, ds=24), NODEV),
            (dict(c=4, ss=48, ds=48), NODEV), (dict(h=32768), NODEV)]),
        (L.prl_hip_find_angle_batch_device, dict(n=1, src=s, sps=ps, ss=12, w=12, h=8, ang=ang, nseg=None, stream=None), [
            (dict(w=0), EMPTY), (dict(h=0), EMPTY), (dict(n=-1), ARG), (dict(src=None), ARG), (dict(ang=None), ARG),
            (dict(ss=11), ARG), (dict(h=32768), ARG), (dict(w=32768, ss=32768), ARG), (dict(n=0), OK),
            (dict(w=0, n=-1), EMPTY), (dict(w=0, src=None), EMPTY), (dict(n=0, ang=None), ARG), (dict(n=0, h=32768), ARG),
            (dict(), NODEV), (dict(nseg=C.addressof(nseg)), NODEV), (dict(h=32767), NODEV)]),
        (L.prl_hip_find_angle_host, dict(src=s, ss=12, w=12, h=8, ang=C.byref(one_angle), nseg=None), [
            (dict(w=0), EMPTY), (dict(h=0), EMPTY), (dict(src=None), EMPTY), (dict(ang=None), ARG), (dict(ss=11), ARG),
            (dict(h=32768), ARG), (dict(w=32768, ss=32768), ARG), (dict(src=None, ang=None), EMPTY), (dict(w=0, ss=0, ang=None), EMPTY),
            (dict(), NODEV), (dict(nseg=C.byref(one_nseg)), NODEV), (dict(h=32767), NODEV)]),
        (L.prl_hip_houghp_device, dict(src=s, ss=12, w=12, h=8, thr=10, ll=5, gap=2, lines=d, cap=4, nl=C.byref(out_w), stream=None), [
            (dict(w=0), EMPTY), (dict(h=0), EMPTY), (dict(src=None), ARG), (dict(nl=None), ARG), (dict(lines=None), ARG),
            (dict(ss=11), ARG), (dict(h=32768), ARG), (dict(w=32768, ss=32768), ARG),
            (dict(w=0, src=None), EMPTY), (dict(h=0, nl=None), EMPTY),
            (dict(), NODEV), (dict(lines=None, cap=0), NODEV), (dict(lines=None, cap=-1), NODEV), (dict(thr=0, ll=0, gap=-1), NODEV),
            (dict(h=32767), NODEV)]),
    ]
    wrong = []
    for fn, args, cases in table:
        for change, want in cases:
            if want == NODEV and has_device:
                continue
            assert set(change) <= set(args), (fn.__name__, change)
            got = fn(*{**args, **change}.values())
            if got != want:
                wrong.append((fn.__name__, change, got, want))
    assert not wrong, wrong
    assert not buf.any()


def test_product_does_not_reference_the_oracle():
    """The oracle is test infrastructure: nothing under prlib_amd/ may import, include or link it."""
    bad = []
    for base, _, files in os.walk(os.path.join(ROOT, "prlib_amd")):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".cpp", "Makefile")):
                txt = open(os.path.join(base, f), errors="ignore").read()
                if re.search(r"#include\s+[\"<][^\">]*oracle|from oracle|import oracle|lprl_oracle|prl_oracle_", txt):
                    bad.append(os.path.join(base, f))
    assert not bad, bad


def test_library_exports_exactly_the_header():
    """libprlib_hip.so exports the functions include/prl_hip.h declares and nothing else (the reference marks exactly its public
    functions CV_EXPORTS: binarizeSauvola.h:43); the test-hooks build adds the seven prl_hip_internal_* entries; both carry the ABI
    version in their SONAME.  The linker maps are generated from the header (tools/gen_export_map.py)."""
    import shutil
    import subprocess
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_export_map as gem

    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_export_map.py"), "--check"]).returncode == 0
    declared = gem.header_functions()
    assert len(declared) == len(set(declared)) >= 56
    from prlib_amd import _capi

    assert sorted(_capi.EXPORTED_SYMBOLS) == sorted(declared)
    if not shutil.which("nm") or not shutil.which("readelf"):
        pytest.skip("binutils not installed")
    abi = re.search(r"#define PRL_HIP_ABI_VERSION (\d+)", open(os.path.join(ROOT, "include", "prl_hip.h")).read()).group(1)
    for path, extra, soname in ((_capi.LIB_PATH, [], "libprlib_hip.so." + abi),
                                (_capi.HOOKS_LIB_PATH, gem.INTERNAL, "libprlib_hip_testhooks.so." + abi)):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        got = sorted(ln.split()[-1].split("@")[0] for ln in out.splitlines() if ln.split() and ln.split()[-2] in "TtWwDdBbRr")
        got = [g for g in got if g != "PRLIB_HIP_" + abi]   # (the version node itself is an absolute symbol)
        assert got == sorted(declared + extra), (path, sorted(set(got) ^ set(declared + extra)))
        dyn = subprocess.run(["readelf", "-d", path], capture_output=True, text=True, check=True).stdout
        assert f"[{soname}]" in dyn, dyn


def test_cmake_install_tree_builds_the_dropin_sample(tmp_path):
    """The CMake route (what a PRLib maintainer uses: the reference builds with CMake, CMakeLists.txt:23-33 there): configure, build,
    install into a scratch prefix; the installed library exports the header's functions only and carries its SONAME; a caller that
    keeps the reference's #include lines (tests/cpp/test_dropin_sample.cpp) builds against the INSTALLED tree alone."""
    import shutil
    import subprocess

    if not shutil.which("cmake") or not os.path.exists("/opt/rocm/bin/hipcc") or not shutil.which("g++"):
        pytest.skip("cmake / hipcc / g++ not installed")
    b, prefix = str(tmp_path / "b"), str(tmp_path / "prefix")
    for cmd in (["cmake", "-S", ROOT, "-B", b, "-DCMAKE_INSTALL_PREFIX=" + prefix], ["cmake", "--build", b, "-j", str(min(8, os.cpu_count() or 1))],
                ["cmake", "--install", b]):
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, " ".join(cmd) + "\n" + r.stdout[-3000:] + r.stderr[-3000:]
    abi = re.search(r"#define PRL_HIP_ABI_VERSION (\d+)", open(os.path.join(ROOT, "include", "prl_hip.h")).read()).group(1)
    so = os.path.join(prefix, "lib", "libprlib_hip.so." + abi)
    assert os.path.exists(so) and os.path.exists(os.path.join(prefix, "lib", "libprlib_hip_host.a"))
    assert os.path.exists(os.path.join(prefix, "lib", "cmake", "prlib_hip", "prlib_hipConfig.cmake"))
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    names = sorted(ln.split()[-1].split("@")[0] for ln in out.splitlines() if ln.split() and ln.split()[-2] in "TtWw")
    from prlib_amd import _capi

    assert names == sorted(_capi.EXPORTED_SYMBOLS)
    from oracle import capi as oc

    oc.build()   # (the sample checks itself against the oracle when it runs on a GPU box; here it only has to build)
    exe = str(tmp_path / "dropin")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I" + os.path.join(prefix, "include", "prl"),
                        os.path.join(ROOT, "tests", "cpp", "test_dropin_sample.cpp"), "-L" + os.path.join(prefix, "lib"), "-lprlib_hip_host", "-lprlib_hip",
                        "-L" + os.path.join(ROOT, "oracle"), "-lprl_oracle", "-Wl,-rpath," + os.path.join(prefix, "lib"), "-Wl,-rpath," + os.path.join(ROOT, "oracle"),
                        "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and os.path.exists(exe), r.stderr[-3000:]
