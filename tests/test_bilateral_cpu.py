"""cv::bilateralFilter on 8-bit planes without a device: the radius, the tap order and both tables of prl_hip_bilateral_tables against
the restatement tests/fbcitb_ref.py, the refusals, self-checks of the restatement (an exact rounding tie, a denormal weight), and
the sensitivity of the inputs the GPU tests use: a fused multiply-add, a reciprocal multiply and the centre-first form each change
at least one byte on one of them.  bilateral.h's own loop is held to the same bytes by tests/cpp/test_fbcitb.cpp
(tests/test_fbcitb_cpu.py runs it under the sanitizers).  Every comparison is an equality."""
import ctypes

import numpy as np
import pytest

import fbcitb_ref as fr

SYMBOLS = ("prl_hip_bilateral_tables", "prl_hip_bilateral_filter_batch_device", "prl_hip_bilateral_filter_host")
# (generator, seed) of 37 x 53 planes at d = 5, sigmas 150 / 150 (binarizeFBCITB's defaults), found by a search over seeds:
# the first changes under "fused" and "centre_first", the second under "reciprocal" and "centre_first"
SENSITIVE = (("noise", 63), ("smooth", 108))


def sensitive_page(gen, seed):
    return fr.noise(37, 53, 1, seed) if gen == "noise" else fr.smooth_noise(37, 53, seed)


@pytest.mark.parametrize("d, sigma_space, radius", [(-1, 2.0, 3), (0, 3.0, 4), (0, 1.0, 2), (0, 0.0, 2), (-1, 0.2, 1), (3, 9.0, 1), (4, 9.0, 2),
                                                    (5, 9.0, 2), (9, 9.0, 4), (31, 9.0, 15), (1, 9.0, 1), (2, 9.0, 1)])
def test_radius_and_side(prl, d, sigma_space, radius):
    """d <= 0 takes cvRound(1.5 sigmaSpace) with ties to even (1.5 * 3 = 4.5 -> 4, 1.5 * 1 = 1.5 -> 2), a sigma <= 0 counts as 1"""
    assert fr.bilateral_radius(d, sigma_space) == radius
    got = prl.bilateralTables(d, 25.0, sigma_space)
    assert got[0] == radius and 2 * radius + 1 <= fr.BILATERAL_MAX_SIDE


def test_tap_order_and_count(prl):
    r, offs, space, color = prl.bilateralTables(5, 150.0, 150.0)
    assert r == 2 and len(offs) == 12 and len(space) == 12
    assert offs.tolist() == [[-2, 0], [-1, -1], [-1, 0], [-1, 1], [0, -2], [0, -1], [0, 1], [0, 2], [1, -1], [1, 0], [1, 1], [2, 0]]
    assert prl.bilateralTables(3, 1.0, 1.0)[1].tolist() == [[-1, 0], [0, -1], [0, 1], [1, 0]], "the corners lie outside the disc"
    assert len(prl.bilateralTables(31, 1.0, 1.0)[1]) == fr.BILATERAL_MAX_TAPS == 708


@pytest.mark.parametrize("d", (-1, 0, 3, 4, 5, 9, 31))
def test_tables_equal_the_restatement_byte_for_byte(prl, d):
    for sc, ss in ((150.0, 150.0), (1.0, 1.0), (3.0, 0.7), (0.0, -2.0), (-5.0, 9.9), (fr.TIE_SIGMA_COLOR, fr.TIE_SIGMA_SPACE)):
        if d <= 0 and fr.bilateral_radius(d, ss) > 15:
            continue
        r, taps, space, color = fr.bilateral_tables(d, sc, ss)
        g_r, g_offs, g_space, g_color = prl.bilateralTables(d, sc, ss)
        assert g_r == r and [tuple(o) for o in g_offs.tolist()] == taps, (d, sc, ss)
        assert g_space.tobytes() == space.tobytes() and g_color.tobytes() == color.tobytes(), (d, sc, ss)
        assert color[0] == 1.0 and (np.diff(color) <= 0).all()
    assert prl.bilateralTables(5, 0.0, 0.0)[3].tobytes() == prl.bilateralTables(5, 1.0, 1.0)[3].tobytes(), "both sigma defaults are 1"
    assert prl.bilateralTables(5, 0.0, 0.0)[2].tobytes() == prl.bilateralTables(5, 1.0, 1.0)[2].tobytes()


def test_the_limit_and_the_other_refusals(prl):
    from prlib_amd import _capi

    L = _capi.lib()
    r, n = ctypes.c_int(-1), ctypes.c_int(-1)
    assert L.prl_hip_bilateral_tables(33, 1.0, 1.0, ctypes.byref(r), ctypes.byref(n), None, None, None, None) == _capi.PRL_ERR_BAD_ARG
    assert r.value == 16 and n.value == 0 and b"31" in L.prl_hip_last_error_detail()
    assert L.prl_hip_bilateral_tables(0, 1.0, 11.0, ctypes.byref(r), ctypes.byref(n), None, None, None, None) == _capi.PRL_ERR_BAD_ARG
    assert r.value == 16, "cvRound(16.5) = 16: one above the limit"
    assert L.prl_hip_bilateral_tables(0, 1.0, 1e300, ctypes.byref(r), ctypes.byref(n), None, None, None, None) == _capi.PRL_ERR_BAD_ARG
    assert L.prl_hip_bilateral_tables(31, 1.0, 1.0, ctypes.byref(r), ctypes.byref(n), None, None, None, None) == 0 and n.value == 708
    assert L.prl_hip_bilateral_tables(5, float("nan"), 1.0, ctypes.byref(r), ctypes.byref(n), None, None, None, None) == _capi.PRL_ERR_BAD_ARG
    assert L.prl_hip_bilateral_tables(5, 1.0, float("inf"), ctypes.byref(r), ctypes.byref(n), None, None, None, None) == _capi.PRL_ERR_BAD_ARG
    assert L.prl_hip_bilateral_tables(5, 1.0, 1.0, None, ctypes.byref(n), None, None, None, None) == _capi.PRL_ERR_BAD_ARG
    # the filter entries check before any device is touched, in the documented order
    buf = np.zeros(64, np.uint8)
    p, q = buf.ctypes.data, buf.ctypes.data + 32
    dev = L.prl_hip_bilateral_filter_batch_device
    assert dev(1, 1, 5, 1.0, 1.0, p, 16, 4, 0, 4, q, 16, 4, None) == _capi.PRL_ERR_EMPTY
    assert dev(1, 5, 5, 1.0, 1.0, p, 16, 4, 4, 4, q, 16, 4, None) == _capi.PRL_ERR_BAD_ARG
    assert dev(1, 1, 5, float("nan"), 1.0, p, 16, 4, 4, 4, q, 16, 4, None) == _capi.PRL_ERR_BAD_ARG
    assert dev(1, 1, 33, 1.0, 1.0, p, 16, 4, 4, 4, q, 16, 4, None) == _capi.PRL_ERR_BAD_ARG and b"31" in L.prl_hip_last_error_detail()
    assert dev(1, 1, 5, 1.0, 1.0, None, 16, 4, 4, 4, q, 16, 4, None) == _capi.PRL_ERR_BAD_ARG
    assert dev(-1, 1, 5, 1.0, 1.0, p, 16, 4, 4, 4, q, 16, 4, None) == _capi.PRL_ERR_BAD_ARG
    assert dev(1, 1, 5, 1.0, 1.0, p, 16, 3, 4, 4, q, 16, 4, None) == _capi.PRL_ERR_BAD_ARG
    assert dev(1, 1, 5, 1.0, 1.0, p, 16, 4, 4, 4, p, 16, 4, None) == _capi.PRL_ERR_BAD_ARG, "src == dst is refused"
    assert dev(1, 1, 5, 1.0, 1.0, p, 16, 4, 4, 4, p + 8, 16, 4, None) == _capi.PRL_ERR_BAD_ARG, "any shared byte is"
    assert dev(0, 1, 5, 1.0, 1.0, p, 16, 4, 4, 4, q, 16, 4, None) == 0, "no pages: nothing to do"
    host = L.prl_hip_bilateral_filter_host
    assert host(1, 5, 1.0, 1.0, p, 4, 4, 0, q, 4) == _capi.PRL_ERR_EMPTY
    assert host(1, 33, 1.0, 1.0, p, 4, 4, 4, q, 4) == _capi.PRL_ERR_BAD_ARG
    assert host(1, 5, 1.0, 1.0, p, 4, 4, 4, p, 4) == _capi.PRL_ERR_BAD_ARG


def test_exports(prl):
    from prlib_amd import _capi

    L = _capi.lib()
    for s in SYMBOLS:
        assert s in _capi.EXPORTED_SYMBOLS and hasattr(L, s), s


# ---- the restatement's own checks -------------------------------------------------------------------------------------------------

def test_a_constant_page_filters_to_itself():
    for v in (0, 1, 128, 255):
        for d, sc, ss in ((3, 1.0, 1.0), (9, 150.0, 150.0), (31, 3.0, 20.0)):
            page = np.full((7, 11), v, np.uint8)
            assert np.array_equal(fr.bilateral(page, d, sc, ss), page)


def test_an_exact_tie_and_a_denormal_weight():
    """the tie page: quotients 10.5 and 11.5 in float32 exactly, rounded to even; a weight that is a float32 denormal takes part"""
    page = fr.tie_page()
    out, q = fr.bilateral_plane(page, 3, fr.TIE_SIGMA_COLOR, fr.TIE_SIGMA_SPACE, with_quotient=True)
    assert q.dtype == np.float32 and float(q[2, 2]) == 10.5 and float(q[6, 6]) == 11.5
    assert out[2, 2] == 10 and out[6, 6] == 12, "ties go to the even byte"
    _r, _taps, space, color = fr.bilateral_tables(3, fr.TIE_SIGMA_COLOR, fr.TIE_SIGMA_SPACE)
    tiny = float(np.finfo(np.float32).tiny)
    assert (space == 1.0).all() and color[1] == 0.5 and color[2] == 0.0625
    assert 0.0 < float(color[12]) < tiny and color[13] == 0.0, "2^-144 is a denormal, 2^-169 is zero"
    assert abs(int(page[2, 6]) - int(page[1, 6])) == 12, "and the page meets it"
    c1 = fr.bilateral_tables(5, 1.0, 1.0)[3]
    assert 0.0 < float(c1[14]) < tiny, "(float)exp(-0.5 * 14 * 14) at sigmaColor 1, the header's example"


def test_the_gpu_inputs_are_sensitive():
    """each form that is NOT the rule changes at least one byte on one of the pages the GPU tests filter"""
    changed = set()
    for gen, seed in SENSITIVE:
        page = sensitive_page(gen, seed)
        base = fr.bilateral_plane(page, 5, 150.0, 150.0)
        for variant in ("fused", "reciprocal", "centre_first"):
            if (fr.bilateral_plane(page, 5, 150.0, 150.0, variant) != base).any():
                changed.add(variant)
    assert changed == {"fused", "reciprocal", "centre_first"}, changed


def test_pages_smaller_than_the_radius_fold():
    page = fr.noise(2, 3, 1, 5)
    out = fr.bilateral(page, 9, 50.0, 3.0)
    assert out.shape == page.shape
    one = np.array([[77]], np.uint8)
    assert fr.bilateral(one, 31, 1.0, 1.0)[0, 0] == 77


def test_channels_are_planes_of_their_own():
    page = fr.noise(9, 8, 3, 2)
    got = fr.bilateral(page, 5, 20.0, 2.0)
    for ch in range(3):
        assert np.array_equal(got[:, :, ch], fr.bilateral_plane(np.ascontiguousarray(page[:, :, ch]), 5, 20.0, 2.0))
