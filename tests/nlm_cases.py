"""What tests/test_nlm_cpu.py and tests/test_nlm_gpu.py share: the test-hooks entries of nlm.hip (prl_hip_internal_nlm_plan /
_nlm_variant / _lab_convert), the strengths that put the weight table's non-zero length on an edge of launch_nlm's rule, and the pages.

The kernel launch_nlm takes follows from n_lut, the number of leading table entries that may be non-zero:
    1 / 2 channels   n_lut <= 639: 4-byte elements, table in LDS (variant 0; 1 = the same with the table read from memory, hooks only)
                     n_lut <= 1024: 8-byte elements, table in LDS (2);  else 8-byte elements, table from memory (3)
    3 channels       n_lut <= 1024: k_nlm<3, true> (4);  else k_nlm<3, false> (5)
"""
import ctypes as C

import numpy as np

XL_LDS, XL_MEM, Y_LDS, Y_MEM, C3_LDS, C3_MEM = range(6)
LUT_MAX_XL, LUT_MAX = 639, 1024          # kLutMaxXL, kLutMax of nlm.hip
EDGES = (LUT_MAX_XL, LUT_MAX_XL + 1, LUT_MAX, LUT_MAX + 1)
SLOT_ENTRIES = 512 * 1024 // 4           # kLutSlot: the table and its closing zero must fit
H_STEP = 1.0 / 4096                      # every k / 4096 below 2^12 is exact in float32

# strengths with exactly these table lengths where this file was written (float32-exact); the tests assert the oracle's length
# before they use one, so another libm's exp() fails loudly instead of testing beside the edge
RECORDED = {1: {639: 11.000244140625, 640: 11.0087890625, 1024: 13.92919921875, 1025: 13.93603515625},
            2: {639: 7.7783203125, 640: 7.784423828125, 1024: 9.849365234375, 1025: 9.854248046875},
            3: {1024: 8.0419921875, 1025: 8.0458984375}}

_HOOKS = None


def hooks():
    """libprlib_hip_testhooks.so with the argument types of the three entries (loading it makes no GPU call)."""
    global _HOOKS
    if _HOOKS is None:
        from prlib_amd import _capi

        L = C.CDLL(_capi.HOOKS_LIB_PATH)
        i, f, vp, sz, ip = C.c_int, C.c_float, C.c_void_p, C.c_size_t, C.POINTER(C.c_int)
        L.prl_hip_internal_nlm_plan.argtypes = [i, f, i, i, ip, ip, vp, i]
        planes = [i, i, f, vp, sz, sz, i, i, vp, sz, sz, vp]
        L.prl_hip_internal_nlm_variant.argtypes = [i] + planes
        L.prl_hip_nlm_planes_device.argtypes = planes
        L.prl_hip_denoise_batch_device.argtypes = planes
        L.prl_hip_internal_lab_convert.argtypes = [i, i, i, vp, sz, sz, i, i, vp, vp, vp]
        L.prl_hip_set_device.argtypes = [i]
        _HOOKS = L
    return _HOOKS


def plan(channels, h, knob_xl=3, knob_glut=0, cap=1 << 18):
    """(status, n_lut, variant, table[:n_lut]) of prl_hip_internal_nlm_plan; the knobs' defaults are the product's values."""
    lut = np.full(cap, -1, np.int32)
    n, v = C.c_int(-1), C.c_int(-1)
    st = hooks().prl_hip_internal_nlm_plan(channels, h, knob_xl, knob_glut, C.byref(n), C.byref(v), lut.ctypes.data, cap)
    return st, n.value, v.value, lut[:max(0, min(n.value, cap))].copy()


def oracle_n_lut(oracle, channels, h):
    """Length of the oracle's table up to its last non-zero weight."""
    nz = np.nonzero(oracle.nlm_weights(channels, h))[0]
    return int(nz[-1]) + 1 if len(nz) else 0


def first_strength_with(oracle, channels, length, k_hi=1 << 22):
    """The smallest h = k / 4096 whose oracle table has at least `length` leading non-zero entries (the length never shrinks as
    h grows: bisection over k)."""
    lo, hi = 0, k_hi          # length(lo) < length <= length(hi)
    assert oracle_n_lut(oracle, channels, hi * H_STEP) >= length > oracle_n_lut(oracle, channels, 0.0)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if oracle_n_lut(oracle, channels, mid * H_STEP) >= length:
            hi = mid
        else:
            lo = mid
    h = hi * H_STEP
    assert float(np.float32(h)) == h
    return h


_EDGE_CACHE = {}


def edge_strength(oracle, channels, length):
    """A float32-exact strength whose table has exactly `length` leading non-zero entries, checked against the oracle."""
    key = (channels, length)
    if key not in _EDGE_CACHE:
        h = first_strength_with(oracle, channels, length)
        got = oracle_n_lut(oracle, channels, h)
        assert got == length, f"{channels} channels: no h = k/4096 gives a table of {length} entries (first at least as long: h = {h}, {got})"
        _EDGE_CACHE[key] = h
    return _EDGE_CACHE[key]


def expected_variant(channels, n_lut, knob_xl=3, knob_glut=0):
    """The rule as the header of this file states it, written out again."""
    if channels == 3:
        return C3_LDS if n_lut <= LUT_MAX else C3_MEM
    bit = 1 << (channels - 1)
    if n_lut <= LUT_MAX_XL and knob_xl & bit:
        return XL_MEM if knob_glut & bit else XL_LDS
    return Y_LDS if n_lut <= LUT_MAX else Y_MEM


def all_colours():
    """4096 x 4096 x 3: every byte triple once; triple i = (i & 255, i >> 8 & 255, i >> 16) sits at row i >> 12, column i & 4095."""
    v = np.arange(1 << 24, dtype="<u4").view(np.uint8).reshape(-1, 4)[:, :3]
    return np.ascontiguousarray(v).reshape(4096, 4096, 3)


# ---- pages ------------------------------------------------------------------------------------------------------------

# a workgroup's tile is 64 x 32 outputs (width x height), a wavefront 8 rows, the reflect-101 halo 13 wide; shapes are rows x columns
SHAPES = [(45, 70), (32, 64), (33, 65), (9, 128), (1, 1), (1, 40), (40, 1), (2, 2), (5, 3), (13, 14), (14, 13)]


def _noisy(shape, seed, sigma, channels):
    from prlib_amd import synth

    rng = np.random.default_rng(seed)
    h, w = shape
    base = synth.page_numpy(h, w, index=seed).astype(np.float64)
    return np.clip(np.rint(base[:, :, None] + rng.normal(0, sigma, (h, w, channels))), 0, 255).astype(np.uint8)


def pages(shape, channels, seed=0):
    """[(name, H x W x C page)]: the contents every variant filters at every shape, as one batch."""
    h, w = shape
    rng = np.random.default_rng(1000 * h + w + 7 * channels + seed)
    yy, xx = np.mgrid[0:h, 0:w]
    noisy = _noisy(shape, seed + 1, 8.0, channels)
    rand = rng.integers(0, 256, (h, w, channels), dtype=np.uint8)                    # nearly every offset clamps to the closing zero
    flat = np.full((h, w, channels), 255, np.uint8)                                  # the estimate reaches 19096 * 441 * 255 < 2^31
    checker = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], channels, 2)   # full weight or the closing zero
    # two levels, the edge through a tile seam: column 64 and row 32 where the page has them, else its middle
    ex, ey = (64 if w > 64 else w // 2), (32 if h > 32 else h // 2)
    step = np.repeat(np.where((xx >= ex) ^ (yy >= ey), 150, 110).astype(np.uint8)[:, :, None], channels, 2)
    step[:, :, channels - 1] += 3
    one = noisy.copy()                                                               # `noisy` but for one sample at (31, 63)
    one[min(31, h - 1), min(63, w - 1), channels - 1] ^= 0x80
    return [("noisy", noisy), ("random", rand), ("flat255", flat), ("checker", checker), ("step", step), ("one-pixel", one)]
