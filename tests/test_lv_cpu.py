"""tests/lv_ref.py (the numpy restatement of the local-variance binarizers the GPU tests hold lv.hip against) checked against what
exists, without a device: the second function against the C oracle on every byte, the integer tail against a literal double
loop, and the filtered function put together from the pieces against the C oracle under the project's stated allowance."""
import numpy as np
import pytest

import lv_ref as lr

# the shapes and (coeff, minResultVariance) pairs of test_lv_gpu.test_without_filters_is_bit_exact, and the degenerate pages
NOFILTER_SHAPES = [(200, 260), (97, 131), (33, 40), (8, 32), (1, 1), (257, 65), (530, 777), (18, 3000), (1, 40), (40, 1)]
NOFILTER_PARAMS = [(0.125, 10), (0.5, 25), (0.0, 0)]
# the shapes and (coeff, minResultVariance, gamma) of test_lv_gpu.test_with_filters_within_tolerance
FILTER_SHAPES = [(200, 260), (97, 131), (64, 48), (300, 411), (140, 700)]
FILTER_PARAMS = [(0.125, 25, 2.0), (0.3, 10, 2.0), (0.125, 25, 1.5)]


@pytest.mark.parametrize("shape", NOFILTER_SHAPES, ids=[f"{h}x{w}" for h, w in NOFILTER_SHAPES])
def test_nofilters_equals_the_oracle(oracle, shape):
    for seed in (1, 2):
        page = lr.colour(shape[0], shape[1], seed)
        for coeff, mv in NOFILTER_PARAMS:
            want = oracle.binarize_lv_nofilters(page, coeff, mv)
            got = lr.nofilters(page, coeff, mv)
            assert np.array_equal(got, want), (shape, seed, coeff, mv, int((got != want).sum()))


def test_nofilters_equals_the_oracle_on_uniform_noise(oracle):
    noise = np.random.default_rng(9).integers(0, 256, (80, 90, 3), dtype=np.uint8)
    hits = 0
    for coeff, mv in NOFILTER_PARAMS + [(0.125, 4000), (8.0, 10)]:
        want = oracle.binarize_lv_nofilters(noise, coeff, mv)
        got = lr.nofilters(noise, coeff, mv)
        assert np.array_equal(got, want), (coeff, mv, int((got != want).sum()))
        hits += 0 < int((want == 255).sum()) < want.size
    assert hits >= 2   # (some of the parameter pairs split the page: both values of the mask are compared)


def test_variance_map_equals_the_oracle(oracle):
    import ctypes as C

    L = oracle.lib()
    for shape in ((1, 1), (1, 40), (40, 1), (33, 40)):
        page = np.ascontiguousarray(lr.colour(shape[0], shape[1], 1))
        out = np.empty(shape + (3,), np.float32)
        L.prl_oracle_local_variance_map.restype = None
        L.prl_oracle_local_variance_map.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
        L.prl_oracle_local_variance_map(page.ctypes.data, page.strides[0], shape[1], shape[0], out.ctypes.data)
        assert np.array_equal(lr.variance_map(page).view(np.uint32), out.view(np.uint32)), shape


def _final_loops(G, N, mvs):
    """cv::adaptiveThreshold(MEAN_C, 15) and the subtraction, pixel by pixel: clamped coordinates, 225 additions"""
    h, w = G.shape
    g = G.tolist()
    n = N.tolist()
    out = {mv: np.zeros((h, w), np.uint8) for mv in mvs}
    for y in range(h):
        for x in range(w):
            total = 0
            for dy in range(-7, 8):
                row = g[min(max(y + dy, 0), h - 1)]
                for dx in range(-7, 8):
                    total += row[min(max(x + dx, 0), w - 1)]
            mean = round(total * (1.0 / 225))     # Python's round: half to even
            a = 127 if g[y][x] - mean > 0 else 0
            diff = max(0, a - n[y][x])
            for mv in mvs:
                out[mv][y, x] = 255 if diff > mv else 0
    return out


@pytest.mark.parametrize("shape", [(1, 1), (7, 9), (15, 15), (16, 40), (33, 65)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_final_from_maps_equals_the_double_loop(shape):
    mvs = (-1, 0, 25, 126, 127)
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    special = np.array([0, 127, 128, 255], np.uint8)
    for kind in range(3):
        G = rng.integers(0, 256, shape, dtype=np.uint8)
        N = rng.integers(0, 256, shape, dtype=np.uint8)
        if kind == 1:     # smooth G (means close to the centre value: the sign of G - mean decides), small N
            yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
            G = np.clip(100 + 3 * xx - 2 * yy + rng.integers(-2, 3, shape), 0, 255).astype(np.uint8)
            N = rng.integers(0, 130, shape, dtype=np.uint8)
        # a third of the positions of either map take one of 0, 127, 128, 255
        pick = rng.random(shape) < 1 / 3
        G[pick] = special[rng.integers(0, 4, int(pick.sum()))]
        pick = rng.random(shape) < 1 / 3
        N[pick] = special[rng.integers(0, 4, int(pick.sum()))]
        if G.size >= 4:
            G.flat[:4] = special
            N.flat[:4] = special[::-1]
        want = _final_loops(G, N, mvs)
        for mv in mvs:
            got = lr.final_from_maps(G, N, mv)
            assert np.array_equal(got, want[mv]), (shape, kind, mv, int((got != want[mv]).sum()))
        assert (want[-1] == 255).all() and not want[127].any()     # 0 > -1 everywhere; a - N <= 127 everywhere
        if G.size >= 100:
            assert 0 < int((want[0] == 255).sum()) < G.size


@pytest.mark.parametrize("shape", FILTER_SHAPES, ids=[f"{h}x{w}" for h, w in FILTER_SHAPES])
def test_pieces_put_together_stay_within_the_allowance_of_the_oracle(oracle, shape):
    """r1_r2, maps64 rounded half to even and final_from_maps against oracle.binarize_lv (float32 logf / expf / powf): ties the model
    of the GPU tests to the C oracle.  The counts are printed; they are near zero."""
    counts = []
    for seed in (3, 4):
        page = lr.colour(shape[0], shape[1], seed, skew=1.0)
        for coeff, mv, gamma in FILTER_PARAMS:
            got, _, _ = lr.with_filters(page, coeff, mv, gamma)
            want = oracle.binarize_lv(page, coeff, mv, gamma)
            bad = int((got != want).sum())
            counts.append(bad)
            assert bad <= lr.allowance(want.size), (shape, seed, coeff, mv, gamma, bad, want.size)
            assert 0 < int((want == 255).sum()) < want.size
    print(f"lv_ref.with_filters vs oracle.binarize_lv at {shape}: differing pixels {counts}")
