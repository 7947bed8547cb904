"""The focus measures LAPM, LAPV, TENG, GLVN (src/detectors/blurDetection.cpp:32-83) restated in numpy: the six integer sums of a
page and channel in int64, with BORDER_REFLECT_101 written as an index function, and the four measures from the sums in numpy
float64, one rounding per operation (include/prl_hip.h, "focus measures").  The yardstick of tests/test_focus_cpu.py and
tests/test_focus_gpu.py; also the page generators they share and the geometry constants of k_focus (focus.hip)."""
import numpy as np

SUM_P, SUM_P2, SUM_LAP, SUM_LAP2, SUM_LAPM4, SUM_TENG = range(6)
LAPM, LAPV, TENG, GLVN = range(4)

# k_focus: a lane takes 4 pixels of a row, a wavefront a tile of STRIP_PX columns x TILE_ROWS rows, a workgroup TILES_PER_GROUP
# tiles; the groups of 4 whose window of dwords would leave the row (the first, the last one to three) go pixel by pixel in an
# edge tile of their own per TILE_ROWS rows, a lane per row
LANE_PX, STRIP_PX, TILE_ROWS, TILES_PER_GROUP = 4, 256, 64, 4

# the bounds stated in the header
MAX_L, MAX_XY, MAX_TENG = 1020, 2040, 2 * 1020 * 1020
MAX_SIDE = 32768


def reflect101(i, n):
    """cv::borderInterpolate(i, n, BORDER_REFLECT_101) for an array of indices in [-1, n]"""
    i = np.asarray(i)
    if n == 1:
        return np.zeros_like(i)
    return np.where(i < 0, -i, np.where(i >= n, 2 * n - 2 - i, i))


def shifted(p, dy, dx):
    """p(y + dy, x + dx) with reflected indices, as int64; p: H x W"""
    h, w = p.shape
    ys, xs = reflect101(np.arange(h) + dy, h), reflect101(np.arange(w) + dx, w)
    return p[np.ix_(ys, xs)].astype(np.int64)


def plane_sums(p, ksize=3):
    """the six sums of one channel (H x W uint8) as a list of Python ints"""
    if ksize not in (1, 3):
        raise ValueError("ksize")
    t = {(dy, dx): shifted(p, dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)}
    c = t[0, 0]
    lap = t[-1, 0] + t[1, 0] + t[0, -1] + t[0, 1] - 4 * c
    wgt = {-1: 1, 0: 2, 1: 1}
    x = sum(wgt[dy] * (2 * t[dy, 0] - t[dy, -1] - t[dy, 1]) for dy in (-1, 0, 1))
    y = sum(wgt[dx] * (2 * t[0, dx] - t[-1, dx] - t[1, dx]) for dx in (-1, 0, 1))
    if ksize == 3:
        gx = sum(wgt[dy] * (t[dy, 1] - t[dy, -1]) for dy in (-1, 0, 1))
        gy = sum(wgt[dx] * (t[1, dx] - t[-1, dx]) for dx in (-1, 0, 1))
    else:
        gx, gy = t[0, 1] - t[0, -1], t[1, 0] - t[-1, 0]
    assert np.abs(lap).max() <= MAX_L and max(np.abs(x).max(), np.abs(y).max()) <= MAX_XY and (gx * gx + gy * gy).max() <= MAX_TENG
    return [int(v.sum()) for v in (c, c * c, lap, lap * lap, np.abs(x) + np.abs(y), gx * gx + gy * gy)]


def sums(page, ksize=3):
    """H x W -> int64 [6]; H x W x C -> int64 [C, 6]"""
    page = np.asarray(page)
    assert page.dtype == np.uint8
    if page.ndim == 2:
        return np.array(plane_sums(page, ksize), np.int64)
    return np.array([plane_sums(page[:, :, c], ksize) for c in range(page.shape[2])], np.int64)


def batch_sums(pages, ksize=3):
    """N x H x W [x C] -> int64 [N, [C,] 6]"""
    return np.stack([sums(p, ksize) for p in pages])


def from_sums(s, width, height):
    """int64 [..., 6] -> float64 [..., 4]; numpy scalars throughout (Python's 0.0 / 0.0 raises)"""
    s = np.asarray(s, np.int64)
    out = np.empty(s.shape[:-1] + (4,), np.float64)
    f = s.astype(np.float64)   # exact below 2^53
    with np.errstate(all="ignore"):
        scale = np.float64(1.0) / np.float64(width * height)
        out[..., LAPM] = (f[..., SUM_LAPM4] / np.float64(4.0)) * scale
        m = f[..., SUM_LAP] * scale
        sd = np.sqrt(np.maximum(f[..., SUM_LAP2] * scale - m * m, np.float64(0.0)))
        out[..., LAPV] = sd * sd
        out[..., TENG] = f[..., SUM_TENG] * scale
        mu = f[..., SUM_P] * scale
        sg = np.sqrt(np.maximum(f[..., SUM_P2] * scale - mu * mu, np.float64(0.0)))
        out[..., GLVN] = (sg * sg) / mu
    return out


def measures(page, ksize=3):
    page = np.asarray(page)
    return from_sums(sums(page, ksize), page.shape[1], page.shape[0])


def same_bits(a, b):
    """bit for bit, NaN equal to NaN"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


# ---- pages ------------------------------------------------------------------------------------------------------------------------

def noise(h, w, c=1, seed=0):
    """random bytes; H x W for c == 1, else H x W x c"""
    rng = np.random.default_rng(1000 * seed + 7 * h + w + c)
    return rng.integers(0, 256, size=(h, w) if c == 1 else (h, w, c), dtype=np.uint8)


def extremes(h, w, seed=0):
    """random pages of 0 and 255 only: the largest terms"""
    rng = np.random.default_rng(31 * seed + h * 3 + w)
    return (rng.integers(0, 2, size=(h, w), dtype=np.uint8) * 255).astype(np.uint8)


def stripes4(h, w):
    """vertical stripes 0, 0, 255, 255: |Gx| = 1020 on every interior pixel (the largest S_TENG)"""
    return np.tile(np.array([0, 0, 255, 255], np.uint8)[(np.arange(w) % 4)], (h, 1))


def checkerboard(h, w):
    """0 / 255 by the parity of x + y: |L| = 1020 (the largest S_LAP2)"""
    yy, xx = np.mgrid[0:h, 0:w]
    return (((yy + xx) & 1) * 255).astype(np.uint8)


def stripes2(h, w):
    """vertical stripes of period 2: |X| = 2040 (the largest S_LAPM4)"""
    return np.tile(((np.arange(w) & 1) * 255).astype(np.uint8), (h, 1))


def flat(h, w, v):
    return np.full((h, w), v, np.uint8)
