"""prl::basicDeblur (src/deblur/basicDeblur.cpp:33-70) and the float32 cv::GaussianBlur under it, restated in numpy float32 with one
rounding per operation (include/prl_hip.h, "basicDeblur"): the size and sigma rules, the weights with math.exp for the terms,
cv::borderInterpolate(BORDER_REFLECT_101) with its loop, the row pass (n >= 7 and n == 1: taps in ascending order; n = 3, 5: centre,
then pairs), the column pass (centre, then pairs outward), addWeighted and the rounding to a byte.  The yardstick of
tests/test_deblur_cpu.py and tests/test_deblur_gpu.py; also the page generators they share and the geometry of k_deblur."""
import math

import numpy as np

f32 = np.float32
MAX_SIDE = 255            # PRL_GAUSS_MAX_SIDE
LDS_BYTES = 64 << 10      # k_deblur: the ring of ny x TW words and two row buffers of TW + 2 rx C words fit this
DBL_EPSILON = 2.220446049250313e-16
_TABLES = {1: [1.0], 3: [0.25, 0.5, 0.25], 5: [0.0625, 0.25, 0.375, 0.25, 0.0625],
           7: [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]}


def reflect101(p, n):
    """cv::borderInterpolate(p, n, BORDER_REFLECT_101), the loop itself"""
    if 0 <= p < n:
        return p
    if n == 1:
        return 0
    while True:
        p = -p if p < 0 else 2 * n - 2 - p
        if 0 <= p < n:
            return p


def side(k, sigma):
    """one side of the kernel; None where cv::GaussianBlur's assertion fails (or the side leaves int)"""
    if not -2 ** 31 <= k < 2 ** 31:
        return None
    if k <= 0:
        if not sigma > 0:
            return None
        v = sigma * 4 * 2 + 1
        if not v < 2 ** 31 - 1:
            return None
        k = int(np.rint(v)) | 1
    return k if k % 2 == 1 else None


def plan(kw, kh, sigma_x, sigma_y):
    """(nx, ny, sx, sy, shared)"""
    if sigma_y <= 0:
        sigma_y = sigma_x
    nx, ny = side(kw, sigma_x), side(kh, sigma_y)
    sx, sy = max(sigma_x, 0.0), max(sigma_y, 0.0)
    return nx, ny, sx, sy, nx == ny and abs(sx - sy) < DBL_EPSILON


def kernel(n, sigma=0.0):
    """cv::getGaussianKernel(n, sigma, CV_32F)"""
    assert n > 0 and n % 2 == 1
    if n <= 7 and not sigma > 0:
        return np.array(_TABLES[n], f32)
    s = sigma if sigma > 0 else ((n - 1) * 0.5 - 1) * 0.3 + 0.8
    scale2x = -0.5 / (s * s)
    t = []
    total = 0.0
    for i in range(n):
        x = i - (n - 1) * 0.5
        t.append(math.exp(scale2x * x * x))
        total += t[-1]
    total = 1.0 / total
    return np.array([v * total for v in t], np.float64).astype(f32)


def kernels(kw, kh, sigma_x, sigma_y):
    nx, ny, sx, sy, shared = plan(kw, kh, sigma_x, sigma_y)
    wx = kernel(nx, sx)
    return wx, (wx if shared else kernel(ny, sy))


def _row_pass(a, w):
    """a: H x W x C float32; taps along the pixel axis"""
    n, r, W = len(w), len(w) // 2, a.shape[1]
    xi = [np.array([reflect101(x - r + k, W) for x in range(W)]) for k in range(n)]
    if n in (3, 5):
        acc = a[:, xi[r]] * w[r]
        for k in range(1, r + 1):
            acc = acc + (a[:, xi[r + k]] + a[:, xi[r - k]]) * w[r + k]
        return acc
    acc = w[0] * a[:, xi[0]]
    for k in range(1, n):
        acc = acc + w[k] * a[:, xi[k]]
    return acc


def _col_pass(a, w):
    r, H = len(w) // 2, a.shape[0]
    yi = [np.array([reflect101(y - r + k, H) for y in range(H)]) for k in range(len(w))]
    acc = w[r] * a[yi[r]]
    for k in range(1, r + 1):
        acc = acc + w[r + k] * (a[yi[r + k]] + a[yi[r - k]])
    return acc


def blur(page, ksize=(0, 0), sigma_x=9.0, sigma_y=0.0):
    """H x W [x C] uint8 -> float32 of the same shape"""
    page = np.asarray(page)
    assert page.dtype == np.uint8
    wx, wy = kernels(ksize[0], ksize[1], sigma_x, sigma_y)
    a = page.astype(f32).reshape(page.shape[0], page.shape[1], -1)
    g = _col_pass(_row_pass(a, wx), wy)
    assert g.dtype == f32
    return g.reshape(page.shape)


def sat_u8(t):
    """saturate_u8(cvRound(t)): half to even; NaN, +-inf and what lies outside int32 give 0"""
    t = np.asarray(t, f32)
    with np.errstate(invalid="ignore"):
        ok = (t >= f32(-2147483648.0)) & (t < f32(2147483648.0))
        r = np.clip(np.rint(np.where(ok, t, f32(0))), 0, 255)
    return r.astype(np.uint8)


def weights(image_weight):
    return f32(2.0 * image_weight), f32(2.0 * image_weight - 2.0)


def deblur_from(page, g, image_weight=0.75):
    alpha, beta = weights(image_weight)
    x = np.asarray(page).astype(f32)
    with np.errstate(all="ignore"):
        t = (x * alpha + g * beta) + f32(0.0)
    assert t.dtype == f32
    return sat_u8(t)


def deblur(page, ksize=0, sigma_x=9.0, sigma_y=0.0, image_weight=0.75):
    return deblur_from(page, blur(page, (ksize, ksize), sigma_x, sigma_y), image_weight)


def blur_loop(page, ksize, sigma_x, sigma_y):
    """the same, written independently sample by sample (small gray pages)"""
    wx, wy = kernels(ksize[0], ksize[1], sigma_x, sigma_y)
    H, W = page.shape
    nx, ny, rx, ry = len(wx), len(wy), len(wx) // 2, len(wy) // 2
    rows = np.zeros((H, W), f32)
    for y in range(H):
        for x in range(W):
            v = [f32(page[y, reflect101(x - rx + k, W)]) for k in range(nx)]
            if nx in (3, 5):
                s = f32(v[rx] * wx[rx])
                for k in range(1, rx + 1):
                    s = f32(s + f32(f32(v[rx + k] + v[rx - k]) * wx[rx + k]))
            else:
                s = f32(wx[0] * v[0])
                for k in range(1, nx):
                    s = f32(s + f32(wx[k] * v[k]))
            rows[y, x] = s
    out = np.zeros((H, W), f32)
    for y in range(H):
        for x in range(W):
            s = f32(wy[ry] * rows[y, x])
            for k in range(1, ry + 1):
                s = f32(s + f32(wy[ry + k] * f32(rows[reflect101(y + k, H), x] + rows[reflect101(y - k, H), x])))
            out[y, x] = s
    return out


def same_bits(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


# ---- the geometry of k_deblur (deblur.hip) -------------------------------------------------------------------------------------

def tile_width(nx, ny, channels):
    """samples of a row a workgroup owns: the widest of 256, 128, 64 whose LDS fits, else 32"""
    for tw in (256, 128, 64):
        if (ny * tw + 2 * (tw + 2 * (nx // 2) * channels)) * 4 <= LDS_BYTES:
            return tw
    return 32


def rows_per_group(ny, height):
    return min(height, max(96, 6 * ny))


# ---- pages ---------------------------------------------------------------------------------------------------------------------

def noise(h, w, c=1, seed=0):
    rng = np.random.default_rng(1000 * seed + 7 * h + w + c)
    return rng.integers(0, 256, size=(h, w) if c == 1 else (h, w, c), dtype=np.uint8)


def checkerboard(h, w, c=1):
    yy, xx = np.mgrid[0:h, 0:w]
    p = (((yy + xx) & 1) * 255).astype(np.uint8)
    return p if c == 1 else np.repeat(p[:, :, None], c, axis=2)


def flat(h, w, v, c=1):
    return np.full((h, w) if c == 1 else (h, w, c), v, np.uint8)
