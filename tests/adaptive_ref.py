"""Restatement of cv::adaptiveThreshold and of the reference's binarizers built on it, for the tests (numpy only).

    M        local mean of the bs x bs block, BORDER_REPLICATE
      MEAN_C      S = integer block sum; M = saturate_u8(cvRound(S * (1.0 / (bs*bs)))), product in float64, half to even
      GAUSSIAN_C  float32 page -> separable float32 Gaussian -> saturate_u8(cvRound(.)):
                  weights: fixed tables for bs 3, 5, 7, else sigma = ((bs-1)*0.5 - 1)*0.3 + 0.8,
                  t_i = exp(-0.5/(sigma*sigma) * x_i*x_i) in float64, the sum in index order, w_i = float32(t_i * (1/sum));
                  row pass bs >= 7: taps in ascending order; bs 3, 5: centre, then pairs; column pass: centre, then pairs;
                  every product and every sum rounded to float32
    on       p - M > -idelta, idelta = ceil(delta) for BINARY, floor(delta) for BINARY_INV
    out      BINARY: on ? imax : 0; BINARY_INV: on ? 0 : imax; imax = saturate_u8(cvRound(maxValue)); maxValue < 0: all 0
    flip     binarizeNativeAdaptive.cpp:108-111: mean(out) < 128 -> 255 - out

Whole-plane functions (mean_box, mean_gauss, adaptive_threshold, the four binarize*) and an independently written
per-pixel model (mean_box_loop, mean_gauss_loop) for small pages.
"""
from __future__ import annotations

import math

import numpy as np

import median_ref

f32 = np.float32
MEAN_C, GAUSSIAN_C = 0, 1
BINARY, BINARY_INV = 0, 1
_SMALL = {3: [0.25, 0.5, 0.25], 5: [0.0625, 0.25, 0.375, 0.25, 0.0625],
          7: [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]}


def gauss_weights(bs):
    if bs in _SMALL:
        return np.array(_SMALL[bs], f32)
    sigma = ((bs - 1) * 0.5 - 1) * 0.3 + 0.8
    scale2x = -0.5 / (sigma * sigma)
    t = []
    total = 0.0
    for i in range(bs):
        x = i - (bs - 1) * 0.5
        t.append(math.exp(scale2x * x * x))
        total += t[-1]
    total = 1.0 / total
    return np.array([v * total for v in t], np.float64).astype(f32)


def _row_pass(a, w):
    n = len(w)
    r = n // 2
    W = a.shape[1]
    p = a[:, np.clip(np.arange(-r, W + r), 0, W - 1)]
    if n <= 5:
        acc = p[:, r:r + W] * w[r]
        for k in range(1, r + 1):
            acc = acc + (p[:, r + k:r + k + W] + p[:, r - k:r - k + W]) * w[r + k]
        return acc
    acc = w[0] * p[:, 0:W]
    for k in range(1, n):
        acc = acc + w[k] * p[:, k:k + W]
    return acc


def _col_pass(a, w):
    r = len(w) // 2
    H = a.shape[0]
    q = a[np.clip(np.arange(-r, H + r), 0, H - 1)]
    acc = w[r] * q[r:r + H]
    for k in range(1, r + 1):
        acc = acc + w[r + k] * (q[r + k:r + k + H] + q[r - k:r - k + H])
    return acc


def mean_gauss(g, bs):
    w = gauss_weights(bs)
    a = _col_pass(_row_pass(g.astype(f32), w), w)   # float32 arrays times float32 scalars: every operation rounds to float32
    assert a.dtype == f32
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def block_sum(g, bs):
    r = bs // 2
    H, W = g.shape
    p = np.pad(g.astype(np.int64), r, mode="edge")
    ii = np.zeros((H + 2 * r + 1, W + 2 * r + 1), np.int64)
    ii[1:, 1:] = p.cumsum(0).cumsum(1)
    return ii[bs:, bs:] - ii[:-bs, bs:] - ii[bs:, :-bs] + ii[:-bs, :-bs]


def mean_box(g, bs):
    s = block_sum(g, bs)
    return np.clip(np.rint(s.astype(np.float64) * (1.0 / (bs * bs))), 0, 255).astype(np.uint8)


def mean_box_integer(g, bs):
    """(2 S + bs^2) // (2 bs^2): the same byte, because S / bs^2 is never closer than 1 / (2 bs^2) to a half (bs^2 is odd)."""
    return ((2 * block_sum(g, bs) + bs * bs) // (2 * bs * bs)).astype(np.uint8)


def local_mean(g, method, bs):
    return mean_gauss(g, bs) if method == GAUSSIAN_C else mean_box(g, bs)


def imax_of(max_value):
    return int(np.clip(np.rint(np.float64(max_value)), 0, 255))


def threshold_from_mean(g, m, max_value, type_, delta, auto_invert=False):
    """The comparison and the flip, given the mean plane (the grids of the tests compute a mean plane once per block size)."""
    if max_value < 0:
        out = np.zeros_like(g)
    else:
        idelta = math.floor(delta) if type_ == BINARY_INV else math.ceil(delta)
        on = (g.astype(np.int64) - m.astype(np.int64)) > -idelta
        out = np.where(on ^ (type_ == BINARY_INV), imax_of(max_value), 0).astype(np.uint8)
    if auto_invert and flips(out):
        out = (255 - out.astype(np.int64)).astype(np.uint8)
    return out


def adaptive_threshold(g, max_value, method, type_, bs, delta, auto_invert=False):
    assert g.dtype == np.uint8 and g.ndim == 2 and bs >= 3 and bs % 2 == 1
    return threshold_from_mean(g, local_mean(g, method, bs), max_value, type_, delta, auto_invert)


def flips(mask):
    return int(mask.astype(np.int64).sum()) < 128 * mask.size


def bgr2gray(img):
    b = img.astype(np.uint32)
    return ((b[..., 0] * 1868 + b[..., 1] * 9617 + b[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def auto_block_size(rows, cols):
    return int(math.sqrt(float(rows * rows + cols * cols)) / 333 + 7)


def binarize_native_adaptive(img, median=5, gaussian=True, max_value=255.0, bs=19, shift=9.0):
    g = bgr2gray(img) if img.ndim == 3 and img.shape[2] > 1 else img.reshape(img.shape[:2])
    b = median_ref.denoise_salt_pepper(g, median, 1)
    if bs < 3:
        bs = auto_block_size(*g.shape)
    return adaptive_threshold(b, max_value, GAUSSIAN_C if gaussian else MEAN_C, BINARY_INV, bs, shift, auto_invert=True)


def binarize_at(img, median, max_value, bs, shift, method=MEAN_C):
    assert img.ndim == 3 and img.shape[2] in (3, 4)
    return adaptive_threshold(bgr2gray(median_ref.denoise_salt_pepper(img, median, 1)), max_value, method, BINARY, bs, int(shift))


def binarize_agt(img, median, max_value, bs, shift):
    return binarize_at(img, median, max_value, bs, shift, method=GAUSSIAN_C)


def binarize_pure_adaptive_gaussian(img, max_value, bs, shift):
    assert img.ndim == 3 and img.shape[2] in (3, 4)
    return adaptive_threshold(bgr2gray(img), max_value, GAUSSIAN_C, BINARY, bs, int(shift))


# ---- per pixel, written independently of the above ----

def mean_box_loop(g, bs):
    H, W = g.shape
    r = bs // 2
    out = np.zeros((H, W), np.uint8)
    scale = 1.0 / (bs * bs)
    for y in range(H):
        for x in range(W):
            s = 0
            for i in range(-r, r + 1):
                for j in range(-r, r + 1):
                    s += int(g[min(max(y + i, 0), H - 1), min(max(x + j, 0), W - 1)])
            v = s * scale
            fl = math.floor(v)
            d = v - fl
            q = fl + 1 if d > 0.5 else fl if d < 0.5 else fl + (fl & 1)   # half to even
            out[y, x] = min(255, max(0, q))
    return out


def mean_gauss_loop(g, bs):
    w = gauss_weights(bs)
    r = bs // 2
    H, W = g.shape
    rows = np.zeros((H, W), f32)
    for y in range(H):
        for x in range(W):
            if bs <= 5:
                s = f32(f32(g[y, x]) * w[r])
                for k in range(1, r + 1):
                    s = f32(s + f32(f32(f32(g[y, min(W - 1, x + k)]) + f32(g[y, max(0, x - k)])) * w[r + k]))
            else:
                s = f32(w[0] * f32(g[y, max(0, x - r)]))
                for k in range(1, bs):
                    s = f32(s + f32(w[k] * f32(g[y, min(W - 1, max(0, x - r + k))])))
            rows[y, x] = s
    out = np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            s = f32(w[r] * rows[y, x])
            for k in range(1, r + 1):
                s = f32(s + f32(w[r + k] * f32(rows[min(H - 1, y + k), x] + rows[max(0, y - k), x])))
            out[y, x] = min(255, max(0, int(np.rint(s))))
    return out


def stripes_page(h=120, w=144):
    """columns x % 12 < 4 at 255, the rest 0: a page binarizeNativeAdaptive's defaults do not flip"""
    xx = np.mgrid[0:h, 0:w][1]
    return np.where(xx % 12 < 4, 255, 0).astype(np.uint8)
