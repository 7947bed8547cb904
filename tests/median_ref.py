"""Restatement of prl::denoiseSaltPepper for the tests: `times` passes of cv::medianBlur(out, out, k) written from its
definition (numpy only, no scipy).

out(y, x, c) = the value at rank (k*k - 1) / 2 of in(clamp(y+i, 0, H-1), clamp(x+j, 0, W-1), c), |i|, |j| <= k/2.

Small windows sort every window (sliding_window_view + np.partition, in row chunks); large windows count: for each level v
the box sum of (page <= v) over the window is the number of window values <= v, and the median is the number of levels whose
count stays at or below the rank.  Both read the replicate-padded page; results are exact integers either way.
"""
from __future__ import annotations

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

PARTITION_MAX_K = 5


def _as3(img):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3)
    return img if img.ndim == 3 else img[:, :, None]


def _pass_partition(a, k, chunk_elems=1 << 24):
    h = k // 2
    H, W, C = a.shape
    t = (k * k - 1) // 2
    p = np.pad(a, ((h, h), (h, h), (0, 0)), mode="edge")
    out = np.empty_like(a)
    rows = max(1, chunk_elems // max(1, W * C * k * k))
    for y0 in range(0, H, rows):
        y1 = min(H, y0 + rows)
        win = sliding_window_view(p[y0:y1 + 2 * h], (k, k), axis=(0, 1))   # (y1-y0, W, C, k, k)
        flat = win.reshape(win.shape[0], W, C, k * k)
        out[y0:y1] = np.partition(flat, t, axis=-1)[..., t]
    return out


def _pass_count(a, k):
    h = k // 2
    H, W, C = a.shape
    t = (k * k - 1) // 2
    p = np.pad(a, ((h, h), (h, h), (0, 0)), mode="edge")
    med = np.zeros((H, W, C), np.int64)
    lo, hi = int(a.min()), int(a.max())
    for v in range(lo, hi):   # levels below min count 0 <= t (add lo once), levels >= max count k*k > t
        s = np.zeros((p.shape[0] + 1, p.shape[1] + 1, C), np.int64)
        s[1:, 1:] = np.cumsum(np.cumsum(p <= v, axis=0, dtype=np.int64), axis=1)
        box = s[k:, k:] - s[:-k, k:] - s[k:, :-k] + s[:-k, :-k]
        med += box <= t
    return (med + lo).astype(np.uint8)


def median_pass(img, k):
    a = _as3(img)
    out = _pass_partition(a, k) if k <= PARTITION_MAX_K else _pass_count(a, k)
    return out if np.asarray(img).ndim == 3 else out[:, :, 0]


def denoise_salt_pepper(img, k, times=1):
    """The whole call: a copy for times == 0 or k == 1, else `times` passes."""
    out = np.array(img, copy=True)
    if k == 1:
        return out
    for _ in range(times):
        out = median_pass(out, k)
    return out


def denoise_salt_pepper_rows(img, k, times, y0, y1):
    """Rows [y0, y1) of denoise_salt_pepper(img, k, times) from a band of the page: row y after `times` passes depends on
    input rows y +- times * (k // 2) only, and the band's own borders coincide with the page's wherever they are clamped."""
    H = np.asarray(img).shape[0]
    m = times * (k // 2)
    a, b = max(0, y0 - m), min(H, y1 + m)
    band = denoise_salt_pepper(np.asarray(img)[a:b], k, times)
    return band[y0 - a:y1 - a]


def median_loop(img, k):
    """One pass pixel by pixel (the definition, for small pages)."""
    a = _as3(img)
    H, W, C = a.shape
    h = k // 2
    out = np.empty_like(a)
    for y in range(H):
        for x in range(W):
            for c in range(C):
                vals = sorted(int(a[min(max(y + i, 0), H - 1), min(max(x + j, 0), W - 1), c])
                              for i in range(-h, h + 1) for j in range(-h, h + 1))
                out[y, x, c] = vals[(k * k - 1) // 2]
    return out if np.asarray(img).ndim == 3 else out[:, :, 0]
