"""Pages and maps for the Hough-line tests.

  sparse_map      a few random points
  designed_maps   empty, one full row, the last column, a diagonal, an all-ones 8 x 8 page
  corner_map      a point in each corner
  edge_page       what the edge-map tests blur and differentiate: 'random' noise, or 'stroke': bars that differ per channel, one
                  gray bar (every channel ties on it) and a little noise
  photo           synthetic photographs for the contour entry, on tests/autocrop_cases.py's quadrilateral:
                    'found'    the bright page on the dark table
                    'broken'   the same with a square of the table's brightness over the middle of every side: a polygon of twenty corners for
                               a contour follower, four straight lines for the votes
                    'flat'     one brightness: no edge, no line
                    'stripes'  parallel bands: lines enough, but no two directions, so no quad
"""
from __future__ import annotations

import numpy as np

import autocrop_cases


def sparse_map(w, h, seed, points=None):
    rng = np.random.default_rng(seed)
    m = np.zeros((h, w), np.uint8)
    k = points if points is not None else max(1, (w * h) // 12)
    m[rng.integers(0, h, k), rng.integers(0, w, k)] = rng.integers(1, 256, k)
    return m


def corner_map(w, h):
    m = np.zeros((h, w), np.uint8)
    m[0, 0] = m[0, w - 1] = m[h - 1, 0] = m[h - 1, w - 1] = 255
    return m


def designed_maps():
    out = {"empty": np.zeros((9, 13), np.uint8)}
    m = np.zeros((40, 70), np.uint8)
    m[17, :] = 255
    out["row"] = m
    m = np.zeros((66, 21), np.uint8)
    m[:, 20] = 1
    out["last_column"] = m
    m = np.zeros((64, 64), np.uint8)
    m[np.arange(64), np.arange(64)] = 200
    out["diagonal"] = m
    out["ones"] = np.ones((8, 8), np.uint8)
    return out


def edge_page(w, h, kind, channels, seed):
    rng = np.random.default_rng(seed)
    shape = (h, w) if channels == 1 else (h, w, channels)
    if kind == "random":
        return rng.integers(0, 256, size=shape, dtype=np.uint8)
    img = np.full((h, w, channels), 200, np.uint8)
    for ch in range(channels):   # a vertical and a horizontal bar per channel, each elsewhere
        x = int(w * (0.15 + 0.2 * ch))
        y = int(h * (0.2 + 0.18 * ch))
        img[:, x:x + max(3, w // 20), ch] = 40 + 30 * ch
        img[y:y + max(3, h // 16), :, ch] = 90 - 10 * ch
    d = np.arange(min(w, h))
    for t in range(-3, 4):   # a gray diagonal: the same step in every channel
        ok = (d + t >= 0) & (d + t < w)
        img[d[ok], (d + t)[ok], :] = 10
    img = img.astype(np.int16) + rng.integers(-3, 4, size=img.shape)
    img = np.clip(img, 0, 255).astype(np.uint8)
    return img[:, :, 0] if channels == 1 else np.ascontiguousarray(img)


def photo(w, h, kind, channels=3, seed=0):
    if kind in ("found", "flat"):
        return autocrop_cases.page(w, h, kind, channels=channels, seed=seed)
    g = np.full((h, w), 40, np.uint8)
    if kind == "broken":
        corners = autocrop_cases.quadrilateral(w, h)
        g[autocrop_cases._inside(w, h, corners)] = 205
        r = max(6, min(w, h) // 14)
        for i in range(4):   # a blot of table over the middle of every side
            (x0, y0), (x1, y1) = corners[i], corners[(i + 1) % 4]
            cx, cy = (x0 + x1) // 2, (y0 + y1) // 2
            g[max(cy - r, 0):cy + r, max(cx - r, 0):cx + r] = 40
    elif kind == "stripes":
        for y in range(h // 8, h - h // 8, max(h // 6, 24)):
            g[y:y + max(h // 14, 10), :] = 205
    else:
        raise ValueError(kind)
    if channels == 1:
        return g
    rng = np.random.default_rng(seed)
    out = np.stack([(g >> 1) + 20, g, 255 - (g >> 2), np.full_like(g, 255)][:channels], axis=2).astype(np.uint8)
    out[..., 0] += rng.integers(0, 2, size=(h, w), dtype=np.uint8)
    return np.ascontiguousarray(out)
