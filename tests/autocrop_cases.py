"""Synthetic photographs for the border detector's tests: a bright quadrilateral (the page) on a dark table.

  found      the quadrilateral alone: the first search finds it
  bridged    the same with a narrow strip of the page's brightness from one side out to the picture's border: the page's outline
             is an open curve, which has no area, until the closing joins the strip's two banks
  flat       one brightness: no edge, no quad
"""
from __future__ import annotations

import numpy as np


def _inside(w, h, corners):
    ys, xs = np.mgrid[0:h, 0:w]
    inside = np.ones((h, w), bool)
    n = len(corners)
    for i in range(n):
        (x0, y0), (x1, y1) = corners[i], corners[(i + 1) % n]
        inside &= (x1 - x0) * (ys - y0) - (y1 - y0) * (xs - x0) >= 0
    return inside


def quadrilateral(w, h, lean=0.04):
    """corners top left, top right, bottom right, bottom left, a little out of square"""
    return [(int(w * 0.14), int(h * (0.12 + lean))), (int(w * 0.86), int(h * 0.12)), (int(w * (0.86 - lean)), int(h * 0.88)),
            (int(w * (0.14 + lean / 2)), int(h * (0.88 - lean / 2)))]


def page(w, h, kind, channels=3, bridge=None, seed=0, lean=0.04):
    """H x W [x C] uint8; kind: 'found', 'bridged', 'flat'; bridge: the strip's width in source pixels; lean: see quadrilateral"""
    rng = np.random.default_rng(seed)
    g = np.full((h, w), 40, np.uint8)
    if kind != "flat":
        g[_inside(w, h, quadrilateral(w, h, lean))] = 205
        if kind == "bridged":
            y = int(h * 0.5)
            g[y:y + bridge, : int(w * 0.5)] = 205
    else:
        g[:] = 120
    if channels == 1:
        return g
    out = np.stack([(g >> 1) + 20, g, 255 - (g >> 2), np.full_like(g, 255)][:channels], axis=2).astype(np.uint8)
    out[..., 0] += rng.integers(0, 2, size=(h, w), dtype=np.uint8)   # a grain of noise below every threshold
    return np.ascontiguousarray(out)
