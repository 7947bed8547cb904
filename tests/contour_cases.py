"""Maps for the contour tests: the hand-made ones of tests/test_contour_cpu.py (also what tests/cpp/test_contour.cpp draws for
itself) and the seeded fuzz families - random polygons, outlines with gaps, noise."""
from __future__ import annotations

import numpy as np


def _line(img, x0, y0, x1, y1):
    """Bresenham, 8-connected"""
    dx, dy = abs(x1 - x0), -abs(y1 - y0)
    sx, sy = (1 if x0 < x1 else -1), (1 if y0 < y1 else -1)
    err = dx + dy
    h, w = img.shape
    while True:
        if 0 <= x0 < w and 0 <= y0 < h:
            img[y0, x0] = 255
        if x0 == x1 and y0 == y1:
            return
        e2 = 2 * err
        if e2 >= dy:
            err += dy
            x0 += sx
        if e2 <= dx:
            err += dx
            y0 += sy


def outline(w, h, corners):
    img = np.zeros((h, w), np.uint8)
    n = len(corners)
    for i in range(n):
        _line(img, *corners[i], *corners[(i + 1) % n])
    return img


def filled(w, h, corners):
    """the polygon's interior and border by the even-odd rule on pixel centres, plus its outline"""
    img = outline(w, h, corners)
    ys, xs = np.mgrid[0:h, 0:w]
    inside = np.zeros((h, w), bool)
    n = len(corners)
    for i in range(n):
        (x0, y0), (x1, y1) = corners[i], corners[(i + 1) % n]
        if y0 == y1:
            continue
        cond = ((y0 <= ys) & (ys < y1)) | ((y1 <= ys) & (ys < y0))
        xi = x0 + (ys - y0) * (x1 - x0) / float(y1 - y0)
        inside ^= cond & (xs < xi)
    img[inside] = 255
    return img


def hand_made():
    """name -> (map, expected: True a quad, False none, None not stated)"""
    cases = {}
    cases["filled_rectangle"] = (filled(40, 30, [(8, 6), (30, 6), (30, 22), (8, 22)]), True)
    cases["one_pixel_outline"] = (outline(40, 30, [(8, 6), (30, 6), (30, 22), (8, 22)]), True)
    # its outer and its hole border run over the same pixels: two candidates of one area, the first in the order is kept
    cases["diamond_outline_tie"] = (outline(64, 64, [(32, 4), (60, 32), (32, 60), (4, 32)]), True)
    cases["outline_on_the_border"] = (outline(40, 30, [(0, 0), (39, 0), (39, 29), (0, 29)]), True)
    cases["rotated_quadrilateral"] = (outline(64, 64, [(30, 4), (58, 30), (32, 58), (5, 31)]), True)
    cases["trapezoid_sides"] = (outline(64, 48, [(20, 6), (44, 6), (60, 40), (4, 40)]), False)
    # a flat isosceles trapezoid: both pairs of opposite sides within 0.85, the legs 28 degrees from parallel
    cases["angle_below_160"] = (outline(64, 64, [(7, 26), (57, 26), (60, 38), (4, 38)]), False)
    cases["below_five_percent"] = (outline(64, 64, [(10, 10), (20, 10), (20, 20), (10, 20)]), False)
    cases["five_sides"] = (outline(64, 64, [(32, 4), (60, 26), (48, 58), (16, 58), (4, 26)]), None)
    iso = np.zeros((9, 9), np.uint8)
    iso[4, 4] = 255
    cases["isolated_pixel"] = (iso, False)
    cases["empty"] = (np.zeros((12, 17), np.uint8), False)
    cases["full"] = (np.full((12, 17), 255, np.uint8), None)
    cases["1x1"] = (np.full((1, 1), 255, np.uint8), False)
    cases["1x9"] = (np.array([[255, 0, 255, 255, 0, 0, 255, 255, 255]], np.uint8).reshape(9, 1).T.copy(), False)
    wide = np.zeros((3, 511), np.uint8)
    wide[0, :] = wide[2, :] = 255
    wide[1, 0] = wide[1, 510] = wide[1, 200] = 255
    cases["511x3"] = (wide, None)
    return cases


def fuzz_map(seed):
    """one map of at most 64 x 64: a family by seed % 3"""
    rng = np.random.default_rng(1000 + seed)
    w, h = int(rng.integers(8, 65)), int(rng.integers(8, 65))
    family = seed % 3
    if family == 0:     # a near-rectangle outline or filled shape, sometimes with extra clutter
        mx, my = max(1, w // 8), max(1, h // 8)
        j = lambda lim: int(rng.integers(0, lim + 1))   # noqa: E731
        corners = [(j(mx), j(my)), (w - 1 - j(mx), j(my)), (w - 1 - j(mx), h - 1 - j(my)), (j(mx), h - 1 - j(my))]
        img = filled(w, h, corners) if rng.random() < 0.3 else outline(w, h, corners)
        for _ in range(int(rng.integers(0, 3))):
            _line(img, int(rng.integers(0, w)), int(rng.integers(0, h)), int(rng.integers(0, w)), int(rng.integers(0, h)))
        return img
    if family == 1:     # a random polygon of 3..7 corners as an outline with gaps
        n = int(rng.integers(3, 8))
        ang = np.sort(rng.random(n) * 2 * np.pi)
        rad = 0.25 + 0.2 * rng.random(n)
        corners = [(int(w / 2 + r * w * np.cos(a)), int(h / 2 + r * h * np.sin(a))) for a, r in zip(ang, rad)]
        img = outline(w, h, corners)
        gaps = rng.random((h, w)) < 0.05 * rng.integers(0, 3)
        img[gaps] = 0
        return img
    img = (rng.random((h, w)) < rng.choice([0.1, 0.3, 0.5, 0.7])).astype(np.uint8) * 255   # noise
    return img
