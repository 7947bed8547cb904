"""The restatement of cv::HoughLines(rho 1, theta pi / 180) and of prl::findHoughLineContour (src/border_detection/houghLine.cpp,
fromVec2f of imageLibCommon.cpp:929-941, intersection of autoCropUtils.cpp:350-366) in numpy, written from the reference's text and
OpenCV's HoughLinesStandard, as include/prl_hip.h ("Hough lines") states them.  float32 where the C++ is float, float64 where it is
double; sin / cos of the vote table are math.sin / math.cos (the C library's, in float64), the float32 cosf / sinf of fromVec2f
come from the C library through ctypes, so that both sides use the machine's libm.
"""
from __future__ import annotations

import ctypes
import ctypes.util
import itertools
import math

import numpy as np

import edges_ref
import median_ref

NUMANGLE = 180                       # cvRound(CV_PI / theta): the rule of OpenCV 3.4 / 4.x (not the later floor + 1 = 181)
THETA = np.float32(math.pi / 180)    # (float)(CV_PI / 180)
F32 = np.float32

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _f in (_libm.cosf, _libm.sinf):
    _f.restype = ctypes.c_float
    _f.argtypes = [ctypes.c_float]


def geometry(w, h):
    return NUMANGLE, (w + h) * 2 + 1


def trig_table():
    """(tabCos, tabSin): the angle accumulated in float32"""
    ang = F32(0)
    c, s = np.zeros(NUMANGLE, F32), np.zeros(NUMANGLE, F32)
    for n in range(NUMANGLE):
        s[n] = F32(math.sin(float(ang)) * 1.0)
        c[n] = F32(math.cos(float(ang)) * 1.0)
        ang = F32(ang + THETA)
    return c, s


def accumulator(edge_map):
    """(numangle + 2) x (numrho + 2) int32, framed by zeros"""
    h, w = edge_map.shape
    _, numrho = geometry(w, h)
    acc = np.zeros((NUMANGLE + 2, numrho + 2), np.int32)
    ys, xs = np.nonzero(edge_map)
    if ys.size == 0:
        return acc
    c, s = trig_table()
    x32, y32 = xs.astype(F32), ys.astype(F32)
    for n in range(NUMANGLE):
        a, b = x32 * c[n], y32 * s[n]          # each a float32 product
        r = np.rint(a + b).astype(np.int64) + (numrho - 1) // 2
        assert r.min() >= 0 and r.max() < numrho
        acc[n + 1, 1:numrho + 1] = np.bincount(r, minlength=numrho)
    return acc


def peaks(acc, threshold):
    """cell indices of the peaks in OpenCV's order, and their counts"""
    a = acc[1:-1, 1:-1]
    ok = (a > threshold) & (a > acc[1:-1, :-2]) & (a >= acc[1:-1, 2:]) & (a > acc[:-2, 1:-1]) & (a >= acc[2:, 1:-1])
    n, r = np.nonzero(ok)
    cell = (n + 1) * acc.shape[1] + r + 1
    cnt = a[n, r]
    order = np.lexsort((cell, -cnt.astype(np.int64)))
    return cell[order], cnt[order]


def lines_from_cells(cells, numrho):
    n = cells // (numrho + 2) - 1
    r = cells - (n + 1) * (numrho + 2) - 1
    rho = (r.astype(F32) - F32(numrho - 1) * F32(0.5)) * F32(1)
    theta = n.astype(F32) * THETA
    return np.stack([rho, theta], axis=1).astype(F32).reshape(-1, 2)


def hough_lines(edge_map, threshold):
    """K x 2 float32 (rho, theta)"""
    h, w = edge_map.shape
    cells, _ = peaks(accumulator(edge_map), threshold)
    return lines_from_cells(cells, geometry(w, h)[1])


# ---- the edge map -----------------------------------------------------------------------------------------------------------------

def colour_gradients(img):
    """dx, dy, padded magnitude of an H x W x C page, per pixel those of the channel of largest |dx| + |dy|, the first of equals;
    also the channel taken and whether two channels tied for it"""
    per = [edges_ref.gradients(img[:, :, ch]) for ch in range(img.shape[2])]
    mags = np.stack([p[2][1:-1, 1:-1] for p in per])
    best = np.argmax(mags, axis=0)   # the first maximum
    dx = np.choose(best, [p[0] for p in per])
    dy = np.choose(best, [p[1] for p in per])
    m = np.max(mags, axis=0)
    tied = (mags == m).sum(axis=0) > 1
    return dx, dy, np.pad(m, 1), best, tied


def classes_from_gradients(dx, dy, mp, t1, t2):
    """cv::Canny's stage 1 on one gradient per pixel (mp: the magnitudes inside one ring of zeros): 2 = edge, 0 = candidate, 1"""
    low, high = edges_ref.canny_thresholds(t1, t2)
    h, w = dx.shape
    m = mp[1:-1, 1:-1]
    at = lambda oy, ox: mp[1 + oy:1 + oy + h, 1 + ox:1 + ox + w]
    ax, ay = np.abs(dx), np.abs(dy) << 15
    t = ax * edges_ref.TG22
    horiz = ay < t
    vert = ~horiz & (ay > t + (ax << 16))
    s_neg = (dx ^ dy) < 0
    diag = np.where(s_neg, (m > at(-1, 1)) & (m > at(1, -1)), (m > at(-1, -1)) & (m > at(1, 1)))
    is_max = np.where(horiz, (m > at(0, -1)) & (m >= at(0, 1)), np.where(vert, (m > at(-1, 0)) & (m >= at(1, 0)), diag)) & (m > low)
    return np.where(is_max, np.where(m > high, 2, 0), 1).astype(np.uint8)


def canny_colour(img, t1, t2):
    if img.ndim == 2:
        return edges_ref.canny(img, t1, t2)
    dx, dy, mp, _, _ = colour_gradients(img)
    return edges_ref.edge_link(classes_from_gradients(dx, dy, mp, t1, t2))


def blurred(img):
    """houghLine.cpp:199-206"""
    cur = median_ref.denoise_salt_pepper(img, 3, 3)
    return median_ref.denoise_salt_pepper(cur, 5, 3)


def hough_edges(img):
    return canny_colour(blurred(img), 25, 50)


# ---- the line filter and the quad search ------------------------------------------------------------------------------------------

def from_vec2f(lines):
    """K x 2 (rho, theta) -> K x 4 float32 (x1, y1, x2, y2), integers"""
    lines = np.asarray(lines, F32).reshape(-1, 2)
    out = np.zeros((len(lines), 4), F32)
    for i, (rho, theta) in enumerate(lines):
        a, b = float(_libm.cosf(float(theta))), float(_libm.sinf(float(theta)))
        x0, y0 = a * float(rho), b * float(rho)
        out[i] = [np.rint(x0 + 1000 * (-b)), np.rint(y0 + 1000 * a), np.rint(x0 - 1000 * (-b)), np.rint(y0 - 1000 * a)]
    return out


def _dist(seg, pts):
    """distanceToLine of integer points pts (K x 2) to the integer segment seg"""
    sx, sy, ex, ey = (int(v) for v in seg)
    normal = np.hypot(float(ex - sx), float(ey - sy))
    cross = (pts[:, 0] - sx) * (ey - sy) - (pts[:, 1] - sy) * (ex - sx)
    return np.abs(cross.astype(np.float64) / normal)


def delete_similar_lines(lines, min_dist=5.0, step_dist=5.0, max_lines=20):
    lines = np.asarray(lines, F32).reshape(-1, 2)
    while len(lines) > max_lines:
        seg = from_vec2f(lines).astype(np.int64)
        used = np.zeros(len(lines), bool)
        kept = []
        for i in range(len(lines)):
            if used[i]:
                continue
            used[i] = True
            kept.append(i)
            js = np.nonzero(~used[i + 1:])[0] + i + 1
            if js.size == 0:
                continue
            d = np.minimum(np.minimum(_dist(seg[i], seg[js, 0:2]), _dist(seg[i], seg[js, 2:4])),
                           np.minimum(_dists_to(seg[js], seg[i, 0:2]), _dists_to(seg[js], seg[i, 2:4])))
            used[js[d < min_dist]] = True
        if len(kept) < 4:
            return lines[:max_lines].copy()
        lines = lines[kept]
        min_dist += step_dist
    return lines


def _dists_to(segs, p):
    """distanceToLine of the integer point p to each of the integer segments segs (K x 4)"""
    sx, sy, ex, ey = segs[:, 0], segs[:, 1], segs[:, 2], segs[:, 3]
    normal = np.hypot((ex - sx).astype(np.float64), (ey - sy).astype(np.float64))
    cross = (int(p[0]) - sx) * (ey - sy) - (int(p[1]) - sy) * (ex - sx)
    return np.abs(cross.astype(np.float64) / normal)


def intersections(seg):
    """at[a, b], ok[a, b]: intersection(seg[a].first, seg[a].second, seg[b].first, seg[b].second) for every ordered pair"""
    o1, p1 = seg[:, None, 0:2], seg[:, None, 2:4]
    o2, p2 = seg[None, :, 0:2], seg[None, :, 2:4]
    x = (o2 - o1).astype(F32)
    d1 = np.broadcast_to((p1 - o1).astype(F32), x.shape)
    d2 = np.broadcast_to((p2 - o2).astype(F32), x.shape)
    cross = (d1[..., 0] * d2[..., 1]).astype(F32) - (d1[..., 1] * d2[..., 0]).astype(F32)
    ok = ~(np.abs(cross.astype(np.float64) - 0.0) <= 1e-7)
    num = (x[..., 0] * d2[..., 1]).astype(F32) - (x[..., 1] * d2[..., 0]).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        t1 = (num / np.where(ok, cross, F32(1))).astype(F32).astype(np.float64)
    step = (d1.astype(np.float64) * t1[..., None]).astype(F32)
    at = (np.broadcast_to(o1, x.shape).astype(F32) + step).astype(F32)
    return at, ok


def _hull_size(pts):
    """vertices of the convex hull of the points (Andrew's chain on float64 coordinates; collinear points are no vertices)"""
    p = sorted(set((float(x), float(y)) for x, y in pts))
    if len(p) < 3:
        return len(p)
    cross = lambda o, a, b: (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])
    lower, upper = [], []
    for q in p:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], q) <= 0:
            lower.pop()
        lower.append(q)
    for q in reversed(p):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], q) <= 0:
            upper.pop()
        upper.append(q)
    return len(lower) + len(upper) - 2


def _is_contour_convex(P):
    """cv::isContourConvex on T x 4 x 2 float32 corners -> T bools"""
    prev, cur = P[:, 2], P[:, 3]
    dx0, dy0 = (cur[:, 0] - prev[:, 0]).astype(F32), (cur[:, 1] - prev[:, 1]).astype(F32)
    orient = np.zeros(len(P), np.int64)
    alive = np.ones(len(P), bool)
    for i in range(4):
        prev, cur = cur, P[:, i]
        dx, dy = (cur[:, 0] - prev[:, 0]).astype(F32), (cur[:, 1] - prev[:, 1]).astype(F32)
        dxdy0, dydx0 = (dx * dy0).astype(F32), (dy * dx0).astype(F32)
        orient |= np.where(dydx0 > dxdy0, 1, np.where(dydx0 < dxdy0, 2, 3))
        alive &= orient != 3
        dx0, dy0 = dx, dy
    return alive


def find_max_valid_contour(lines, width, height):
    """4 x 2 float32 corners or None"""
    lines = np.asarray(lines, F32).reshape(-1, 2)
    L = len(lines)
    if L < 4:
        return None
    at, ok = intersections(from_vec2f(lines))
    idx = np.array([t for t in itertools.permutations(range(L), 4)], np.int64)   # (i, j, k, m) in the loops' order
    i, j, k, m = idx.T
    good = ok[j, i] & ok[k, j] & ok[m, k] & ok[i, m]
    idx = idx[good]
    if len(idx) == 0:
        return None
    i, j, k, m = idx.T
    P = np.stack([at[j, i], at[k, j], at[m, k], at[i, m]], axis=1)   # T x 4 x 2
    outside = ((P[..., 0] < 0) | (P[..., 0] > F32(width)) | (P[..., 1] < 0) | (P[..., 1] > F32(height))).any(axis=1)
    P = P[~outside]
    if len(P) == 0:
        return None
    prev = np.roll(P, 1, axis=1).astype(np.float64)
    area = np.abs((prev[..., 0] * P[..., 1].astype(np.float64) - prev[..., 1] * P[..., 0].astype(np.float64)).sum(axis=1) * 0.5)
    cand = np.nonzero(_is_contour_convex(P) & (area > 0.0))[0]
    # the largest area wins, of equal areas the first in the loops' order: walk down that order to the first hull of four
    for t in cand[np.lexsort((cand, -area[cand]))]:
        if _hull_size(P[t]) == 4:
            return P[t].copy()
    return None


def hough_line_quad(lines, width, height):
    """4 x 2 int32 (truncated) or None: houghLine.cpp:231-255"""
    lines = np.asarray(lines, F32).reshape(-1, 2)
    if len(lines) < 4:
        return None
    q = find_max_valid_contour(delete_similar_lines(lines), width, height)
    return None if q is None else np.trunc(q).astype(np.int32)


def hough_line_contour(img):
    """(quad or None, number of lines cv::HoughLines found)"""
    edge_map = hough_edges(img)
    lines = hough_lines(edge_map, 50)
    return hough_line_quad(lines, edge_map.shape[1], edge_map.shape[0]), len(lines)
