"""Restatement of cv::pyrDown, cv::Canny (8UC1, apertureSize 3, L1 magnitude), the edge map of prl::documentContour and the index
tables of prl::resize's scale path, as include/prl_hip.h states them ("pyramid, edge map, resize").  Test code: two models of
every routine written independently of each other, a vectorised one (numpy, what the GPU tests compare with) and a per-pixel
one (*_loop: plain Python on ints, the definitions read off line by line); test_edges_cpu.py holds them against each other and
against answers worked out by hand.
"""
import math

import numpy as np

TG22 = 13573   # tan(22.5 deg) * 2^15, rounded


# ---- cv::borderInterpolate(p, len, BORDER_REFLECT_101) ---------------------------------------------------------------------------

def reflect101(p, n):
    if 0 <= p < n:
        return p
    if n == 1:
        return 0
    while not 0 <= p < n:
        p = -p if p < 0 else 2 * n - 2 - p
    return p


def reflect101_table(idx, n):
    """the same for an int array, by the closed form of the repeated fold (period 2 n - 2)"""
    idx = np.asarray(idx, np.int64)
    if n == 1:
        return np.zeros_like(idx)
    q = np.mod(idx, 2 * n - 2)
    return np.where(q < n, q, 2 * n - 2 - q)


# ---- cv::pyrDown -------------------------------------------------------------------------------------------------------------------

def pyr_down(img, levels=1):
    """H x W [x C] uint8 -> (H+1)/2 x (W+1)/2 [x C], `levels` times"""
    a = img if img.ndim == 3 else img[:, :, None]
    for _ in range(levels):
        h, w, _c = a.shape
        oh, ow = (h + 1) // 2, (w + 1) // 2
        s = a.astype(np.int32)   # (v <= 65280)
        cols = [reflect101_table(2 * np.arange(ow) + d, w) for d in (-2, -1, 0, 1, 2)]
        r = s[:, cols[0]] + 4 * s[:, cols[1]] + 6 * s[:, cols[2]] + 4 * s[:, cols[3]] + s[:, cols[4]]
        rows = [reflect101_table(2 * np.arange(oh) + d, h) for d in (-2, -1, 0, 1, 2)]
        v = r[rows[0]] + 4 * r[rows[1]] + 6 * r[rows[2]] + 4 * r[rows[3]] + r[rows[4]]
        a = ((v + 128) >> 8).astype(np.uint8)
    return a if img.ndim == 3 else a[:, :, 0]


def pyr_down_loop(img):
    """one level, pixel by pixel"""
    a = img if img.ndim == 3 else img[:, :, None]
    h, w, ch = a.shape
    oh, ow = (h + 1) // 2, (w + 1) // 2
    out = np.zeros((oh, ow, ch), np.uint8)
    k = (1, 4, 6, 4, 1)
    for y in range(oh):
        for x in range(ow):
            for c in range(ch):
                v = 0
                for i in range(5):
                    sy = reflect101(2 * y - 2 + i, h)
                    rs = 0
                    for j in range(5):
                        rs += k[j] * int(a[sy, reflect101(2 * x - 2 + j, w), c])
                    v += k[i] * rs
                out[y, x, c] = (v + 128) >> 8
    return out if img.ndim == 3 else out[:, :, 0]


# ---- cv::Canny ---------------------------------------------------------------------------------------------------------------------

def canny_thresholds(t1, t2):
    """(low, high) as cv::Canny reads them; a NaN has no answer"""
    assert not (math.isnan(t1) or math.isnan(t2))
    if t1 > t2:
        t1, t2 = t2, t1
    clamp = lambda v: int(min(2041.0, max(-1.0, float(math.floor(v)) if math.isfinite(v) else v)))
    return clamp(t1), clamp(t2)


def direction(dx, dy):
    """the branch of the non-maximum suppression: 0 = horizontal neighbours, 1 = vertical, 2 = the diagonal of sign(dx ^ dy)"""
    ax, ay = abs(dx), abs(dy) << 15
    t = ax * TG22
    return 0 if ay < t else 1 if ay > t + (ax << 16) else 2


def gradients(img):
    """dx, dy (Sobel 3 x 3, BORDER_REPLICATE) and m = |dx| + |dy| padded by one ring of zeros"""
    p = np.pad(img.astype(np.int64), 1, mode="edge")
    dx = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])
    dy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])
    return dx, dy, np.pad(np.abs(dx) + np.abs(dy), 1)


def canny_classes(img, t1, t2, with_branch=False):
    """OpenCV's map codes: 2 = edge, 0 = candidate, 1 = neither.  with_branch: also 0 / 1 / 2 = horizontal / vertical / diagonal"""
    low, high = canny_thresholds(t1, t2)
    dx, dy, mp = gradients(img)
    h, w = img.shape
    m = mp[1:-1, 1:-1]
    at = lambda oy, ox: mp[1 + oy:1 + oy + h, 1 + ox:1 + ox + w]
    ax, ay = np.abs(dx), np.abs(dy) << 15
    t = ax * TG22
    horiz = ay < t
    vert = ~horiz & (ay > t + (ax << 16))
    s_neg = (dx ^ dy) < 0
    # s = -1: (x + 1, y - 1) and (x - 1, y + 1); s = +1: (x - 1, y - 1) and (x + 1, y + 1)
    diag_max = np.where(s_neg, (m > at(-1, 1)) & (m > at(1, -1)), (m > at(-1, -1)) & (m > at(1, 1)))
    is_max = np.where(horiz, (m > at(0, -1)) & (m >= at(0, 1)), np.where(vert, (m > at(-1, 0)) & (m >= at(1, 0)), diag_max)) & (m > low)
    cls = np.where(is_max, np.where(m > high, 2, 0), 1).astype(np.uint8)
    if with_branch:
        return cls, np.where(horiz, 0, np.where(vert, 1, 2)).astype(np.uint8)
    return cls


def canny_classes_loop(img, t1, t2):
    low, high = canny_thresholds(t1, t2)
    h, w = img.shape
    px = lambda x, y: int(img[min(max(y, 0), h - 1), min(max(x, 0), w - 1)])

    def grad(x, y):
        gx = (px(x + 1, y - 1) + 2 * px(x + 1, y) + px(x + 1, y + 1)) - (px(x - 1, y - 1) + 2 * px(x - 1, y) + px(x - 1, y + 1))
        gy = (px(x - 1, y + 1) + 2 * px(x, y + 1) + px(x + 1, y + 1)) - (px(x - 1, y - 1) + 2 * px(x, y - 1) + px(x + 1, y - 1))
        return gx, gy

    def mag(x, y):
        if not (0 <= x < w and 0 <= y < h):
            return 0
        gx, gy = grad(x, y)
        return abs(gx) + abs(gy)

    out = np.ones((h, w), np.uint8)
    for y in range(h):
        for x in range(w):
            gx, gy = grad(x, y)
            m = abs(gx) + abs(gy)
            if not m > low:
                continue
            ax, ay = abs(gx), abs(gy) * 32768
            t = ax * TG22
            if ay < t:
                ok = m > mag(x - 1, y) and m >= mag(x + 1, y)
            elif ay > t + ax * 65536:
                ok = m > mag(x, y - 1) and m >= mag(x, y + 1)
            else:
                s = -1 if (gx < 0) != (gy < 0) else 1   # the sign bit of dx ^ dy
                ok = m > mag(x - s, y - 1) and m > mag(x + s, y + 1)
            if ok:
                out[y, x] = 2 if m > high else 0
    return out


def edge_link(cls):
    """255 where class 2, or class 0 reaching a class 2 through 8-connected class 0: a breadth-first walk on index arrays"""
    h, w = cls.shape
    out = cls == 2
    free = cls == 0
    fy, fx = np.nonzero(out)
    while fy.size:
        ny = (fy[:, None] + np.array([-1, -1, -1, 0, 0, 1, 1, 1])).ravel()
        nx = (fx[:, None] + np.array([-1, 0, 1, -1, 1, -1, 0, 1])).ravel()
        ok = (ny >= 0) & (ny < h) & (nx >= 0) & (nx < w)
        ny, nx = ny[ok], nx[ok]
        ok = free[ny, nx]
        ny, nx = ny[ok], nx[ok]
        free[ny, nx] = False   # (duplicates are marked once, and leave the next frontier through np.unique)
        out[ny, nx] = True
        flat = np.unique(ny * w + nx)
        fy, fx = flat // w, flat % w
    return np.where(out, 255, 0).astype(np.uint8)


def edge_link_loop(cls):
    """OpenCV's walk: a stack of the class-2 pixels, every popped pixel promotes its class-0 neighbours"""
    h, w = cls.shape
    m = [[int(v) for v in row] for row in cls]
    stack = [(y, x) for y in range(h) for x in range(w) if m[y][x] == 2]
    while stack:
        y, x = stack.pop()
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                yy, xx = y + oy, x + ox
                if 0 <= yy < h and 0 <= xx < w and m[yy][xx] == 0:
                    m[yy][xx] = 2
                    stack.append((yy, xx))
    return np.array([[255 if v == 2 else 0 for v in row] for row in m], np.uint8).reshape(h, w)


def canny(img, t1, t2):
    return edge_link(canny_classes(img, t1, t2))


def canny_loop(img, t1, t2):
    return edge_link_loop(canny_classes_loop(img, t1, t2))


# ---- the edge map of prl::documentContour (autoCrop.cpp:67-101) -------------------------------------------------------------------

def document_edges_geometry(w, h):
    levels, long_side = 0, max(w, h)
    while long_side // 2 >= 256:
        w, h = (w + 1) // 2, (h + 1) // 2
        long_side = max(w, h)
        levels += 1
    return levels, w, h


def most_informative_channel(img):
    """the first maximum of cv::meanStdDev's standard deviations, from the per-channel histograms in float64"""
    a = img if img.ndim == 3 else img[:, :, None]
    n = float(a.shape[0] * a.shape[1])
    best, best_sd = 0, None
    for c in range(a.shape[2]):
        hist = np.bincount(a[:, :, c].ravel(), minlength=256)
        s1 = sum(int(hist[v]) * v for v in range(256))
        s2 = sum(int(hist[v]) * v * v for v in range(256))
        mean = float(s1) / n
        sd = math.sqrt(max(float(s2) / n - mean * mean, 0.0))
        if best_sd is None or best_sd < sd:
            best, best_sd = c, sd
    return best


def document_edges(img):
    """(edge map, chosen channel)"""
    a = img if img.ndim == 3 else img[:, :, None]
    levels, _w, _h = document_edges_geometry(a.shape[1], a.shape[0])
    small = pyr_down(a, levels) if levels else a
    ch = most_informative_channel(small)
    return canny(np.ascontiguousarray(small[:, :, ch]), 25.0, 50.0), ch


def colour_from_gray(g, channels=3):
    """a colour page made from a gray one, its channels of different spread: g / 2 + 64, g, 255 - g [, 255]"""
    planes = [(g >> 1) + 64, g, 255 - g, np.full_like(g, 255)]
    return np.ascontiguousarray(np.stack(planes[:channels], axis=2).astype(np.uint8))


# ---- prl::resize (resize.cpp:29-62) ---------------------------------------------------------------------------------------------

def resize_pyramid_levels(w, h, max_size):
    assert max_size >= 1
    levels = 0
    while max(w, h) > max_size:
        w, h = (w + 1) // 2, (h + 1) // 2
        levels += 1
    return levels, w, h


def replicate_table(n, scale):
    """source index of every result index: floor(d * (1.0 / scale)) in float64, clamped to the last source index"""
    inv = 1.0 / float(scale)
    return np.array([min(int(math.floor(float(d) * inv)), n - 1) for d in range(n * scale)], np.int64)


def resize(img, scale_x, scale_y, max_size):
    if scale_x > 0 and scale_y > 0:
        return np.ascontiguousarray(img[replicate_table(img.shape[0], scale_y)][:, replicate_table(img.shape[1], scale_x)])
    levels = resize_pyramid_levels(img.shape[1], img.shape[0], max_size)[0]
    return pyr_down(img, levels) if levels else img.copy()
