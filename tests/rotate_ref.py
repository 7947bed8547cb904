"""prl::rotate's arithmetic (include/prl_hip.h, "rotate") restated for the tests from the operation's definition: the quarter-turn
branches of rotate.cpp:37-57 (cv::transpose + cv::flip), and for every other angle cv::getRotationMatrix2D about the centre of the
max(w, h) square, cv::warpAffine's inversion of that matrix and its INTER_LINEAR remap of the inverted page on 8-bit pixels - twice:
one pixel at a time in Python floats and ints (rotate_loop) and whole planes in numpy float64 / int64 (rotate_numpy).  Python floats
and numpy float64 are IEEE doubles with one rounding per written operation; math.cos / math.sin are the C library's.

    kind(angle)                 0 general, 1 / 2 / 3 for 90 / 180 / 270 within 1e-7 after fmod(angle, 360)
    out_size(w, h, angle)       (ow, oh)
    matrix(w, h, angle)         the six float64 of the inverted matrix, dst -> src
    rotate_loop(img, angle, rows=None)     H x W or H x W x C uint8 -> oh x ow (x C); rows: only these output rows, in that order
    rotate_numpy(img, angle)
"""
import math

import numpy as np

AB_BITS = 10                 # warpAffine's coordinate fraction bits
INTER_BITS = 5               # of which the bilinear weights keep this many
AB_SCALE = 1 << AB_BITS
INTER_TAB = 1 << INTER_BITS  # 32
ROUND_DELTA = AB_SCALE // INTER_TAB // 2   # 16: rounds the 10-bit coordinate to its nearest 5-bit one
REMAP_BITS = 15              # the four weights add up to 2^15
EQ_DELTA = 1e-7


def kind(angle):
    a = math.fmod(angle, 360.0)      # keeps the sign of `angle`: -90 stays -90
    if abs(a - 90.0) <= EQ_DELTA:
        return 1
    if abs(a - 180.0) <= EQ_DELTA:
        return 2
    if abs(a - 270.0) <= EQ_DELTA:
        return 3
    return 0


def out_size(w, h, angle):
    k = kind(angle)
    if k in (1, 3):
        return h, w
    if k == 2:
        return w, h
    return max(w, h), max(w, h)


def matrix(w, h, angle):
    """getRotationMatrix2D(Point2f(len/2, len/2), angle, 1.0), then warpAffine's invertAffineTransform (no WARP_INVERSE_MAP)."""
    ln = max(w, h)
    cx = cy = float(np.float32(ln / 2.0))
    a = math.fmod(angle, 360.0)
    a = a * (math.pi / 180)
    alpha, beta = math.cos(a) * 1.0, math.sin(a) * 1.0
    m = [alpha, beta, (1 - alpha) * cx - beta * cy,
         -beta, alpha, beta * cx + (1 - alpha) * cy]
    d = m[0] * m[4] - m[1] * m[3]
    d = 1.0 / d if d != 0 else 0.0
    a11, a22 = m[4] * d, m[0] * d
    m[0] = a11
    m[1] = m[1] * -d
    m[3] = m[3] * -d
    m[4] = a22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return m


def _rint(v):
    return int(np.rint(v))       # half to even, as the conversion instruction does


def _planes(img):
    a = img if img.ndim == 3 else img[:, :, None]
    assert a.dtype == np.uint8 and 1 <= a.shape[2] <= 4
    return a


def _quarter(a, k):
    if k == 1:
        return a.swapaxes(0, 1)[:, ::-1]      # cv::transpose, cv::flip(1): around the vertical axis
    if k == 2:
        return a[::-1, ::-1]                  # cv::flip(-1): both axes
    return a.swapaxes(0, 1)[::-1]             # cv::transpose, cv::flip(0): around the horizontal axis


def rotate_loop(img, angle, rows=None):
    a = _planes(img)
    h, w, ch = a.shape
    k = kind(angle)
    ow, oh = out_size(w, h, angle)
    ys = list(range(oh)) if rows is None else list(rows)
    out = np.empty((len(ys), ow, ch), np.uint8)
    if k:
        for n, y in enumerate(ys):
            for x in range(ow):
                if k == 1:
                    t = a.swapaxes(0, 1)      # t[y][x] = a[x][y]; flipped left-right: column ow - 1 - x
                    out[n, x] = t[y, ow - 1 - x]
                elif k == 2:
                    out[n, x] = a[h - 1 - y, w - 1 - x]
                else:
                    t = a.swapaxes(0, 1)      # flipped upside down: row oh - 1 - y
                    out[n, x] = t[oh - 1 - y, x]
        return out if img.ndim == 3 else out[:, :, 0]
    m = matrix(w, h, angle)
    inv = 255 - a.astype(np.int64)            # cv::bitwise_not(input)
    adelta = [_rint(m[0] * x * AB_SCALE) for x in range(ow)]
    bdelta = [_rint(m[3] * x * AB_SCALE) for x in range(ow)]

    def tap(yy, xx):
        return inv[yy, xx] if 0 <= yy < h and 0 <= xx < w else 0      # BORDER_CONSTANT, value 0

    for n, y in enumerate(ys):
        x0 = _rint((m[1] * y + m[2]) * AB_SCALE) + ROUND_DELTA
        y0 = _rint((m[4] * y + m[5]) * AB_SCALE) + ROUND_DELTA
        for x in range(ow):
            X = (x0 + adelta[x]) >> (AB_BITS - INTER_BITS)
            Y = (y0 + bdelta[x]) >> (AB_BITS - INTER_BITS)
            sx = max(-32768, min(32767, X >> INTER_BITS))             # saturate_cast<short>
            sy = max(-32768, min(32767, Y >> INTER_BITS))
            fx, fy = X & (INTER_TAB - 1), Y & (INTER_TAB - 1)
            # the weight table: the 2 x 2 products of (1 - f, f) in 1/32 steps, scaled to 2^15 (exact: 32 * 32 * 32)
            w00, w01 = 32 * (32 - fx) * (32 - fy), 32 * fx * (32 - fy)
            w10, w11 = 32 * (32 - fx) * fy, 32 * fx * fy
            s = tap(sy, sx) * w00 + tap(sy, sx + 1) * w01 + tap(sy + 1, sx) * w10 + tap(sy + 1, sx + 1) * w11
            out[n, x] = 255 - ((s + (1 << (REMAP_BITS - 1))) >> REMAP_BITS)    # the second bitwise_not
    return out if img.ndim == 3 else out[:, :, 0]


def rotate_numpy(img, angle):
    a = _planes(img)
    h, w, ch = a.shape
    k = kind(angle)
    if k:
        out = np.ascontiguousarray(_quarter(a, k))
        return out if img.ndim == 3 else out[:, :, 0]
    ln = max(w, h)
    m = matrix(w, h, angle)
    xs, ys = np.arange(ln, dtype=np.float64), np.arange(ln, dtype=np.float64)
    adelta = np.rint(m[0] * xs * AB_SCALE).astype(np.int64)
    bdelta = np.rint(m[3] * xs * AB_SCALE).astype(np.int64)
    x0 = np.rint((m[1] * ys + m[2]) * AB_SCALE).astype(np.int64) + ROUND_DELTA
    y0 = np.rint((m[4] * ys + m[5]) * AB_SCALE).astype(np.int64) + ROUND_DELTA
    X = (x0[:, None] + adelta[None, :]) >> (AB_BITS - INTER_BITS)
    Y = (y0[:, None] + bdelta[None, :]) >> (AB_BITS - INTER_BITS)
    sx = np.clip(X >> INTER_BITS, -32768, 32767)
    sy = np.clip(Y >> INTER_BITS, -32768, 32767)
    fx, fy = X & (INTER_TAB - 1), Y & (INTER_TAB - 1)
    # the inverted page with a frame of zeros: every tap that can carry weight lies in rows -1 .. h and columns -1 .. w
    padded = np.zeros((h + 2, w + 2, ch), np.int64)
    padded[1:h + 1, 1:w + 1] = 255 - a.astype(np.int64)
    acc = np.zeros((ln, ln, ch), np.int64)
    for dy, dx, wt in ((0, 0, 32 * (32 - fx) * (32 - fy)), (0, 1, 32 * fx * (32 - fy)),
                       (1, 0, 32 * (32 - fx) * fy), (1, 1, 32 * fx * fy)):
        yy, xx = sy + dy, sx + dx
        inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        v = padded[np.where(inside, yy + 1, 0), np.where(inside, xx + 1, 0)]     # (0, 0) of `padded` is a zero
        acc += v * wt[:, :, None]
    out = (255 - ((acc + (1 << (REMAP_BITS - 1))) >> REMAP_BITS)).astype(np.uint8)
    return out if img.ndim == 3 else out[:, :, 0]
