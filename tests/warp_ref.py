"""prl::warpCrop's arithmetic (include/prl_hip.h, "perspective crop") restated for the tests: the size rule of warp.cpp:42-53,
cv::getPerspectiveTransform's 8 x 8 LU solve, the closed-form 3 x 3 inversion and cv::warpPerspective(INTER_LINEAR) on 8-bit
pages, twice - one pixel at a time in Python floats (warp_loop) and vectorised in numpy float64 / int64 (warp_numpy).  A third
variant without OpenCV's block rule (warp_numpy(..., block_rule=False): xb = 0, x1 = x) exists only to show that the fixtures
can tell the two apart.  Python floats and numpy float64 are IEEE doubles with one rounding per written operation.
"""
import math

import numpy as np

BORDER_CONSTANT, BORDER_REPLICATE = 0, 1
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
LIMIT = 2.0 ** 500          # largest magnitude of a matrix entry
MAX_SIDE = 32767


class Singular(ValueError):
    pass


# ---- host routines ---------------------------------------------------------------------------------------------------------

def cv_round(v):
    """cvRound: half to even; NaN and values that do not fit an int give INT_MIN (the x86 conversion's answer)."""
    if not (v >= -2147483648.5 and v <= 2147483647.5):
        return INT_MIN
    r = float(np.rint(v))
    if r >= 2147483648.0 or r < -2147483648.0:
        return INT_MIN
    return int(r)


def _wrap32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= (1 << 31) else v


def _side(ax, ay, bx, by):
    """std::sqrt of the int expression (bx-ax)^2 + (by-ay)^2, which wraps like 32-bit two's complement."""
    dx, dy = _wrap32(bx - ax), _wrap32(by - ay)
    e = _wrap32(_wrap32(dx * dx) + _wrap32(dy * dy))
    return math.sqrt(e) if e >= 0 else float("nan")


def _max(a, b):   # std::max(a, b) = a < b ? b : a
    return b if a < b else a


def crop_size(quad, ratio):
    """-> (W, H) of warp.cpp:42-53, before any limit is applied (may be <= 0 or above MAX_SIDE)."""
    x0, y0, x1, y1, x2, y2, x3, y3 = [int(v) for v in quad]
    s1, s2 = _side(x0, y0, x1, y1), _side(x2, y2, x3, y3)
    s3, s4 = _side(x0, y0, x3, y3), _side(x1, y1, x2, y2)
    w, h = cv_round(_max(s1, s2)), cv_round(_max(s3, s4))
    if ratio > 0.0:
        w = cv_round(float(h) / ratio)
    return w, h


def size_ok(w, h):
    return 0 < w <= MAX_SIDE and 0 < h <= MAX_SIDE


def lu_solve(a, b):
    """OpenCV's LU with partial pivoting on Python floats; a (n x n) and b (n) are lists and are destroyed."""
    n = len(b)
    eps = 100 * 2.220446049250313e-16
    for i in range(n):
        k = i
        for j in range(i + 1, n):
            if abs(a[j][i]) > abs(a[k][i]):
                k = j
        if abs(a[k][i]) < eps:
            raise Singular("pivot")
        if k != i:
            a[i], a[k] = a[k], a[i]
            b[i], b[k] = b[k], b[i]
        d = -1 / a[i][i]
        for j in range(i + 1, n):
            alpha = a[j][i] * d
            for c in range(i + 1, n):
                a[j][c] += alpha * a[i][c]
            b[j] += alpha * b[i]
    for i in range(n - 1, -1, -1):
        s = b[i]
        for k in range(i + 1, n):
            s -= a[i][k] * b[k]
        b[i] = s / a[i][i]
    return b


def perspective_transform(src_xy, dst_xy):
    """cv::getPerspectiveTransform: corners through float32, the 8 x 8 system, LU; -> 9 floats, M[8] = 1."""
    s = [float(np.float32(v)) for v in src_xy]
    d = [float(np.float32(v)) for v in dst_xy]
    a = [[0.0] * 8 for _ in range(8)]
    b = [0.0] * 8
    for i in range(4):
        sx, sy, dx, dy = s[2 * i], s[2 * i + 1], d[2 * i], d[2 * i + 1]
        a[i] = [sx, sy, 1.0, 0.0, 0.0, 0.0, -sx * dx, -sy * dx]
        a[i + 4] = [0.0, 0.0, 0.0, sx, sy, 1.0, -sx * dy, -sy * dy]
        b[i], b[i + 4] = dx, dy
    return lu_solve(a, b) + [1.0]


def invert3(m):
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = [float(v) for v in m]
    det = m00 * (m11 * m22 - m12 * m21) - m01 * (m10 * m22 - m12 * m20) + m02 * (m10 * m21 - m11 * m20)
    if det == 0 or det != det:
        raise Singular("det")
    d = 1 / det
    return [(m11 * m22 - m12 * m21) * d, (m02 * m21 - m01 * m22) * d, (m01 * m12 - m02 * m11) * d,
            (m12 * m20 - m10 * m22) * d, (m00 * m22 - m02 * m20) * d, (m02 * m10 - m00 * m12) * d,
            (m10 * m21 - m11 * m20) * d, (m01 * m20 - m00 * m21) * d, (m00 * m11 - m01 * m10) * d]


def matrix_ok(m):
    return all(math.isfinite(v) and abs(v) <= LIMIT for v in m)


def crop_matrix(quad, w, h):
    """the matrix warpCrop hands to cv::warpPerspective (source -> result)"""
    return perspective_transform([float(v) for v in quad], [0.0, 0.0, float(w), 0.0, float(w), float(h), 0.0, float(h)])


def border_bytes(value):
    """saturate_cast<uchar>(borderValue[c])"""
    return [min(255, max(0, cv_round(float(v)))) for v in value]


def block_width(ow, oh):
    return min(1024 // min(16, oh), ow)


# ---- the remap, one pixel at a time ----------------------------------------------------------------------------------------

def _pixel_coords(m, x, y, bw):
    xb = (x // bw) * bw
    x1 = x - xb
    X0 = m[0] * xb + m[1] * y + m[2]
    Y0 = m[3] * xb + m[4] * y + m[5]
    W0 = m[6] * xb + m[7] * y + m[8]
    W = W0 + m[6] * x1
    W = 32.0 / W if W != 0 else 0.0
    out = []
    for base, coef in ((X0, m[0]), (Y0, m[3])):
        f = (base + coef * x1) * W
        f = f if f < 2147483647.0 else 2147483647.0      # std::min(INT_MAX, f): a NaN ends as INT_MAX
        f = f if -2147483648.0 < f else -2147483648.0
        out.append(int(np.rint(f)))
    return out


def warp_loop(src, m, ow, oh, border=BORDER_CONSTANT, value=(0, 0, 0, 0), dst=None):
    """src: H x W x C uint8; m: the INVERTED matrix (result -> source).  -> oh x ow x C (written into dst's corner if given)."""
    h, w, ch = src.shape
    m = [float(v) for v in m]
    cval = border_bytes(value)
    out = np.zeros((oh, ow, ch), np.uint8) if dst is None else dst
    bw = block_width(ow, oh)
    for y in range(oh):
        for x in range(ow):
            X, Y = _pixel_coords(m, x, y, bw)
            sx = max(-32768, min(32767, X >> 5))
            sy = max(-32768, min(32767, Y >> 5))
            fx, fy = X & 31, Y & 31
            wts = (32 * (32 - fx) * (32 - fy), 32 * fx * (32 - fy), 32 * (32 - fx) * fy, 32 * fx * fy)
            taps = ((sx, sy), (sx + 1, sy), (sx, sy + 1), (sx + 1, sy + 1))
            for c in range(ch):
                acc = 0
                for (tx, ty), wt in zip(taps, wts):
                    if border == BORDER_REPLICATE:
                        v = int(src[min(h - 1, max(0, ty)), min(w - 1, max(0, tx)), c])
                    elif 0 <= tx < w and 0 <= ty < h:
                        v = int(src[ty, tx, c])
                    else:
                        v = cval[c]
                    acc += v * wt
                out[y, x, c] = (acc + (1 << 14)) >> 15
    return out


# ---- the remap in numpy ----------------------------------------------------------------------------------------------------

def warp_numpy(src, m, ow, oh, border=BORDER_CONSTANT, value=(0, 0, 0, 0), block_rule=True):
    h, w, ch = src.shape
    m = np.asarray(m, np.float64)
    cval = np.asarray(border_bytes(value)[:ch], np.int64)
    x = np.arange(ow, dtype=np.int64)[None, :]
    y = np.arange(oh, dtype=np.float64)[:, None]
    bw = block_width(ow, oh) if block_rule else max(ow, 1) + 1
    xb = ((x // bw) * bw).astype(np.float64)
    x1 = (x % bw).astype(np.float64)
    with np.errstate(all="ignore"):
        X0 = m[0] * xb + m[1] * y + m[2]
        Y0 = m[3] * xb + m[4] * y + m[5]
        W0 = m[6] * xb + m[7] * y + m[8]
        W = W0 + m[6] * x1
        W = np.where(W != 0, 32.0 / np.where(W != 0, W, 1.0), 0.0)

        def fixed(base, coef):
            f = (base + coef * x1) * W
            f = np.where(f < 2147483647.0, f, 2147483647.0)
            f = np.where(-2147483648.0 < f, f, -2147483648.0)
            return np.rint(f).astype(np.int64)

        X, Y = fixed(X0, m[0]), fixed(Y0, m[3])
    sx, sy = np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)
    fx, fy = X & 31, Y & 31
    acc = np.zeros((oh, ow, ch), np.int64)
    s64 = src.astype(np.int64)
    for dx, dy, wt in ((0, 0, 32 * (32 - fx) * (32 - fy)), (1, 0, 32 * fx * (32 - fy)), (0, 1, 32 * (32 - fx) * fy), (1, 1, 32 * fx * fy)):
        tx, ty = sx + dx, sy + dy
        v = s64[np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1)]
        if border != BORDER_REPLICATE:
            inside = (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
            v = np.where(inside[:, :, None], v, cval[None, None, :])
        acc += v * wt[:, :, None]
    return ((acc + (1 << 14)) >> 15).astype(np.uint8)


def warp_perspective(src, m, ow, oh, inverse_map=False, border=BORDER_CONSTANT, value=(0, 0, 0, 0), block_rule=True):
    """cv::warpPerspective(src, M, Size(ow, oh), INTER_LINEAR [| WARP_INVERSE_MAP], border, value), numpy restatement"""
    s = src if src.ndim == 3 else src[:, :, None]
    mi = [float(v) for v in m] if inverse_map else invert3(m)
    out = warp_numpy(s, mi, ow, oh, border, value, block_rule)
    return out if src.ndim == 3 else out[:, :, 0]


def warp_crop(src, quad, ratio=-1.0, border=BORDER_CONSTANT, value=(0, 0, 0, 0)):
    w, h = crop_size(quad, ratio)
    if not size_ok(w, h):
        raise ValueError("size")
    return warp_perspective(src, crop_matrix(quad, w, h), w, h, False, border, value)


# ---- fixtures --------------------------------------------------------------------------------------------------------------

OUT_H = (1, 3, 16, 17)
OUT_W = (1, 63, 64, 65, 257, 400)
SIZES = [(ow, oh) for oh in OUT_H for ow in OUT_W]
SOURCES = [(67, 45), (300, 130)]   # width, height


def multi_block(ow, oh):
    return block_width(ow, oh) < ow


def _rng(name):
    return np.random.default_rng(sum(ord(c) * (i + 1) for i, c in enumerate(name)) + 20240613)


def _mild(sw, sh, ow, oh, name):
    e = _rng(name).uniform(-1, 1, 6)
    return [sw / ow * (0.9 + 0.05 * e[0]), 0.11 * e[1], 1.5 + e[2],
            0.07 * e[3], sh / oh * (0.9 + 0.05 * e[4]), 0.7 + e[5],
            0.1 / ow, 0.06 / oh, 1.0]


def _horizon(sw, sh, ow, oh, name):
    # W = 1 - x / 8 is exactly 0 at x = 8 (the `W ? 32 / W : 0` branch) and changes sign there
    e = _rng(name).uniform(-1, 1, 2)
    return [sw / 40.0, 0.3 * e[0], 3.0, 0.2 * e[1], sh / 30.0, 2.0, -0.125, 0.0, 1.0]


def _outside(sw, sh, ow, oh, name):
    e = _rng(name).uniform(0, 1, 2)
    return [2.0 * sw / ow, 0.0, -0.9 * sw - e[0], 0.0, 2.5 * sh / oh, -0.8 * sh - e[1], 0.0, 0.0, 1.0]


def _huge(sw, sh, ow, oh, name):
    # 32 X leaves the int range on both sides: fX is clamped to -2^31 / 2^31 - 1, sx to -32768 / 32767
    return [3.0e7, 0.0, -3.0e9, 0.0, 2.0e8, -1.0e9, 0.0, 0.0, 1.0]


def _far(sw, sh, ow, oh, name):
    # X >> 5 leaves the short range (sx clamps) while 32 X still fits an int
    return [3000.0, 0.0, -90000.0, 0.0, 0.5, 1.25, 0.0, 0.0, 1.0]


def _cancel(sw, sh, ow, oh, name):
    # Row `r` only: 2^45 y + C cancels to a small number there.  With the block rule M[0] xb is added to 2^45 r first and is
    # rounded to that magnitude's grid (1/64 or coarser: the fixed-point coordinate moves by up to a quarter); without it
    # the cancellation happens first and M[0] x is added exactly.  The fixture that tells the two models apart (0.1549 was
    # picked so that the single second-block pixel of a 65-pixel row is among the pixels that differ).
    r = min(2, oh - 1)
    big = 2.0 ** 45
    return [0.1549, big, 5.3 - big * r, 0.0, 0.41, 3.3, 0.0, 0.0, 1.0]


# name -> (builder of the result -> source map, how it reaches the entry: inverse_map flag)
_BUILDERS = [("mild", _mild, 0), ("horizon", _horizon, 0), ("outside", _outside, 0), ("huge", _huge, 1), ("far", _far, 0),
             ("mild_inverse", _mild, 1), ("cancel", _cancel, 1)]
MATRICES = [name for name, _, _ in _BUILDERS]


def matrix_case(name, sw, sh, ow, oh):
    """-> (M as handed to the entry, inverse_map).  With inverse_map = 0 the entry (and warp_perspective) inverts M itself."""
    for n, fn, inv in _BUILDERS:
        if n == name:
            d = [float(v) for v in fn(sw, sh, ow, oh, name)]
            return (d, 1) if inv else (invert3(d), 0)
    raise KeyError(name)


# ---- page families (the style of mokji_ref.families) -------------------------------------------------------------------------

def noise_page(w, h, ch, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, ch), dtype=np.uint8)


def text_page(w, h, ch, seed):
    """two levels, text-like: dark runs on a light page"""
    rng = np.random.default_rng(seed)
    p = np.full((h, w), 230, np.uint8)
    for y in range(2, h - 2, 5):
        x = int(rng.integers(1, 6))
        while x < w - 2:
            n = int(rng.integers(2, 9))
            p[y:y + 3, x:min(w - 1, x + n)] = 25
            x += n + int(rng.integers(1, 5))
    return np.repeat(p[:, :, None], ch, axis=2)


def gradient_page(w, h, ch, seed):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([((xx * (3 + c) + yy * (7 - c) + seed) % 256).astype(np.uint8) for c in range(ch)], axis=2)


def flat_page(w, h, ch, v):
    return np.full((h, w, ch), v, np.uint8)


def families(w, h, ch=1, seed=1):
    return [("noise", noise_page(w, h, ch, seed)), ("text", text_page(w, h, ch, seed)), ("gradient", gradient_page(w, h, ch, seed)),
            ("flat", flat_page(w, h, ch, 77))]
