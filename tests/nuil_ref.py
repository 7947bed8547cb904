"""Restatement of prl::correctNUIL (src/correctNUIL.cpp:33-90) and of the OpenCV calls under it, for the tests: numpy only,
written from the definitions.

  element      cv::getStructuringElement(shape, Size(kw, kh)), anchor (kw/2, kh/2): row i is the half-open column span
               [j1, j2) of element_spans()
  erode/dilate dst(y, x, c) = min / max over the element's set pixels (i, j) of src(y + i - kh/2, x + j - kw/2, c); taps
               outside the page are ignored; the element is not reflected between the two; channels are independent
  morphologyEx OPEN = erode, dilate; CLOSE = dilate, erode; TOPHAT = src - open; BLACKHAT = close - src (saturating); once
  correctNUIL  per channel: x ^ 255 where sum < 128 * W * H (cv::mean < 128), then 255 - blackhat(channel, ellipse(size, size))

[upstream] OpenCV 3.4 / 4.x, unpinned like the rest of the project.  `*_loop` are per-pixel versions for cross-checking.
"""
from __future__ import annotations

import math

import numpy as np

RECT, CROSS, ELLIPSE = 0, 1, 2
ERODE, DILATE, OPEN, CLOSE, TOPHAT, BLACKHAT = 0, 1, 2, 3, 5, 6
OPS = (ERODE, DILATE, OPEN, CLOSE, TOPHAT, BLACKHAT)
SHAPES = (RECT, CROSS, ELLIPSE)


def _as3(img):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3)
    return img if img.ndim == 3 else img[:, :, None]


def cv_round(v):
    """cvRound of a double: to nearest, ties to even"""
    f = math.floor(v)
    d = v - f
    if d > 0.5 or (d == 0.5 and f % 2 == 1):
        return int(f) + 1
    return int(f)


def element_spans(shape, kw, kh):
    if kw < 1 or kh < 1:
        raise ValueError("getStructuringElement: ksize.width > 0 && ksize.height > 0")
    if kw == 1 and kh == 1:
        shape = RECT
    r, c = kh // 2, kw // 2
    inv_r2 = 1.0 / float(r * r) if r else 0.0
    spans = []
    for i in range(kh):
        if shape == RECT or (shape == CROSS and i == r):
            spans.append((0, kw))
        elif shape == CROSS:
            spans.append((c, c + 1))
        else:
            dy = i - r
            if abs(dy) > r:
                spans.append((0, 0))
                continue
            dx = cv_round(c * math.sqrt((r * r - dy * dy) * inv_r2))
            spans.append((max(c - dx, 0), min(c + dx + 1, kw)))
    return spans


def element_mask(shape, kw, kh):
    m = np.zeros((kh, kw), bool)
    for i, (a, b) in enumerate(element_spans(shape, kw, kh)):
        m[i, a:b] = True
    return m


def _pass(a, spans, kw, kh, erode):
    """one erode / dilate of an H x W x C page: every set pixel of the element is one shifted view of the padded page"""
    H, W, C = a.shape
    ay, ax = kh // 2, kw // 2
    pad = 255 if erode else 0
    p = np.full((H + kh - 1, W + kw - 1, C), pad, np.uint8)
    p[ay:ay + H, ax:ax + W] = a
    f = np.minimum if erode else np.maximum
    out = np.full_like(a, pad)
    rows = {}   # rows of the element with the same span share their horizontal part
    for i, (j1, j2) in enumerate(spans):
        if j2 <= j1:
            continue
        if (j1, j2) not in rows:
            h = np.full((H + kh - 1, W, C), pad, np.uint8)
            for j in range(j1, j2):
                f(h, p[:, j:j + W], out=h)
            rows[(j1, j2)] = h
        f(out, rows[(j1, j2)][i:i + H], out=out)
    return out


def erode(img, shape, kw, kh):
    return _pass(_as3(img), element_spans(shape, kw, kh), kw, kh, True).reshape(np.shape(img))


def dilate(img, shape, kw, kh):
    return _pass(_as3(img), element_spans(shape, kw, kh), kw, kh, False).reshape(np.shape(img))


def _sat_sub(a, b):
    return np.clip(a.astype(np.int16) - b.astype(np.int16), 0, 255).astype(np.uint8)


def morphology_ex(img, op, shape, kw, kh):
    a = _as3(img)
    spans = element_spans(shape, kw, kh)
    e = lambda x: _pass(x, spans, kw, kh, True)    # noqa: E731
    d = lambda x: _pass(x, spans, kw, kh, False)   # noqa: E731
    if op == ERODE:
        r = e(a)
    elif op == DILATE:
        r = d(a)
    elif op == OPEN:
        r = d(e(a))
    elif op == CLOSE:
        r = e(d(a))
    elif op == TOPHAT:
        r = _sat_sub(a, d(e(a)))
    elif op == BLACKHAT:
        r = _sat_sub(e(d(a)), a)
    else:
        raise ValueError("unknown morphology operation")
    return r.reshape(np.shape(img))


def channel_inverted(img):
    """per channel: cv::mean < 128, decided in integers"""
    a = _as3(img)
    H, W, C = a.shape
    return [int(a[:, :, c].sum(dtype=np.int64)) < 128 * W * H for c in range(C)]


def correct_nuil(img, size=31, inverted=None):
    a = _as3(img)
    if a.size == 0:
        raise ValueError("Input image for filtration is empty")
    inv = channel_inverted(a) if inverted is None else inverted
    work = a.copy()
    for c, flag in enumerate(inv):
        if flag:
            work[:, :, c] ^= 255
    return (255 - morphology_ex(work, BLACKHAT, ELLIPSE, size, size)).reshape(np.shape(img))


def correct_nuil_rows(img, size, y0, y1):
    """rows [y0, y1) of correct_nuil(img, size), from a band with the two passes' reach on each side"""
    a = _as3(img)
    reach = 2 * (size - 1)
    b0, b1 = max(0, y0 - reach), min(a.shape[0], y1 + reach)
    band = correct_nuil(a[b0:b1], size, inverted=channel_inverted(a))
    return band[y0 - b0:y1 - b0].reshape((y1 - y0,) + np.shape(img)[1:])


def _pass_loop(a, mask, erode):
    H, W, C = a.shape
    kh, kw = mask.shape
    ay, ax = kh // 2, kw // 2
    out = np.empty_like(a)
    taps = [(i, j) for i in range(kh) for j in range(kw) if mask[i, j]]
    for y in range(H):
        for x in range(W):
            for c in range(C):
                v = 255 if erode else 0
                for i, j in taps:
                    yy, xx = y + i - ay, x + j - ax
                    if 0 <= yy < H and 0 <= xx < W:
                        s = int(a[yy, xx, c])
                        v = min(v, s) if erode else max(v, s)
                out[y, x, c] = v
    return out


def morphology_loop(img, op, shape, kw, kh):
    """morphology_ex pixel by pixel, from the element's mask"""
    a = _as3(img)
    m = element_mask(shape, kw, kh)
    first = op in (ERODE, OPEN, TOPHAT)
    r = _pass_loop(a, m, first)
    if op not in (ERODE, DILATE):
        r = _pass_loop(r, m, not first)
    if op == TOPHAT:
        r = np.array([[[max(int(a[y, x, c]) - int(r[y, x, c]), 0) for c in range(a.shape[2])] for x in range(a.shape[1])]
                      for y in range(a.shape[0])], np.uint8).reshape(a.shape)
    if op == BLACKHAT:
        r = np.array([[[max(int(r[y, x, c]) - int(a[y, x, c]), 0) for c in range(a.shape[2])] for x in range(a.shape[1])]
                      for y in range(a.shape[0])], np.uint8).reshape(a.shape)
    return r.reshape(np.shape(img))


def correct_nuil_loop(img, size):
    a = _as3(img).copy()
    H, W, C = a.shape
    for c in range(C):
        if sum(int(v) for v in a[:, :, c].ravel()) / float(W * H) < 128:
            a[:, :, c] = 255 - a[:, :, c]
    return (255 - morphology_loop(a, BLACKHAT, ELLIPSE, size, size)).reshape(np.shape(img))
