"""Restatement of prl::removeLines (src/removeLines.cpp:30-76) for the tests, composed from what the project already pins:

  gray    oracle.bgr2gray (the 14-bit luma) for 3 channels, else the page
  bw      inv = 255 - gray; t = oracle.otsu(inv) (getThreshVal_Otsu_8u); bw = inv > t ? 255 : 0
  open    erode then dilate of tests/nuil_ref.py with RECT (W // 50) x 1 and RECT 1 x (H // 50): anchor k // 2, taps outside the
          page ignored by both, the element not reflected
  out     255 - ((bw - horizontal) - vertical), saturating

Beside it an independent run-length model of the two openings (open_runs), the input families the CPU and GPU tests share, and
an emulation in numpy uint64 of the word algorithm of prlib_amd/csrc/lines.hip (emulate_words): the same tile geometry, shifted
loads, doubling steps, funnel shifts, pad values and masks, so that the algorithm is checked where no device is.
"""
from __future__ import annotations

import numpy as np

import nuil_ref as nr

MIN_SIDE = 50

# width x height: the places the bit kernels can break (see tests/test_lines_gpu.py)
SIZES = [(50, 50), (99, 120), (100, 100), (150, 150),
         (3150, 64), (3200, 65), (3250, 63), (64, 3150), (65, 3200), (63, 3250),
         (6450, 130), (13000, 60), (60, 13000), (1031, 517)]


def element_lengths(w, h):
    return w // 50, h // 50


def gray_of(img):
    from oracle import capi as oracle

    img = np.asarray(img)
    if img.ndim == 3 and img.shape[2] == 3:
        return oracle.bgr2gray(np.ascontiguousarray(img))
    if img.ndim == 3 and img.shape[2] == 1:
        return np.ascontiguousarray(img[:, :, 0])
    if img.ndim != 2:
        raise ValueError("removeLines: 1 or 3 channels")   # cv::threshold(THRESH_OTSU) takes 8UC1 only
    return np.ascontiguousarray(img)


def mask_of(gray):
    """bw (bool) and the Otsu threshold of the inverted page"""
    from oracle import capi as oracle

    inv = np.ascontiguousarray(255 - gray)
    t, _ = oracle.otsu(inv)
    return inv > t, int(t)


def _check_size(w, h):
    if w < MIN_SIDE or h < MIN_SIDE:
        raise ValueError("getStructuringElement: ksize.width > 0 && ksize.height > 0")


def openings(bw):
    """horizontal and vertical opening (bool) of a bool mask, by nuil_ref's erode / dilate"""
    h, w = bw.shape
    _check_size(w, h)
    L, Lv = element_lengths(w, h)
    b = np.where(bw, 255, 0).astype(np.uint8)
    hor = nr.dilate(nr.erode(b, nr.RECT, L, 1), nr.RECT, L, 1)
    ver = nr.dilate(nr.erode(b, nr.RECT, 1, Lv), nr.RECT, 1, Lv)
    return hor > 0, ver > 0


def compose(bw, hor, ver):
    b = np.where(bw, 255, 0).astype(np.uint8)
    r = nr._sat_sub(nr._sat_sub(b, np.where(hor, 255, 0).astype(np.uint8)), np.where(ver, 255, 0).astype(np.uint8))
    return (255 - r).astype(np.uint8)


def remove_lines(img):
    gray = gray_of(img)
    _check_size(gray.shape[1], gray.shape[0])
    bw, _ = mask_of(gray)
    hor, ver = openings(bw)
    return compose(bw, hor, ver)


# ---- the run-length model ------------------------------------------------------------------------------------------------

def open_line_runs(line, k):
    """erode then dilate of a 1-D bool line with k taps at the offsets -k//2 .. k-1-k//2, taps outside ignored: per run of set
    pixels [s, e) (a run touching a border counts as reaching past it) the eroded pixels are [s + a, e - k + a], and each eroded
    interval [p, q] dilates to [p - (k - 1 - a), q + a]"""
    n = line.shape[0]
    a = k // 2
    out = np.zeros(n, bool)
    x = 0
    far = 4 * (n + k)
    while x < n:
        if not line[x]:
            x += 1
            continue
        s = x
        while x < n and line[x]:
            x += 1
        e = x
        s_ext = -far if s == 0 else s
        e_ext = far if e == n else e
        p, q = max(s_ext + a, 0), min(e_ext - k + a, n - 1)
        if p <= q:
            out[max(p - (k - 1 - a), 0):min(q + a, n - 1) + 1] = True
    return out


def open_runs(bw, k, axis):
    out = np.zeros_like(bw)
    if axis == 1:
        for y in range(bw.shape[0]):
            out[y] = open_line_runs(bw[y], k)
    else:
        for x in range(bw.shape[1]):
            out[:, x] = open_line_runs(bw[:, x], k)
    return out


def remove_lines_runs(img):
    gray = gray_of(img)
    h, w = gray.shape
    _check_size(w, h)
    bw, _ = mask_of(gray)
    L, Lv = element_lengths(w, h)
    keep = bw & ~open_runs(bw, L, 1) & ~open_runs(bw, Lv, 0)
    return np.where(keep, 0, 255).astype(np.uint8)


# ---- input families ------------------------------------------------------------------------------------------------------

PAPER, INK = 225, 30


def _page(w, h, ink):
    return np.where(ink, INK, PAPER).astype(np.uint8)


def stroke_pages(w, h):
    """1-pixel strokes of length k-2 .. k+2: starting at 0, ending at the far border, and starting at offsets = 0, 1, 63 (mod 64)"""
    L, Lv = element_lengths(w, h)
    hor = np.zeros((h, w), bool)
    i = 0
    for n in range(max(L - 2, 1), L + 3):
        mid = (w // 2) // 64 * 64
        for start in (0, w - n, mid, mid + 1, mid + 63):
            y = (2 * i + 1) % h
            i += 1
            s = max(0, min(start, w - n))
            hor[y, s:s + n] = True
    ver = np.zeros((h, w), bool)
    i = 0
    for n in range(max(Lv - 2, 1), Lv + 3):
        mid = (h // 2) // 64 * 64
        for start in (0, h - n, mid, mid + 1, mid + 63):
            x = (2 * i + 1) % w
            i += 1
            s = max(0, min(start, h - n))
            ver[s:s + n, x] = True
    return [_page(w, h, hor), _page(w, h, ver), _page(w, h, hor | ver)]


def table_page(w, h, seed):
    """crossing rules plus short text-like strokes, on slightly noisy paper"""
    rng = np.random.default_rng(seed)
    L, Lv = element_lengths(w, h)
    ink = np.zeros((h, w), bool)
    for y in range(h // 7, h, max(h // 5, 2)):
        ink[y:y + 1 + (y % 2), w // 20:w - w // 20] = True
    for x in range(w // 6, w, max(w // 4, 2)):
        ink[h // 20:h - h // 20, x:x + 1 + (x % 2)] = True
    for _ in range(max(8, w * h // 4000)):
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        if rng.random() < 0.5:
            ink[y, x:x + int(rng.integers(1, max(L, 2)))] = True
        else:
            ink[y:y + int(rng.integers(1, max(Lv, 2))), x] = True
    page = _page(w, h, ink).astype(np.int16) + rng.integers(-12, 13, size=(h, w))
    return np.clip(page, 0, 255).astype(np.uint8)


def families(w, h, seed=0):
    """(name, gray page) for one size"""
    rng = np.random.default_rng(1000 * seed + w + 7 * h)
    out = [(f"strokes{i}", p) for i, p in enumerate(stroke_pages(w, h))]
    for dens in (0.3, 0.9, 0.99):
        out.append((f"ink{dens}", _page(w, h, rng.random((h, w)) < dens)))
    out.append(("flat0", np.zeros((h, w), np.uint8)))
    out.append(("flat255", np.full((h, w), 255, np.uint8)))
    two = np.full((h, w), 200, np.uint8)
    two[h // 3:, : 2 * w // 3] = 90
    out.append(("two_level", two))
    out.append(("table", table_page(w, h, seed + 1)))
    return out


def tie_page(mid=4, w=160, h=128):
    """two equal classes (100 / 150) and `mid` isolated pixels half-way (125): Otsu's between-class variance is, up to float64
    rounding, the same for every threshold between a class and the middle on either side, so where the first maximum falls
    depends on the end the scan starts from.  mid = 4: t(inv) = 105 where the mirror of t(gray) = 100 is 154; mid = 8: 130 / 129."""
    p = np.full((h, w), 100, np.uint8)
    p[:, w // 2:] = 150
    for j in range(mid // 2):
        p[1, 10 + 3 * j] = 125
        p[1, w // 2 + 10 + 3 * j] = 125
    return p


# ---- the word algorithm of lines.hip, in numpy uint64 --------------------------------------------------------------------

LDS_WORDS, H_WORDS = 3840, 2048
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def geometry(w, h):
    """ln_geom of lines.hip"""
    L, Lv = element_lengths(w, h)
    wp = (w + 63) // 64
    P = (w + 2 * (L - 1) + 63) // 64
    nr_ = max(1, min(H_WORDS // P, h))
    halo = 2 * (Lv - 1)
    cw = 32
    while True:
        th = LDS_WORDS // cw - halo
        if th >= 2 * halo or cw == 1:
            break
        cw //= 2
    return dict(W=w, H=h, wp=wp, L=L, Lv=Lv, P=P, nr=nr_, CW=cw, TH=min(th, h))


def ones_below(n):
    n = np.asarray(n, np.int64)
    r = np.where(n >= 64, ONES, (np.uint64(1) << np.clip(n, 0, 63).astype(np.uint64)) - np.uint64(1))
    return np.where(n <= 0, np.uint64(0), r).astype(np.uint64)


def pack(bw):
    """bool H x W -> uint64 H x wp, bit b of word k = pixel 64 k + b, pad bits 0 (what k_ln_mask writes)"""
    h, w = bw.shape
    wp = (w + 63) // 64
    a = np.zeros((h, wp * 64), np.uint8)
    a[:, :w] = bw
    return np.packbits(a, axis=1, bitorder="little").view("<u8").reshape(h, wp).astype(np.uint64)


def unpack(words, w):
    h = words.shape[0]
    b = np.unpackbits(np.ascontiguousarray(words.astype("<u8")).view(np.uint8).reshape(h, -1), axis=1, bitorder="little")
    return b[:, :w].astype(bool)


def _funnel(lo, hi, sh):
    return lo if sh == 0 else (lo >> np.uint64(sh)) | (hi << np.uint64(64 - sh))


def _read_cols(cur, sft, pad):
    """per word of each row: the 64 bits starting sft bits further right; words past the row's end are `pad`"""
    rows, P = cur.shape
    q, sh = sft >> 6, sft & 63
    ext = np.concatenate([cur, np.full((rows, q + 2), pad, np.uint64)], axis=1)
    return _funnel(ext[:, q:q + P], ext[:, q + 1:q + 1 + P], sh)


def _steps(k):
    """the shifts of the doubling: span 1 -> 2 -> 4 ... then the overlapping last step to k"""
    out, s = [], 1
    while True:
        if 2 * s <= k:
            out.append(s)
            s *= 2
        elif k > s:
            out.append(k - s)
            break
        else:
            break
    return out


def emulate_hopen(words, g):
    """k_ln_hopen over all rows (its row groups are independent of each other)"""
    W, wp, L, P = g["W"], g["wp"], g["L"], g["P"]
    H = words.shape[0]
    a = L // 2
    tail = ones_below(W - 64 * (wp - 1))
    src = words.copy()
    src[:, wp - 1] |= ~tail
    cur = np.empty((H, P), np.uint64)
    for c in range(P):
        s = 64 * c - 2 * a
        q, sh = s >> 6, s & 63   # floor / remainder, as the arithmetic shift does for negative s
        lo = src[:, q] if 0 <= q < wp else np.full(H, ONES, np.uint64)
        hi = src[:, q + 1] if 0 <= q + 1 < wp else np.full(H, ONES, np.uint64)
        cur[:, c] = _funnel(lo, hi, sh)
    for phase in (0, 1):
        pad = np.uint64(0) if phase else ONES
        for sft in _steps(L):
            v = _read_cols(cur, sft, pad)
            cur = (cur | v) if phase else (cur & v)
        if phase == 0:
            c = np.arange(P)
            cur = cur & (ones_below(a + W - 64 * c) & ~ones_below(a - 64 * c))[None, :]
    out = cur[:, :wp].copy()
    out[:, wp - 1] &= tail
    return out


def emulate_vopen(words, hwords, g):
    """k_ln_vopen tile by tile: out = bw & ~h & ~open_v"""
    H, wp, Lv, CW, TH = g["H"], g["wp"], g["Lv"], g["CW"], g["TH"]
    a = Lv // 2
    TR = TH + 2 * (Lv - 1)
    out = np.zeros_like(words)
    for y0 in range(0, H, TH):
        for x0 in range(0, wp, CW):
            cur = np.full((TR, CW), ONES, np.uint64)
            for r in range(TR):
                yy = y0 - 2 * a + r
                if 0 <= yy < H:
                    cols = min(CW, wp - x0)
                    cur[r, :cols] = words[yy, x0:x0 + cols]
            for phase in (0, 1):
                pad = np.uint64(0) if phase else ONES
                for sft in _steps(Lv):
                    v = np.concatenate([cur[sft:], np.full((min(sft, TR), CW), pad, np.uint64)], axis=0)[:TR]
                    cur = (cur | v) if phase else (cur & v)
                if phase == 0:
                    yy = y0 - a + np.arange(TR)
                    cur[(yy < 0) | (yy >= H)] = np.uint64(0)
            rows, cols = min(TH, H - y0), min(CW, wp - x0)
            sl = (slice(y0, y0 + rows), slice(x0, x0 + cols))
            out[sl] = words[sl] & ~hwords[sl] & ~cur[:rows, :cols]
    return out


def emulate_words(bw):
    """the device's bit path from the bw mask on: pack, horizontal opening, vertical opening + composition, expand"""
    h, w = bw.shape
    g = geometry(w, h)
    words = pack(bw)
    res = emulate_vopen(words, emulate_hopen(words, g), g)
    return np.where(unpack(res, w), 0, 255).astype(np.uint8)
