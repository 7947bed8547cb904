"""prl::binarizeMokji restated (src/binarizations/binarizeMokji.cpp:35-94) - test infrastructure, no product code.

    mokji_loops      (a) the reference's statements line for line in Python ints on a zeroed matrix: the two loops over the interior
                         and over the pairs, then `int threshold = 0.5 * nominator / denominator + 0.5` in double
    mokji            (b) the vectorised numpy model: a sliding-window maximum for the dilation, a bincount over dil * 256 + gray
    threshold_int    (c) the integer form (nom + den) / (2 den) the device uses
Write E for maxEdgeWidth and M for minEdgeMagnitude.  Where the reference is undefined (denominator == 0: a NaN converted to int
is INT_MIN on x86 and cv::threshold with a negative threshold sets every pixel; M > 256 reads outside the matrix) the restatement
gives t = -1 and a page of 255, the decision stated in include/prl_hip.h.  Gray is the project's 14-bit luma of B, G, R.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = [(257, 3), (64, 64), (203, 117), (1031, 517)]   # w x h
BIG = (1031, 517)
# (E, M) per size: the GPU tests' thresholds and masks, and the CPU tests' (a) == (b)
PARAMS = [(3, 20), (1, 1), (7, 40), (3, 255), (3, 256)]
PARAMS_BIG = [(127, 20)]          # the widest element, on 1031 x 517 only
PARAMS_FLAT = [(2, 20)]           # 257 x 3: rows <= 2E, no interior
BORDERS = [0, 1, 3]
MIN_DIFFS = [0, 1, 20, 255, 256]


def params_of(size):
    return PARAMS + (PARAMS_BIG if size == BIG else []) + (PARAMS_FLAT if size == (257, 3) else [])


# ---- the pieces -------------------------------------------------------------------------------------------------------------

def gray_of(img):
    """cv::cvtColor(BGR2GRAY) as the 14-bit fixed-point luma; a 2-D page is its own gray"""
    if img.ndim == 2:
        return img
    if img.shape[2] == 1:
        return img[:, :, 0]
    if img.shape[2] not in (3, 4):
        raise ValueError("1, 3 or 4 channels")
    b, g, r = (img[:, :, i].astype(np.int64) for i in range(3))
    return ((b * 1868 + g * 9617 + r * 4899 + (1 << 13)) >> 14).astype(np.uint8)


def dilate_shifts(gray, e):
    """cv::dilate with RECT (2e + 1)^2, anchor at the centre, taps outside the page ignored: the maximum over every offset, one
    axis after the other (the form (a) uses)"""
    h, w = gray.shape
    rows = gray.copy()
    for d in range(1, min(e, w - 1) + 1):
        np.maximum(rows[:, d:], gray[:, :-d], out=rows[:, d:])
        np.maximum(rows[:, :-d], gray[:, d:], out=rows[:, :-d])
    out = rows.copy()
    for d in range(1, min(e, h - 1) + 1):
        np.maximum(out[d:], rows[:-d], out=out[d:])
        np.maximum(out[:-d], rows[d:], out=out[:-d])
    return out


def dilate_windows(gray, e):
    """the same as a sliding-window maximum over a page padded with zeros (the identity of max on bytes): the form (b) uses"""
    from numpy.lib.stride_tricks import sliding_window_view

    k = 2 * e + 1
    p = np.pad(gray, ((0, 0), (e, e)))
    rows = sliding_window_view(p, k, axis=1).max(axis=2)
    p = np.pad(rows, ((e, e), (0, 0)))
    return np.ascontiguousarray(sliding_window_view(p, k, axis=0).max(axis=2))


def _weights(m_min):
    n, m = np.mgrid[0:256, 0:256]
    mask = (n - m >= m_min).astype(np.int64)
    return mask, mask * (n + m)


_W = {}


def nom_den(matrix, m_min):
    """the two sums over the pairs n - m >= M of matrix[n][m], as Python ints"""
    m_min = min(int(m_min), 256)
    if m_min not in _W:
        _W[m_min] = _weights(m_min)
    mask, wsum = _W[m_min]
    mat = np.asarray(matrix, np.int64)
    return int((mat * wsum).sum()), int((mat * mask).sum())


def threshold_double_of(nom, den):
    """binarizeMokji.cpp:92 in double; denominator == 0: -1"""
    if den == 0:
        return -1
    return int(0.5 * float(nom) / float(den) + 0.5)


def threshold_int_of(nom, den):
    if den == 0:
        return -1
    return (nom + den) // (2 * den)


def threshold_double(matrix, m_min):
    return threshold_double_of(*nom_den(matrix, m_min))


def threshold_int(matrix, m_min):
    """(c)"""
    return threshold_int_of(*nom_den(matrix, m_min))


def apply_threshold(gray, t):
    return np.where(gray.astype(np.int64) > t, 255, 0).astype(np.uint8)


# ---- (a) the loops ------------------------------------------------------------------------------------------------------------

def matrix_loops(img, e):
    """the loop over the interior (binarizeMokji.cpp:55-71) on a zeroed matrix: a list of lists of Python ints"""
    gray = gray_of(img)
    h, w = gray.shape
    matrix = [[0] * 256 for _ in range(256)]
    if w > 2 * e and h > 2 * e:
        dilated = dilate_shifts(gray, e)
        for y in range(e, h - e):
            grow = gray[y].tolist()
            drow = dilated[y].tolist()
            for x in range(e, w - e):
                pixel = grow[x]
                darkest_neighbour = drow[x]
                assert darkest_neighbour >= pixel
                matrix[darkest_neighbour][pixel] += 1
    return matrix


def threshold_loops(matrix, m_min):
    """the loop over the pairs and the double sequence (:73-92)"""
    nominator = 0
    denominator = 0
    for m in range(0, 256 - min(m_min, 256)):
        for n in range(m + m_min, 256):
            val = matrix[n][m]
            nominator += (m + n) * val
            denominator += val
    if denominator == 0:
        return -1               # NaN -> INT_MIN on x86: every pixel is above it
    return int(0.5 * float(nominator) / float(denominator) + 0.5)


def mokji_loops(img, e=3, m_min=20, matrix=None):
    """-> (mask, t, matrix); `matrix`: matrix_loops(img, e) where the caller already has it"""
    if e < 1:
        raise ValueError("mokjiThreshold: invalid maxEdgeWidth")
    if m_min < 1:
        raise ValueError("mokjiThreshold: invalid minEdgeMagnitude")
    if matrix is None:
        matrix = matrix_loops(img, e)
    threshold = threshold_loops(matrix, m_min)
    return apply_threshold(gray_of(img), threshold), threshold, matrix


# ---- (b) the numpy model --------------------------------------------------------------------------------------------------------

def cooccurrence(a, b, border=0, min_diff=0):
    """out[b(y, x)][a(y, x)] over the interior, for the pairs with b - a >= min_diff; min_diff == 0 counts every pair, those with
    b < a included (int64 256 x 256)"""
    h, w = a.shape
    out = np.zeros((256, 256), np.int64)
    if w <= 2 * border or h <= 2 * border:
        return out
    ai = a[border:h - border, border:w - border].astype(np.int64).ravel()
    bi = b[border:h - border, border:w - border].astype(np.int64).ravel()
    keep = (bi - ai >= min_diff) if min_diff > 0 else np.ones(ai.shape, bool)
    out += np.bincount(bi[keep] * 256 + ai[keep], minlength=65536).reshape(256, 256)
    return out


def emulate_cooc(a, b, border=0, min_diff=0):
    """k_mokji_cooc's accounting lane by lane: a lane takes 4 pixels of an interior row, 64 consecutive lanes are a wavefront; a
    wavefront whose 256 pairs are one pair adds 256 once, a lane whose 4 pairs agree adds 4 once, every other pixel adds 1; a
    pair with b - a < min_diff (min_diff > 0) adds nothing"""
    h, w = a.shape
    out = np.zeros(65536, np.int64)
    iw, ih = w - 2 * border, h - 2 * border
    if iw <= 0 or ih <= 0:
        return out.reshape(256, 256)
    quads = (iw + 3) // 4
    lanes = (quads + 63) // 64 * 64
    ai = np.zeros((ih, lanes * 4), np.int64)
    bi = np.zeros((ih, lanes * 4), np.int64)
    ai[:, :iw] = a[border:h - border, border:w - border]
    bi[:, :iw] = b[border:h - border, border:w - border]
    key = (bi * 256 + ai).reshape(ih, lanes, 4)
    n = np.clip(iw - 4 * np.arange(lanes), 0, 4)[None, :].repeat(ih, axis=0)
    flat = (n == 4) & (key == key[:, :, :1]).all(axis=2)
    waves = key.reshape(ih, lanes // 64, 64, 4)
    wflat = flat.reshape(ih, lanes // 64, 64)
    uniform = wflat.all(axis=2) & (waves[:, :, :, 0] == waves[:, :, :1, 0]).all(axis=2)

    def add(keys, weight):
        keys = keys.ravel()
        if min_diff > 0:
            keys = keys[(keys // 256) - (keys % 256) >= min_diff]
        np.add.at(out, keys, weight)

    add(waves[:, :, 0, 0][uniform], 256)
    lane_uniform = np.repeat(uniform[:, :, None], 64, axis=2).reshape(ih, lanes)
    add(key[:, :, 0][flat & ~lane_uniform], 4)
    rest = ~flat & ~lane_uniform
    valid = np.arange(4)[None, None, :] < n[:, :, None]
    add(key[rest[:, :, None] & valid], 1)
    return out.reshape(256, 256)


def mokji_matrix(img, e=3):
    gray = gray_of(img)
    h, w = gray.shape
    if w <= 2 * e or h <= 2 * e:
        return np.zeros((256, 256), np.int64)
    return cooccurrence(gray, dilate_windows(gray, e), e, 0)


def mokji(img, e=3, m_min=20):
    """-> (mask, t)"""
    gray = gray_of(img)
    t = threshold_double(mokji_matrix(img, e), m_min)
    return apply_threshold(gray, t), t


# ---- page families --------------------------------------------------------------------------------------------------------------

def flat_page(w, h, v):
    return np.full((h, w), v, np.uint8)


def two_level_page(w, h, lo=50, hi=200):
    p = np.full((h, w), lo, np.uint8)
    p[:, w // 2:] = hi
    return p


def checker_page(w, h, a=17, b=200, cell=5):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where(((yy // cell) + (xx // cell)) % 2 == 0, a, b).astype(np.uint8)


def ramp_page(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((xx * 3 + yy * 7) % 256).astype(np.uint8)


def noise_page(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w), dtype=np.uint8)


def document_page(w, h, seed):
    from prlib_amd import synth

    return synth.page_numpy(h, w, index=seed)


def corners_page(w, h, seed):
    """black with lone white dots, a white block and a black block: bins (0, 0), (255, 255) and (255, 0)"""
    rng = np.random.default_rng(seed)
    p = np.zeros((h, w), np.uint8)
    p[:, 2 * w // 3:] = 255
    n = max(1, w * h // 400)
    p[rng.integers(0, h, n), rng.integers(0, max(1, w // 3), n)] = 255
    return p


def families(w, h, seed=1):
    return [("flat0", flat_page(w, h, 0)), ("flat255", flat_page(w, h, 255)), ("flat215", flat_page(w, h, 215)),
            ("two_level", two_level_page(w, h)), ("checker", checker_page(w, h)), ("ramp", ramp_page(w, h)),
            ("noise", noise_page(w, h, seed)), ("document", document_page(w, h, seed)), ("corners", corners_page(w, h, seed))]


def colour_page(w, h, seed, channels=3):
    rng = np.random.default_rng(seed + 100)
    g = document_page(w, h, seed).astype(np.int16)
    img = np.stack([g + rng.integers(-25, 26, size=g.shape) for _ in range(3)], axis=2)
    img = np.clip(img, 0, 255).astype(np.uint8)
    if channels == 4:
        img = np.concatenate([img, rng.integers(0, 256, size=(h, w, 1), dtype=np.uint8)], axis=2)
    return img
