"""The mask morphology of the binarizers (prlib_amd/csrc/morph.hip) from its definition, and the pages that aim at its kernels'
boundaries.  Test infrastructure: plain numpy on boolean arrays, no scipy, no oracle.

    close_open(mask_bool, n)   n > 0: dilate then erode with the (2n+1) x (2n+1) rectangle (closing); n < 0: erode then dilate
                               (opening).  A tap outside the page is ignored by both operators (cv::dilate / cv::erode with the
                               default border value).

Pages.  `m` is |n| everywhere.  Every builder returns the page in the polarity in which it says something about a CLOSING (set
pixels on a cleared page); pages_for() hands the complement to an opening, for which the same page then says the same thing about
the other operator pair.  All builders are deterministic.

    gap pairs   two set pixels in one row with g cleared pixels between them.  The dilations of the two touch iff g <= 2m, so a
                closing fills the gap for g = 2m (the two pixels 2m + 1 apart) and leaves it for g = 2m + 1: the filled pixel next
                to the left one needs the +m tap of the dilation and of the erosion, and a kernel that reaches one pixel too far or
                not far enough gets one of the two wrong.  Around a boundary column b the left pixel sits at b - 1 - j, j = 0..2m:
                the pair straddles b at every split.  One pair per boundary per band of m + 1 rows (pairs m + 1 rows apart keep
                their own row's answer); a page shorter than 2 (2m + 1) bands shows a part of the (j, g) combinations, chosen by
                `phase`, and n_phases() says how many pages show them all.
    bars        the same for runs: a block 2m + 1 rows high and 2m or 2m + 1 columns wide that starts at b - j.  An opening
                removes the first and keeps the second (built here as its complement: holes in a set page, which a closing fills or
                keeps).
    random      density 2.5 / (2m+1)^2: the closing of such a page is neither the page nor all white (test_morph_cpu.py asserts it).
    edges       set pixels within 2m + 1 of the four page edges only, plus the all-cleared and the all-set page.
"""
from __future__ import annotations

import numpy as np


def _rect(a: np.ndarray, m: int, is_or: bool) -> np.ndarray:
    """OR (or AND) over the (2m+1)^2 offsets; taps outside the page are ignored"""
    h, w = a.shape
    out = a.copy()
    for dy in range(-m, m + 1):
        y0, y1 = max(0, -dy), min(h, h - dy)
        if y0 >= y1:
            continue
        for dx in range(-m, m + 1):
            x0, x1 = max(0, -dx), min(w, w - dx)
            if x0 >= x1 or (dy == 0 and dx == 0):
                continue
            if is_or:
                out[y0:y1, x0:x1] |= a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
            else:
                out[y0:y1, x0:x1] &= a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def close_open(mask: np.ndarray, n: int) -> np.ndarray:
    assert mask.dtype == np.bool_ and mask.ndim == 2 and n != 0
    m = abs(n)
    return _rect(_rect(mask, m, n > 0), m, n < 0)


def to_bytes(mask: np.ndarray) -> np.ndarray:
    return np.where(mask, np.uint8(255), np.uint8(0))


def pack_rows(mask: np.ndarray) -> np.ndarray:
    """the bit plane of a page: pixel x of a row is bit x & 7 of byte x >> 3"""
    return np.packbits(mask, axis=1, bitorder="little")


def unpack_rows(bits: np.ndarray, width: int) -> np.ndarray:
    return np.unpackbits(bits, axis=1, count=width, bitorder="little").astype(bool)


# ---- pattern pages ---------------------------------------------------------------------------------------------------------------------
def _combos(m: int):
    """(j, g): the split and the gap (or run) length, both lengths next to each other"""
    return [(j, g) for j in range(2 * m + 1) for g in (2 * m, 2 * m + 1)]


def n_phases(extent: int, m: int, band: int) -> int:
    """pages of `extent` rows (bands of `band` rows) that together show every combination"""
    bands = max(1, (extent + band - 1) // band)
    return (len(_combos(m)) + bands - 1) // bands


def gap_pairs_h(h: int, w: int, m: int, xs, phase: int = 0) -> np.ndarray:
    """horizontal pairs around the boundary columns xs; band k (row k (m + 1)) shows combination k + phase * bands"""
    a = np.zeros((h, w), bool)
    c = _combos(m)
    s = m + 1
    bands = max(1, (h + s - 1) // s)
    for k in range(bands):
        for i, b in enumerate(xs):
            j, g = c[(k + phase * bands + 7 * i) % len(c)]
            left = b - 1 - j
            for x in (left, left + g + 1):
                if 0 <= x < w:
                    a[k * s, x] = True
    return a


def gap_pairs_v(h: int, w: int, m: int, ys, phase: int = 0) -> np.ndarray:
    """vertical pairs around the boundary rows ys (bands run along x)"""
    return np.ascontiguousarray(gap_pairs_h(w, h, m, ys, phase).T)


def gap_pairs_diag(h: int, w: int, m: int, x0: int, y0: int) -> np.ndarray:
    """two pixels on a diagonal, 2m and (further right) 2m + 1 apart both ways: their dilations share one pixel or touch at a
    corner, and neither pair fuses (no window fits into two squares that are offset diagonally)"""
    a = np.zeros((h, w), bool)
    for k, d in enumerate((2 * m, 2 * m + 1)):
        for y, x in ((y0, x0 + k * (4 * m + 6)), (y0 + d, x0 + k * (4 * m + 6) + d)):
            if 0 <= y < h and 0 <= x < w:
                a[y, x] = True
    return a


def bars_h(h: int, w: int, m: int, xs, phase: int = 0) -> np.ndarray:
    """holes 2m + 1 rows high and 2m / 2m + 1 columns wide in a set page, starting at b - j; bands of 2m + 2 rows"""
    a = np.ones((h, w), bool)
    c = _combos(m)
    s = 2 * m + 2
    bands = max(1, (h + s - 1) // s)
    for k in range(bands):
        for i, b in enumerate(xs):
            j, g = c[(k + phase * bands + 7 * i) % len(c)]
            x0, x1 = max(0, b - j), min(w, b - j + g)
            if x0 < x1:
                a[k * s:k * s + 2 * m + 1, x0:x1] = False
    return a


def bars_v(h: int, w: int, m: int, ys, phase: int = 0) -> np.ndarray:
    return np.ascontiguousarray(bars_h(w, h, m, ys, phase).T)


def random_mask(h: int, w: int, m: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).random((h, w)) < 2.5 / (2 * m + 1) ** 2


def edge_mask(h: int, w: int, m: int, seed: int) -> np.ndarray:
    """set pixels (one in four) in rows and columns 0..2m and in the last 2m + 1, none further inside"""
    a = np.random.default_rng(seed).random((h, w)) < 0.25
    t = 2 * m + 1
    a[t:max(t, h - t), t:max(t, w - t)] = False
    return a


def pages_for(n: int, h: int, w: int, xs, ys, seed: int = 1, max_phases: int = 6, phase0: int = 0):
    """[(name, page)] for radius n: every pattern above around the boundary columns xs and rows ys, in the polarity of n.  At most
    max_phases pages per pattern, the first of them showing the combinations of phase `phase0`."""
    m = abs(n)
    xs = sorted({int(b) for b in xs if 0 < b < w + 2 * m + 1})
    ys = sorted({int(b) for b in ys if 0 < b < h + 2 * m + 1})
    out = []
    if xs:
        for p in range(min(max_phases, n_phases(h, m, m + 1))):
            a = gap_pairs_h(h, w, m, xs, p + phase0)
            if p == 0:
                a |= gap_pairs_diag(h, w, m, xs[0] - m - 1, h // 2 + 1)
            out.append((f"gap_h{p}", a))
        for p in range(min(max_phases, n_phases(h, m, 2 * m + 2))):
            out.append((f"bar_h{p}", bars_h(h, w, m, xs, p + phase0)))
    if ys:
        for p in range(min(max_phases, n_phases(w, m, m + 1))):
            out.append((f"gap_v{p}", gap_pairs_v(h, w, m, ys, p + phase0)))
        for p in range(min(max_phases, n_phases(w, m, 2 * m + 2))):
            out.append((f"bar_v{p}", bars_v(h, w, m, ys, p + phase0)))
    out.append(("random", random_mask(h, w, m, seed)))
    out.append(("edges", edge_mask(h, w, m, seed + 1)))
    return [(name, a if n > 0 else ~a) for name, a in out]


def flat_pages(h: int, w: int):
    return [("all0", np.zeros((h, w), bool)), ("all255", np.ones((h, w), bool))]
