"""What the CPU oracle's HoughLinesP segments must satisfy (CPU only): the GPU kernels are compared with oracle.houghp byte for
byte (tests/test_houghp_gpu.py), so the thing they are compared with is itself held to what cv::HoughLinesP's definition implies,
on the whole shared case list (tests/houghp_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import houghp_cases as hc

CASES = hc.cases()
IDS = [c[0] for c in CASES]


@pytest.fixture(scope="module")
def segments(oracle):
    """The oracle's segments of every case, computed once."""
    return {name: oracle.houghp(img, thr, ll, gap) for name, img, thr, ll, gap, _ in CASES}


def _walk_table():
    """How HoughLinesProbabilistic walks a line of angle n: (xflag, dx0, dy0), the longer component one pixel a step, the other
    in 16.16 fixed point (float32 trig table, a = -sin, b = cos)."""
    theta = np.float32(np.pi / 180)
    tab = []
    for n in range(180):
        c, s = np.float32(np.cos(n * float(theta))), np.float32(np.sin(n * float(theta)))
        a, b = -s, c
        if abs(a) > abs(b):
            tab.append((1, 1 if a > 0 else -1, int(round(float(b * np.float32(65536.0)) / abs(float(a))))))
        else:
            tab.append((0, int(round(float(a * np.float32(65536.0)) / abs(float(b)))), 1 if b > 0 else -1))
    return tab


def _walk(xflag, x0, y0, dx, dy, steps):
    """Pixels (j, i) of steps 0..steps-1 of a walk from the 16.16 start (x0, y0)."""
    s = np.arange(steps, dtype=np.int64)
    x, y = x0 + s * dx, y0 + s * dy
    return (x, y >> 16) if xflag else (x >> 16, y)


def _replays(mask, seg, table, gap):
    """The walks that HoughLinesProbabilistic can have made to report `seg` = (x of end 0, y of end 0, x of end 1, y of end 1) on
    `mask`: a start pixel (j, i) that is a point and an angle whose walk reaches end 0 after k >= 0 steps forwards and end 1
    after m >= 0 steps backwards, with no more than `gap` steps in a row without a point in between.  Yields the (j, i) index
    arrays of the pixels from end 1 to end 0, each distinct walk once."""
    h, w = mask.shape
    ex0, ey0, ex1, ey1 = (int(v) for v in seg)
    seen = set()
    for xflag, dx0, dy0 in table:
        # u: the component that moves one pixel a step, v: the one in 16.16 fixed point
        eu0, ev0, eu1, ev1, du, dv = (ex0, ey0, ex1, ey1, dx0, dy0) if xflag else (ey0, ex0, ey1, ex1, dy0, dx0)
        span = (eu0 - eu1) * du
        if span < 0:
            continue
        k = np.arange(span + 1, dtype=np.int64)                # steps from the start pixel to end 0
        u = eu0 - k * du
        v = ev0 - ((32768 + k * dv) >> 16)                     # ev0 = ((v << 16) + 32768 + k dv) >> 16
        v16 = (v << 16) + 32768 - (span - k) * dv              # the walk's fixed-point component at end 1
        ok = ((v16 >> 16) == ev1) & (v >= 0) & (v < (h if xflag else w))
        if not ok.any():
            continue
        ok[ok] = mask[v[ok], u[ok]] if xflag else mask[u[ok], v[ok]]
        for start16 in np.unique(v16[ok]):
            key = (xflag, du, dv, int(start16))
            if key in seen:
                continue
            seen.add(key)
            jj, ii = _walk(xflag, eu1 if xflag else int(start16), int(start16) if xflag else eu1, dx0, dy0, span + 1)
            if _connected(mask, jj, ii, gap):
                yield jj, ii


def _connected(mask, jj, ii, gap):
    h, w = mask.shape
    if jj.min() < 0 or jj.max() >= w or ii.min() < 0 or ii.max() >= h:
        return False
    on = np.flatnonzero(mask[ii, jj] != 0)
    return len(on) > 0 and on[0] == 0 and on[-1] == len(jj) - 1 and (len(on) < 2 or np.diff(on).max() - 1 <= gap)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_segments_are_lines_of_the_page(case, segments):
    name, img, thr, ll, gap, want_n = case
    seg = segments[name]
    assert len(seg) == want_n                                  # the count found when the case was written
    h, w = img.shape
    table = _walk_table()
    mask = (img != 0).copy()
    for n, s in enumerate(seg):
        x0, y0, x1, y1 = (int(v) for v in s)
        assert 0 <= x0 < w and 0 <= x1 < w and 0 <= y0 < h and 0 <= y1 < h, (n, s)
        assert img[y0, x0] and img[y1, x1], (n, s)             # both ends are points of the input
        assert max(abs(x1 - x0), abs(y1 - y0)) >= ll, (n, s)
        # ... which no earlier segment erased: replay the erasures on a copy of the mask.  Of the walks that can have given this
        # segment on the mask as it is now (start pixel and angle are not part of the result) only the pixels that ALL of them
        # cross are erased: the mask never loses a point the transform still had (it keeps those of the lines too short to
        # count, too), so every check here is a necessary condition.
        assert mask[y0, x0] and mask[y1, x1], (n, s)
        common = None
        for jj, ii in _replays(mask, s, table, gap):
            px = ii * w + jj
            common = px if common is None else np.intersect1d(common, px)
        assert common is not None, (n, s)                      # the segment is a walk over points of the page with gaps <= line_gap
        assert y0 * w + x0 in common and y1 * w + x1 in common
        mask.reshape(-1)[common] = False


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_same_list_again_and_under_a_smaller_capacity(case, segments, oracle):
    name, img, thr, ll, gap, _ = case
    seg = segments[name]
    assert np.array_equal(oracle.houghp(img, thr, ll, gap), seg)
    h, w = img.shape
    for cap in {0, 1, max(0, len(seg) - 1)}:                   # a list smaller than the result changes what is stored, not the count
        lines = np.full((8 + cap, 4), -7, np.int32)
        n = oracle.lib().prl_oracle_houghp(img.ctypes.data_as(C.c_void_p), img.strides[0], w, h, thr, ll, gap,
                                           lines.ctypes.data_as(C.c_void_p), cap)
        assert n == len(seg)
        k = min(cap, len(seg))
        assert np.array_equal(lines[:k], seg[:k]) and (lines[k:] == -7).all()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_no_segment_longer_than_the_page(case, oracle):
    name, img, thr, ll, gap, _ = case
    assert len(oracle.houghp(img, thr, max(img.shape) + 1, gap)) == 0
