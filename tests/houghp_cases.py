"""The HoughLinesP cases shared by tests/test_houghp_cpu.py (what the oracle's segments must satisfy) and tests/test_houghp_gpu.py
(every kernel and every group size against the oracle): pages of a few hundred pixels, each the smallest on which its regime can
still go wrong.  Seeded numpy and prlib_amd.synth only.

cases() -> list of (name, image, threshold, line_length, line_gap, min_segments).  min_segments is the number of segments the
oracle finds (cv::HoughLinesP's definition run on the CPU); the tests assert len(want) >= min_segments, so that a case that
silently degenerates fails loudly."""
import numpy as np

from prlib_amd import synth


def frame_page():
    """97 x 203: the four border rows and columns, both diagonals, 600 clutter points."""
    a = np.zeros((97, 203), np.uint8)
    a[0, :] = a[-1, :] = 255
    a[:, 0] = a[:, -1] = 255
    i = np.arange(97)
    a[i, 2 * i] = 255
    a[i, 202 - 2 * i] = 255
    rng = np.random.default_rng(5)
    a[rng.integers(0, 97, 600), rng.integers(0, 203, 600)] = 1       # any non-zero value is a point
    return a


def dense_bar_page():
    """64 x 160, a solid block: many points of one 64-lane vote land in one cell (the ranking in visiting order)."""
    a = np.zeros((64, 160), np.uint8)
    a[20:30, 10:150] = 255
    return a


def text_page():
    """300 x 420, a text page the way findAngle sees it."""
    from oracle import capi as oc

    _, binary = oc.otsu(synth.text_page_numpy(300, 420, 5, skew_deg=2.0))
    return 255 - binary


def long_page():
    """24 x 4400: walks of more than 2048 steps per direction (their erasure cannot be put off)."""
    a = np.zeros((24, 4400), np.uint8)
    a[11, 30:4380] = 255
    a[5, 100:2300:2] = 255
    rng = np.random.default_rng(5)
    a[rng.integers(0, 24, 3000), rng.integers(0, 4400, 3000)] = 1
    return a


def side_page(width=8000):
    """16 x 8000 (the longest side the int16 cells are sized for): row 8 fully set, row 3 every third pixel."""
    a = np.zeros((16, width), np.uint8)
    a[8, :] = 255
    a[3, ::3] = 255
    return a


def first_n_page(n):
    """40 x 50 with the first n pixels in raster order set: point counts around the block (64), fetch (256) and ring (1024) sizes."""
    a = np.zeros(40 * 50, np.uint8)
    a[:n] = 255
    return a.reshape(40, 50)


def narrow_page():
    """61 x 23 (fewer than 32 columns: a row of the bit mask is one partly filled dword): the border, a diagonal, two columns."""
    a = np.zeros((61, 23), np.uint8)
    a[:, 0] = a[:, 22] = a[:, 11] = 255
    a[0, :] = a[60, :] = 255
    i = np.arange(61)
    a[i, (i * 22) // 60] = 255
    rng = np.random.default_rng(7)
    a[rng.integers(0, 61, 120), rng.integers(0, 23, 120)] = 1
    return a


def one_row_page():
    """1 x 300 (one row high): three runs with gaps of 2, 5 and 9 pixels between and inside them."""
    a = np.zeros((1, 300), np.uint8)
    a[0, 3:90] = 255
    a[0, 92:180:2] = 255
    a[0, 185:240] = 255
    a[0, 249:300:3] = 255
    return a


def w65_page():
    """70 x 129 (width 1 mod 64: the last 64-pixel chunk of a row holds one pixel): the last column, the column before the chunk
    edge, a row, a diagonal into the last column, clutter."""
    a = np.zeros((70, 129), np.uint8)
    a[:, 128] = 255
    a[:, 63] = 255
    a[35, :] = 255
    i = np.arange(70)
    a[i, 128 - i] = 255
    rng = np.random.default_rng(9)
    a[rng.integers(0, 70, 300), rng.integers(0, 129, 300)] = 1
    return a


N_POINTS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
_N_SEGMENTS = (0, 3, 2, 1, 5, 5, 6, 27, 26, 27)

_cache = None


def cases():
    global _cache
    if _cache is None:
        frame, long_, side = frame_page(), long_page(), side_page()
        c = [
            ("frame", frame, 40, 30, 3, 6),
            ("frame_thr16", frame, 16, 10, 1, 8),          # the lowest threshold the group kernel takes
            ("frame_gap0", frame, 30, 20, 0, 4),
            ("dense_bar", dense_bar_page(), 60, 50, 2, 10),
            ("text", text_page(), 100, 52, 20, 62),
            ("long_good", long_, 100, 550, 20, 2),
            ("long_short", long_, 100, 4390, 20, 0),       # every line too short to count: erased, no un-votes, nothing stored
            ("side8000", side, 2000, 1000, 5, 2),          # one cell counts to 8000
            ("side8000_high", side, 15999, 1000, 5, 0),    # a threshold above any count
        ]
        c += [("n%d" % n, first_n_page(n), 20, 10, 1, k) for n, k in zip(N_POINTS, _N_SEGMENTS)]
        c += [
            ("narrow23", narrow_page(), 20, 15, 2, NARROW_SEGMENTS),
            ("one_row", one_row_page(), 16, 20, 4, ONE_ROW_SEGMENTS),
            ("w129", w65_page(), 30, 25, 2, W129_SEGMENTS),
        ]
        for _, img, *_ in c:
            img.setflags(write=False)
        _cache = c
    return _cache


# the oracle's counts for the three cases this file adds to the issue's list
NARROW_SEGMENTS = 5
ONE_ROW_SEGMENTS = 2
W129_SEGMENTS = 4


def case(name):
    for c in cases():
        if c[0] == name:
            return c
    raise KeyError(name)
