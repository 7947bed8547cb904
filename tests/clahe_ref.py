"""cv::CLAHE::apply on 8-bit pages, cv::equalizeHist and EnhanceLocalContrastByCLAHE (src/imageLibCommon.cpp:327-395) restated in
numpy as include/prl_hip.h ("contrast") states them: integer histograms and the integer clip-and-redistribute in int64, every
float operation on float32 arrays, one numpy call per operation, in the written order (numpy never fuses).  The yardstick of
tests/test_clahe_cpu.py and tests/test_clahe_gpu.py; also the page generators they share and the geometry constants of the kernels
(clahe.hip, clahe.h)."""
import numpy as np

# k_clahe_hist: a tile taller than HIST_BAND_ROWS rows is split into bands, a workgroup each; a workgroup takes tiles (bands) until
# it has about HIST_UNIT_PX pixels.  k_clahe_interp: a workgroup's block is BLOCK_W x BLOCK_H pixels, 4 pixels a lane; it stages up to
# STAGE_TABLES tile tables per channel in LDS and reads them from global memory when its block touches more.
HIST_BAND_ROWS, HIST_UNIT_PX, BLOCK_W, BLOCK_H, STAGE_TABLES, LANE_PX = 64, 4096, 128, 64, 16, 4
MAX_TILES, MAX_SIDE = 64, 32768

F = np.float32


def reflect101(i, n):
    """cv::borderInterpolate(i, n, BORDER_REFLECT_101) for an array of any indices: a side of 1 gives 0, else reflect until inside"""
    i = np.array(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    while True:
        out = (i < 0) | (i >= n)
        if not out.any():
            return i
        i = np.where(i < 0, -i, np.where(i >= n, 2 * n - 2 - i, i))


def geometry(width, height, tiles=(8, 8), clip_limit=40.0):
    """(tile_w, tile_h, ext_w, ext_h, clip): both sides grow unless both divide"""
    tx, ty = tiles
    if width % tx == 0 and height % ty == 0:
        ew, eh = width, height
    else:
        ew, eh = width + (tx - width % tx), height + (ty - height % ty)
    tw, th = ew // tx, eh // ty
    clip = 0
    if clip_limit > 0:
        with np.errstate(over="ignore"):
            q = np.float64(clip_limit) * np.float64(tw * th) / np.float64(256)
        c = int(q) if -2.0 ** 31 <= q < 2.0 ** 31 else -2 ** 31   # (int) of a double as x86 converts it
        clip = max(c, 1)
    return tw, th, ew, eh, clip


def extended(plane, tiles):
    """the page the tiles are cut from"""
    h, w = plane.shape
    _, _, ew, eh, _ = geometry(w, h, tiles, 0.0)
    if (ew, eh) == (w, h):
        return plane
    return plane[np.ix_(reflect101(np.arange(eh), h), reflect101(np.arange(ew), w))]


def sat_u8(t):
    """saturate_cast<uchar> of finite float32 values: half to even, then clamp"""
    t = np.asarray(t)
    assert t.dtype == np.float32
    return np.clip(np.rint(t), 0, 255).astype(np.uint8)


def redistribute(hist, clip):
    """the clip and the 3.4 / 4.x redistribution of int64 bins [..., 256] (clip > 0); returns new bins"""
    h = np.array(hist, np.int64).reshape(-1, 256)
    clipped = np.maximum(h - clip, 0).sum(axis=1)
    h = np.minimum(h, clip)
    batch = clipped // 256
    residual = clipped - 256 * batch
    h += batch[:, None]
    for t in np.nonzero(residual)[0]:
        step = max(256 // int(residual[t]), 1)
        h[t, np.arange(0, 256, step)[:int(residual[t])]] += 1     # i = 0, step, 2 step, ... while i < 256 and residual > 0
    return h.reshape(np.shape(hist))


def redistribute_v24(hist, clip):
    """OpenCV 2.4's rule, for the test that tells the two apart: the first `residual` bins get the extra"""
    h = np.array(hist, np.int64)
    clipped = int(np.maximum(h - clip, 0).sum())
    h = np.minimum(h, clip) + clipped // 256
    h[:clipped % 256] += 1
    return h


def redistribute_loop(hist, clip):
    """the same as `redistribute` for one tile, loop for loop as clahe.cpp writes it"""
    h = [int(v) for v in hist]
    clipped = 0
    for i in range(256):
        if h[i] > clip:
            clipped += h[i] - clip
            h[i] = clip
    batch = clipped // 256
    residual = clipped - batch * 256
    for i in range(256):
        h[i] += batch
    if residual != 0:
        step = max(256 // residual, 1)
        i = 0
        while i < 256 and residual > 0:
            h[i] += 1
            i += step
            residual -= 1
    return np.array(h, np.int64)


def tile_lut(hist, clip, area):
    """bins [..., 256] -> tables [..., 256] uint8"""
    h = np.array(hist, np.int64)
    if clip > 0:
        h = redistribute(h, clip)
    scale = F(255) / F(area)
    return sat_u8(np.cumsum(h, axis=-1).astype(F) * scale)


def tile_hists(plane, tiles):
    """H x W uint8 -> int64 [tilesY, tilesX, 256] over the extended page"""
    tx, ty = tiles
    ext = extended(plane, tiles)
    th, tw = ext.shape[0] // ty, ext.shape[1] // tx
    t = ext.reshape(ty, th, tx, tw).transpose(0, 2, 1, 3).reshape(ty * tx, th * tw).astype(np.int64)
    t = t + 256 * np.arange(ty * tx)[:, None]
    return np.bincount(t.ravel(), minlength=256 * ty * tx).reshape(ty, tx, 256)


def plane_luts(plane, clip_limit=40.0, tiles=(8, 8)):
    """H x W -> uint8 [tilesY, tilesX, 256]"""
    h, w = plane.shape
    tw, th, _, _, clip = geometry(w, h, tiles, clip_limit)
    return tile_lut(tile_hists(plane, tiles), clip, tw * th)


def axis(n, tile, tiles):
    """per coordinate 0..n-1: (t1, t2, a, a1), the weights float32"""
    inv = F(1.0) / F(tile)
    txf = np.arange(n).astype(F) * inv - F(0.5)
    f = np.floor(txf)
    a = txf - f
    a1 = F(1.0) - a
    f = f.astype(np.int64)
    assert a.dtype == F and a1.dtype == F
    return np.maximum(f, 0), np.minimum(f + 1, tiles - 1), a, a1


def _corners(plane, L, tiles):
    h, w = plane.shape
    tx, ty = tiles
    tw, th, _, _, _ = geometry(w, h, tiles, 0.0)
    tx1, tx2, xa, xa1 = axis(w, tw, tx)
    ty1, ty2, ya, ya1 = axis(h, th, ty)
    v = plane.astype(np.int64)
    pick = lambda yy, xx: L[yy[:, None], xx[None, :], v]  # noqa: E731
    return (pick(ty1, tx1), pick(ty1, tx2), pick(ty2, tx1), pick(ty2, tx2)), (xa[None, :], xa1[None, :], ya[:, None], ya1[:, None])


def plane_clahe(plane, clip_limit=40.0, tiles=(8, 8), luts=None):
    L = plane_luts(plane, clip_limit, tiles) if luts is None else luts
    (l11, l12, l21, l22), (xa, xa1, ya, ya1) = _corners(plane, L, tiles)
    l11, l12, l21, l22 = (x.astype(F) for x in (l11, l12, l21, l22))
    top = l11 * xa1 + l12 * xa
    bottom = l21 * xa1 + l22 * xa
    res = top * ya1 + bottom * ya
    assert res.dtype == F
    return sat_u8(res)


def plane_blend64(plane, clip_limit=40.0, tiles=(8, 8)):
    """the blend's value in float64, from the same tables and the float32 weights xa, ya taken as exact numbers"""
    L = plane_luts(plane, clip_limit, tiles)
    (l11, l12, l21, l22), (xa, _, ya, _) = _corners(plane, L, tiles)
    xa, ya = xa.astype(np.float64), ya.astype(np.float64)
    l11, l12, l21, l22 = (x.astype(np.float64) for x in (l11, l12, l21, l22))
    return (l11 * (1.0 - xa) + l12 * xa) * (1.0 - ya) + (l21 * (1.0 - xa) + l22 * xa) * ya


def _per_channel(page, f):
    page = np.asarray(page)
    assert page.dtype == np.uint8
    if page.ndim == 2:
        return f(page)
    return np.stack([f(np.ascontiguousarray(page[:, :, c])) for c in range(page.shape[2])], axis=-1)


def clahe(page, clip_limit=40.0, tiles=(8, 8)):
    """H x W [x C] -> the same shape"""
    return _per_channel(page, lambda p: plane_clahe(p, clip_limit, tiles))


def luts(page, clip_limit=40.0, tiles=(8, 8)):
    """H x W -> [1, tilesY, tilesX, 256]; H x W x C -> [C, tilesY, tilesX, 256]"""
    page = np.asarray(page)
    planes = [page] if page.ndim == 2 else [np.ascontiguousarray(page[:, :, c]) for c in range(page.shape[2])]
    return np.stack([plane_luts(p, clip_limit, tiles) for p in planes])


def equalize_lut(hist):
    hist = np.asarray(hist, np.int64)
    total = int(hist.sum())
    i = int(np.nonzero(hist)[0][0])
    if hist[i] == total:
        return np.arange(256, dtype=np.uint8)
    scale = F(255.0) / F(total - int(hist[i]))
    h = hist.copy()
    h[:i + 1] = 0
    lut = sat_u8(np.cumsum(h).astype(F) * scale)
    lut[:i + 1] = 0
    return lut


def histogram(page):
    """H x W -> int64 [256]; H x W x C -> [C, 256]"""
    page = np.asarray(page)
    if page.ndim == 2:
        return np.bincount(page.ravel(), minlength=256)
    return np.stack([np.bincount(page[:, :, c].ravel(), minlength=256) for c in range(page.shape[2])])


def equalize(page):
    return _per_channel(page, lambda p: equalize_lut(histogram(p))[p])


def enhance(page, clip_limit, equalize_flag=False):
    out = clahe(page, clip_limit, (8, 8))
    return equalize(out) if equalize_flag else out


# ---- pages ------------------------------------------------------------------------------------------------------------------------

def _shape(h, w, c):
    return (h, w) if c == 1 else (h, w, c)


def noise(h, w, c=1, seed=0):
    rng = np.random.default_rng(1000 * seed + 7 * h + w + c)
    return rng.integers(0, 256, size=_shape(h, w, c), dtype=np.uint8)


def flat(h, w, v, c=1):
    return np.full(_shape(h, w, c), v, np.uint8)


def two_valued(h, w, lo=40, hi=200, c=1, seed=0):
    """mostly `hi` (paper) with about a tenth `lo` (ink)"""
    rng = np.random.default_rng(77 * seed + 3 * h + w + c)
    return np.where(rng.random(_shape(h, w, c)) < 0.1, lo, hi).astype(np.uint8)


def gradient(h, w, c=1):
    """a diagonal ramp over the whole byte range, the channels shifted against each other"""
    yy, xx = np.mgrid[0:h, 0:w]
    g = ((yy * 3 + xx * 5) * 255 // max(3 * (h - 1) + 5 * (w - 1), 1)).astype(np.uint8)
    return g if c == 1 else np.stack([np.roll(g, 2 * k, axis=1) for k in range(c)], axis=-1)


def paper(h, w, c=1, seed=0):
    """a flat page with a few noisy rectangles: the flat-wavefront shortcut and its neighbours in one page"""
    rng = np.random.default_rng(5 * seed + h + w + c)
    p = np.full(_shape(h, w, c), 230, np.uint8)
    for _ in range(6):
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        hh, ww = int(rng.integers(1, max(h // 3, 2))), int(rng.integers(1, max(w // 3, 2)))
        p[y:y + hh, x:x + ww] = rng.integers(0, 256, size=p[y:y + hh, x:x + ww].shape, dtype=np.uint8)
    return p


# ---- the vectors of tests/cpp/test_clahe.cpp ------------------------------------------------------------------------------------------

GOLDEN_PAGES = [  # (h, w, c, tiles, clip_limit, clahe, equalize, generator)
    (13, 16, 1, (8, 8), 40.0, 1, 0, "noise"), (16, 16, 1, (8, 8), 2.0, 1, 0, "gradient"), (1, 1, 1, (8, 8), 0.5, 1, 1, "noise"),
    (3, 17, 3, (8, 8), 3.0, 1, 1, "noise"), (9, 7, 4, (3, 5), 0.0, 1, 0, "paper"), (12, 10, 2, (1, 1), 40.0, 1, 1, "two"),
    (11, 14, 1, (64, 64), 1e6, 1, 0, "noise"), (10, 9, 3, (8, 8), 0.0, 0, 1, "two"), (20, 33, 1, (8, 8), 2.0, 1, 1, "paper"),
]
GOLDEN_TILES = [(1, 64), (2, 300), (3, 1000), (17, 4097), (0, 500)]   # (clip, area)


def _golden_page(h, w, c, gen, seed):
    return {"noise": lambda: noise(h, w, c, seed), "gradient": lambda: gradient(h, w, c), "paper": lambda: paper(h, w, c, seed),
            "two": lambda: two_valued(h, w, c=c, seed=seed)}[gen]()


def golden_bytes():
    """The vectors as one byte string.  Records, little-endian: int32 kind; kind 1 (a page): int32 h, w, c, tiles_x, tiles_y, clahe,
    equalize, float64 clip_limit, h * w * c bytes in, h * w * c bytes out; kind 2 (a tile): int32 clip, area, 256 uint32 bins, 256
    bytes; kind 0 ends the file."""
    import struct

    out = []
    for k, (h, w, c, tiles, clip, with_clahe, eq, gen) in enumerate(GOLDEN_PAGES):
        page = _golden_page(h, w, c, gen, k)
        res = clahe(page, clip, tiles) if with_clahe else page
        res = equalize(res) if eq else res
        out.append(struct.pack("<8id", 1, h, w, c, tiles[0], tiles[1], with_clahe, eq, clip) + page.tobytes() + res.tobytes())
    for k, (clip, area) in enumerate(GOLDEN_TILES):
        rng = np.random.default_rng(900 + k)
        bins = np.bincount(np.clip(rng.normal(128, 9 + 20 * k, area), 0, 255).astype(np.int64), minlength=256).astype(np.uint32)
        out.append(struct.pack("<3i", 2, clip, area) + bins.tobytes() + tile_lut(bins, clip, area).tobytes())
    out.append(struct.pack("<i", 0))
    return b"".join(out)


if __name__ == "__main__":
    import sys

    open(sys.argv[1], "wb").write(golden_bytes())
