"""Rule R (include/prl_hip.h, next to prl_hip_external_rects) and the component labels restated with scipy's flood fills, on whole
batches of equally sized maps at once: the maps are laid out as the cells of a mosaic, one pixel of background between and around
them, so that "the page is thought of as surrounded by background" is literal - a background component is outer iff it is the
mosaic's frame component.  Nothing here shares code or a method with components.h (union-find) or contour.h (border following).

    external_rects_batch(maps)   [(rects [(x, y, w, h), ...], found), ...]  for maps N x H x W
    external_rects(m)            the same for one map
    components(m, connectivity)  (labels int32 H x W: 0 / 1 .. K by first pixel, stats K x 5: left, top, width, height, area)
and the map families of the tests."""
import numpy as np
from scipy import ndimage

EIGHT = np.ones((3, 3), int)


def kept(bw, bh, area):
    """everything but a straight one-pixel line (a contour of fewer than 3 points), a single pixel included"""
    return not (area == max(bw, bh) and (min(bw, bh) == 1 or bw == bh))


def components(m, connectivity=8):
    fg = np.asarray(m) != 0
    lab, k = ndimage.label(fg, structure=EIGHT if connectivity == 8 else None)
    if k == 0:
        return np.zeros(fg.shape, np.int32), np.zeros((0, 5), np.int32)
    flat = lab.ravel()
    ids, first = np.unique(flat, return_index=True)   # the first pixel of every label in raster order
    if ids[0] == 0:
        ids, first = ids[1:], first[1:]
    rank = np.empty(k + 1, np.int64)
    rank[0] = 0
    rank[ids[np.argsort(first)]] = np.arange(1, k + 1)
    out = rank[lab].astype(np.int32)
    stats = np.zeros((k, 5), np.int32)
    for i, sl in enumerate(ndimage.find_objects(out)):
        stats[i] = (sl[1].start, sl[0].start, sl[1].stop - sl[1].start, sl[0].stop - sl[0].start, 0)
    stats[:, 4] = np.bincount(out.ravel(), minlength=k + 1)[1:]
    return out, stats


def external_rects_batch(maps):
    maps = np.asarray(maps)
    n, h, w = maps.shape
    cols = int(np.ceil(np.sqrt(n)))
    rows = (n + cols - 1) // cols
    full = np.zeros((rows * cols, h + 1, w + 1), bool)
    full[:n, 1:, 1:] = maps != 0
    mosaic = np.zeros((rows * (h + 1) + 1, cols * (w + 1) + 1), bool)
    mosaic[:-1, :-1] = full.reshape(rows, cols, h + 1, w + 1).transpose(0, 2, 1, 3).reshape(rows * (h + 1), cols * (w + 1))
    fg, k = ndimage.label(mosaic, structure=EIGHT)
    out = [([], 0) for _ in range(n)]
    if k == 0:
        return out
    bg, _ = ndimage.label(~mosaic)           # 4-connected
    frame = bg[0, 0]
    mw = mosaic.shape[1]
    ids, first = np.unique(fg.ravel(), return_index=True)
    ids, first = ids[1:], first[1:]
    area = np.bincount(fg.ravel(), minlength=k + 1)
    boxes = ndimage.find_objects(fg)
    fy, fx = first // mw, first % mw
    cell = ((fy - 1) // (h + 1)) * cols + (fx - 1) // (w + 1)
    ly, lx = (fy - 1) % (h + 1), (fx - 1) % (w + 1)
    external = (lx == 0) | (bg.ravel()[first - 1] == frame)
    order = np.lexsort((ly * w + lx, cell))
    lists = [[] for _ in range(n)]
    found = [0] * n
    for j in order:
        if not external[j]:
            continue
        c = int(cell[j])
        found[c] += 1
        sl = boxes[ids[j] - 1]
        bw, bh = sl[1].stop - sl[1].start, sl[0].stop - sl[0].start
        if kept(bw, bh, int(area[ids[j]])):
            lists[c].append((int((sl[1].start - 1) % (w + 1)), int((sl[0].start - 1) % (h + 1)), bw, bh))
    return list(zip(lists, found))


def external_rects(m):
    return external_rects_batch(np.asarray(m)[None])[0]


# ---- the map families ------------------------------------------------------------------------------------------------------------

def all_maps(h, w):
    """every map of h x w (h w <= 16): N x h x w of 0 / 255"""
    n = 1 << (h * w)
    bits = (np.arange(n)[:, None] >> np.arange(h * w)[None, :]) & 1
    return (bits.reshape(n, h, w) * 255).astype(np.uint8)


def dilate(m, times):
    m = np.asarray(m) != 0
    for _ in range(times):
        m = ndimage.binary_dilation(m, structure=EIGHT)
    return (m * 255).astype(np.uint8)


def random_maps(seed, count, max_side=24):
    """`count` seeded maps of 1 .. max_side a side at densities 1 .. 60 %, grouped by shape: {(h, w): N x h x w}"""
    rng = np.random.default_rng(seed)
    groups = {}
    for _ in range(count):
        h, w = int(rng.integers(1, max_side + 1)), int(rng.integers(1, max_side + 1))
        density = rng.uniform(0.01, 0.6)
        groups.setdefault((h, w), []).append(((rng.random((h, w)) < density) * 255).astype(np.uint8))
    return {k: np.stack(v) for k, v in groups.items()}


def ring(size, wall, inner=None):
    """a square ring of `size` a side with walls `wall` thick; inner: a map put into the middle of its hole"""
    m = np.zeros((size, size), np.uint8)
    m[:, :] = 255
    m[wall:size - wall, wall:size - wall] = 0
    if inner is not None:
        ih, iw = inner.shape
        y0, x0 = (size - ih) // 2, (size - iw) // 2
        assert y0 > wall and x0 > wall, "the inner map must not touch the wall"
        m[y0:y0 + ih, x0:x0 + iw] = inner
    return m


def nested_rings(depth, wall, gap=2, core=None):
    """rings inside rings to `depth`, `gap` background pixels between them, and a blob (or `core`) in the innermost hole"""
    m = np.full((3, 3), 255, np.uint8) if core is None else core
    for _ in range(depth):
        m = ring(m.shape[0] + 2 * (wall + gap), wall, m)
    return m


def framed(m, pad=1):
    return np.pad(m, pad)
