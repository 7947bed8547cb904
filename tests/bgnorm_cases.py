"""Pages for prl::backgroundNormalization's kernels (bgnorm.hip), built from a tile pattern so that each case has one named feature
at the smallest size that shows it.  tests/test_bgnorm_cpu.py checks on the CPU that every case does have its feature and that the
oracle equals the independent numpy model on it; tests/test_bgnorm_gpu.py runs the same cases on the device.

The operation (Leptonica's pixBackgroundNormSimple): tiles of 10 x 15 pixels; foreground = pixels below 60 on the gray / green
channel, dilated 7 x 7; a complete tile with at least 40 background pixels gets their average, any other tile 0; holes are filled
along columns, columns without data from their neighbours; the map is smoothed and inverted; out = min(255, p * inv >> 8).
"""
import numpy as np

SX, SY, THRESH, MINCOUNT = 10, 15, 60, 40
DARK = 20


def tile_values(ny, nx, rng):
    return rng.integers(90, 251, (ny, nx))


def page_from_tiles(vals, holes=(), extra_w=0, extra_h=0, channels=1, rng=None, inset=False):
    """A page of vals.shape tiles: tile (i, j) has the value vals[i, j] (90 .. 250) with noise of +-3; the tiles of `holes` are painted
    DARK, which makes them foreground - whole (their 7 x 7 dilation then takes 3 pixels off every neighbour, which keeps at least
    4 x 15 background pixels between two holes) or, with inset, all but a frame of 3 pixels, so that the dilation covers the tile and
    nothing else.  extra_w < 10 columns and extra_h < 15 rows of incomplete tiles replicate the edge.  With 3 or 4 channels the
    pattern (and the dark paint) is the green channel's; red and blue have tile values of their own, a fourth channel random bytes."""
    rng = rng or np.random.default_rng(0)
    vals = np.asarray(vals)
    ny, nx = vals.shape
    assert 0 <= extra_w < SX and 0 <= extra_h < SY and vals.min() >= 90 and vals.max() <= 250

    def plane(v):
        p = np.kron(v, np.ones((SY, SX), np.int64)) + rng.integers(-3, 4, (ny * SY, nx * SX))
        return p

    g = plane(vals)
    for i, j in holes:
        if inset:
            g[i * SY + 3:(i + 1) * SY - 3, j * SX + 3:(j + 1) * SX - 3] = DARK
        else:
            g[i * SY:(i + 1) * SY, j * SX:(j + 1) * SX] = DARK
    if channels == 1:
        planes = [g]
    else:
        planes = [plane(90 + (vals * 7 + 31) % 161), g, plane(90 + (vals * 3 + 77) % 161)]
        if channels == 4:
            planes.append(rng.integers(0, 256, g.shape))
    page = np.stack(planes, axis=-1).astype(np.uint8)
    page = np.pad(page, ((0, extra_h), (0, extra_w), (0, 0)), mode="edge")
    return np.ascontiguousarray(page[:, :, 0] if channels == 1 else page)


def paint(page, ys, xs, value=DARK, channel=None):
    """page[ys, xs] = value on the gray / green channel (or on `channel`)"""
    if page.ndim == 2:
        page[ys, xs] = value
    else:
        page[ys, xs, 1 if channel is None else channel] = value


def _case(name, stage, page, failed=False, **expect):
    return dict(name=name, stage=stage, page=page, failed=failed, **expect)


def _col(ny, j):
    return [(i, j) for i in range(ny)]


# ---- the map stage (k_bg_maps) -------------------------------------------------------------------------------------------------------

def map_cases():
    out = []
    rng = np.random.default_rng(1000)

    def add(name, ny, nx, holes, extra_w=0, extra_h=0, channels=1, failed=False, inset=False, **expect):
        vals = tile_values(ny, nx, rng)
        page = page_from_tiles(vals, holes, extra_w, extra_h, channels, rng, inset)
        expect.setdefault("zero_tiles", sorted(set(holes)))
        out.append(_case(name, "map", page, failed, extra=(extra_w > 0, extra_h > 0), **expect))

    add("missing_left", 6, 8, _col(6, 0) + _col(6, 1), missing=[0, 1])
    add("missing_between", 6, 9, _col(6, 3) + _col(6, 4) + _col(6, 7), missing=[3, 4, 7])
    add("missing_last_and_incomplete", 6, 8, _col(6, 7), extra_w=4, missing=[7])
    add("missing_left_between_last_colour", 5, 9, _col(5, 0) + _col(5, 4) + _col(5, 5) + _col(5, 8), extra_w=7, extra_h=3, channels=3,
        missing=[0, 4, 5, 8])
    add("holes_above_first_below_last", 7, 7, [(0, 2), (1, 2), (6, 2), (0, 5), (5, 5), (6, 5), (3, 3)], extra_h=9, missing=[])
    add("holes_above_below_colour4", 6, 6, [(0, 1), (5, 1), (0, 4), (1, 4), (2, 4), (4, 4), (5, 4)], extra_w=2, extra_h=1, channels=4, missing=[])
    add("one_good_column", 6, 8, [(i, j) for i in range(6) for j in range(8) if j != 3], missing=[0, 1, 2, 4, 5, 6, 7])
    add("one_good_column_last", 5, 6, [(i, j) for i in range(5) for j in range(6) if j != 5], extra_w=5, missing=[0, 1, 2, 3, 4])
    add("one_good_tile", 6, 8, [(i, j) for i in range(6) for j in range(8) if (i, j) != (2, 3)], inset=True, missing=[0, 1, 2, 4, 5, 6, 7])
    add("one_good_tile_colour", 5, 6, [(i, j) for i in range(5) for j in range(6) if (i, j) != (4, 0)], inset=True, channels=3, extra_w=3,
        extra_h=4, missing=[1, 2, 3, 4, 5])
    add("no_good_tile", 6, 8, [(i, j) for i in range(6) for j in range(8)], failed=True, missing=list(range(8)))
    add("no_good_tile_colour", 5, 6, [(i, j) for i in range(5) for j in range(6)], channels=3, failed=True, missing=list(range(6)))
    add("map_4_wide_5_high", 5, 4, [], failed=True, missing=[])
    add("map_5_wide_4_high", 4, 5, [], failed=True, missing=[])
    add("map_4_wide_5_high_colour4", 5, 4, [], channels=4, failed=True, missing=[])
    add("map_5x5", 5, 5, [(2, 2)], missing=[])
    add("map_4x4_and_incomplete", 4, 4, [(1, 1)], extra_w=1, extra_h=1, missing=[])      # 5 x 5 with the incomplete row and column
    for ew, eh in ((0, 0), (6, 0), (0, 11), (6, 11)):
        add(f"extra_{ew}_{eh}", 6, 7, [(0, 0), (5, 6), (2, 3), (3, 3)], extra_w=ew, extra_h=eh, missing=[])
        add(f"extra_{ew}_{eh}_colour", 5, 6, [(4, 5), (0, 2)], extra_w=ew, extra_h=eh, channels=3, missing=[])
    # the 256-thread stride over the columns: maps 257 and 513 columns wide on pages 75 rows high, columns without data on both
    # sides of every multiple of 256
    add("map_257_wide", 5, 257, _col(5, 0) + _col(5, 255) + _col(5, 256) + [(0, 254), (4, 254), (2, 100)], missing=[0, 255, 256])
    add("map_513_wide", 5, 513, _col(5, 256) + _col(5, 257) + _col(5, 511) + _col(5, 512) + [(0, 255), (1, 255), (4, 510), (3, 300)],
        missing=[256, 257, 511, 512])
    add("map_257_wide_incomplete", 5, 256, _col(5, 255) + [(2, 254)], extra_w=9, missing=[255])
    for v in (255, 254):
        out.append(_case(f"flat_{v}", "map", np.full((90, 80), v, np.uint8), missing=[], zero_tiles=[], clamp=True, extra=(False, False)))
    return out


# ---- the tile stage (k_bg_tiles) -----------------------------------------------------------------------------------------------------

TILE_WIDTHS = [250, 251, 253, 256, 257, 259, 260, 500, 503, 510, 753]    # a workgroup takes 250 columns and a halo of 3 on each side


def _seam_xs(w):
    return [x for x in list(range(246, 254)) + list(range(496, 504)) if x < w]


def tile_cases():
    out = []
    rng = np.random.default_rng(2000)
    chans = (1, 3, 4)
    for n, w in enumerate(TILE_WIDTHS):
        nx, ew = w // SX, w % SX
        # a mark per tile row, each alone in its row: the dilation of one cannot hide another's
        for kind in ("columns", "pixels"):
            c = chans[(n + (kind == "pixels")) % 3]
            page = page_from_tiles(tile_values(8, nx, rng), (), ew, 0, c, rng)
            for x in _seam_xs(w):
                k = (x - 246) % 250
                if kind == "columns":
                    paint(page, slice(SY * k + 4, SY * k + 11), x)
                else:
                    paint(page, SY * k + 7, x)
            out.append(_case(f"seam_{kind}_{w}", "tile", page, marks=True))
    # the vertical dilation across tile rows: marks at rows 12 .. 17 and 27 .. 32, 20 columns apart
    for n, w in enumerate((250, 257, 503)):
        page = page_from_tiles(tile_values(5, w // SX, rng), (), w % SX, 4, chans[n], rng)
        for k, y in enumerate(list(range(12, 18)) + list(range(27, 33))):
            paint(page, y, 5 + 20 * k)
        out.append(_case(f"rows_{w}", "tile", page, marks=True))
    # the page's corners and edges
    n = 0
    for xi in range(5):
        for yi in range(3):
            w = TILE_WIDTHS[n % len(TILE_WIDTHS)]
            page = page_from_tiles(tile_values(5, w // SX, rng), (), w % SX, 7 * (n % 2), chans[n % 3], rng)
            h = page.shape[0]
            x, y = [0, 1, 2, w - 3, w - 1][xi], [0, 2, h - 1][yi]
            paint(page, y, x)
            out.append(_case(f"edge_x{['0', '1', '2', 'w-3', 'w-1'][xi]}_y{['0', '2', 'h-1'][yi]}_{w}", "tile", page, marks=True))
            n += 1
    # mincount at its edge.  Tile row 2 (page rows 30 .. 44; the smoothing never reads row 0 or column 0 of a map, so a tile there
    # would show in the raw maps alone) with rows 35 .. 39 dark over the full width: foreground rows 32 .. 42, 4 rows x 10 = 40
    # background pixels in every tile.  One dark pixel at (47, 10 j + 12) takes pixel (44, 10 j + 9) from tile (2, j): 39.  Rows
    # 35 .. 38 dark leave 50; a dark pixel at (45, 10 j + 10) takes rows 42 .. 44 of the tile's last three columns: 41.  j = 24 is the
    # last tile of a workgroup: the extra pixel lies in the next one.
    for c in chans:
        for j, w in ((2, 60), (24, 300)):
            for count in (39, 40, 41):
                page = page_from_tiles(tile_values(5, w // SX, rng), (), 0, 0, c, rng)
                paint(page, slice(35, 39 if count == 41 else 40), slice(None))
                if count == 39:
                    paint(page, 47, SX * j + 12)
                if count == 41:
                    paint(page, 45, SX * j + 10)
                out.append(_case(f"mincount_{count}_tile{j}_c{c}", "tile", page, counts={(2, j): count}, marks=True))
    # dark in red / blue only is not foreground
    page = page_from_tiles(tile_values(5, 26, rng), (), 3, 2, 3, rng)
    paint(page, slice(20, 40), slice(100, 130), 5, channel=0)
    paint(page, slice(50, 70), slice(240, 255), 0, channel=2)
    out.append(_case("dark_red_and_blue_only", "tile", page, no_foreground=True, zero_tiles=[]))
    page = page_from_tiles(tile_values(5, 7, rng), (), 0, 0, 4, rng)
    paint(page, slice(None), slice(None), 10, channel=0)
    paint(page, slice(None), slice(None), 10, channel=3)
    out.append(_case("dark_red_and_alpha_only_c4", "tile", page, no_foreground=True, zero_tiles=[]))
    return out


# ---- the apply stage (k_bg_apply) ----------------------------------------------------------------------------------------------------

APPLY_GRAY_WIDTHS = [48, 49, 55, 57, 63, 64, 65]      # groups of 16 pixels and their tail
APPLY_COLOUR_WIDTHS = [41, 47, 48, 49, 55]            # groups of 8 pixels and their tail


def apply_cases():
    out = []
    rng = np.random.default_rng(3000)
    for c, widths in ((1, APPLY_GRAY_WIDTHS), (3, APPLY_COLOUR_WIDTHS), (4, APPLY_COLOUR_WIDTHS)):
        for w in widths:
            page = page_from_tiles(tile_values(5, w // SX, rng), [(1, 1)], w % SX, 2, c, rng)
            # bytes of every size through the multiplier, the saturating ones included
            h = page.shape[0]
            if c == 1:
                page[40:, :] = rng.integers(60, 256, (h - 40, w), dtype=np.uint8)
            else:
                page[40:, :, :] = rng.integers(60, 256, (h - 40, w, c), dtype=np.uint8)
            out.append(_case(f"apply_{w}_c{c}", "apply", page))
    return out


def all_cases():
    return map_cases() + tile_cases() + apply_cases()


# ---- views and the mixed batch -------------------------------------------------------------------------------------------------------

VIEW_H, VIEW_W = 77, 131


def view_pages(c, n=2):
    rng = np.random.default_rng(4000 + c)
    return [page_from_tiles(tile_values(VIEW_H // SY, VIEW_W // SX, rng), [(1, 2), (3, 12)], VIEW_W % SX, VIEW_H % SY, c, rng) for _ in range(n)]


def mixed_batch():
    """four 4-channel pages of one call: good, all green dark (fails: copied as its first three channels), good, all green dark"""
    rng = np.random.default_rng(5000)
    pages = [page_from_tiles(tile_values(5, 6, rng), [(0, 0)] if i == 0 else [], 4, 3, 4, rng) for i in range(4)]
    for i in (1, 3):
        pages[i][:, :, 1] = rng.integers(0, THRESH, pages[i].shape[:2], dtype=np.uint8)
    return pages, [False, True, False, True]


def small_batch():
    """three 4-channel pages too small for a map (5 x 4 tiles): all copied"""
    rng = np.random.default_rng(6000)
    return [page_from_tiles(tile_values(4, 5, rng), (), 0, 0, 4, rng) for _ in range(3)]


# ---- what the oracle says about a page, stage by stage (oracle: the oracle.capi module) ---------------------------------------------

def tile_counts(oracle, page):
    """(background pixels per complete tile, the foreground mask), from the oracle's foreground mask"""
    fg = oracle.bgnorm_fgmask(page)
    h, w = fg.shape
    ny, nx = h // SY, w // SX
    return (fg[:ny * SY, :nx * SX] == 0).reshape(ny, SY, nx, SX).sum(axis=(1, 3)), fg


def oracle_raw_maps(oracle, page):
    """och x mh x mw: sum // count of the pixels outside the oracle's foreground mask, 0 below mincount, in plain numpy over the
    complete tiles; the row and column of incomplete tiles are 0"""
    cnt, fg = tile_counts(oracle, page)
    ny, nx = cnt.shape
    h, w = fg.shape
    a = page[:, :, None] if page.ndim == 2 else page[:, :, :3]
    keep = fg[:ny * SY, :nx * SX] == 0
    out = np.zeros((a.shape[2], -(-h // SY), -(-w // SX)), np.int64)
    for ch in range(a.shape[2]):
        s = (a[:ny * SY, :nx * SX, ch].astype(np.int64) * keep).reshape(ny, SY, nx, SX).sum(axis=(1, 3))
        out[ch, :ny, :nx] = np.where(cnt >= MINCOUNT, s // np.maximum(cnt, 1), 0)
    return out


def oracle_inv_maps(oracle, page):
    """(failed, och x mh x mw inverse maps or None): the oracle's chain bgnorm_bgmap -> bgnorm_invmap (which smooths with
    bgnorm_blockconv first), channel after channel, stopping at the first that fails"""
    och = 1 if page.ndim == 2 else 3
    invs = []
    for ch in range(och):
        failed, m = oracle.bgnorm_bgmap(page, ch)
        if not failed:
            failed, inv = oracle.bgnorm_invmap(m)
        if failed:
            return True, None
        invs.append(inv)
    return False, np.stack(invs)


def oracle_failed(oracle, page):
    return oracle_inv_maps(oracle, page)[0]
