"""No GPU: the numpy thinning reference of tests/thin_ref.py against the C oracle, and the features the inputs of
tests/test_thin_gpu.py are chosen for - shown here, on the CPU, so that the GPU tests cannot lose them unnoticed."""
import numpy as np
import pytest

import thin_ref as R

METHODS = pytest.mark.parametrize("method", [0, 1], ids=["zhangsuen", "guohall"])


def _cpu_pages():
    from prlib_amd import synth

    rng = np.random.default_rng(5)
    yield "noise", rng.random((61, 83)) < 0.55
    blobs = np.zeros((90, 140), bool)
    for _ in range(9):
        y, x = int(rng.integers(0, 90)), int(rng.integers(0, 140))
        blobs[max(0, y - 9):y + 9, max(0, x - 14):x + 14] = True
    yield "blobs", blobs
    yield "text", synth.text_page_numpy(120, 260, 3) < 128
    win, pages = R.nb_batch(False, 7)
    yield "neighbourhoods", pages[13]
    yield "skeleton_already", R.bar_page(1)
    yield "empty", np.zeros((9, 40), bool)
    yield "full", np.ones((20, 45), bool)


@METHODS
def test_reference_equals_the_oracle_at_convergence(oracle, method):
    """Skeleton and pass count.  The reference's loop compares with a `prev` that starts as zeros (thinZhangSuen.cpp:88-96), so for a
    non-empty page that its first pass leaves unchanged it reports 2 passes where the first unchanged pass is pass 1: that one case
    is what oracle_pass_count() states; everywhere else the counts are equal."""
    seen = set()
    for name, im in _cpu_pages():
        img = im.astype(np.uint8) * 255
        want, want_passes = oracle.thin(img, method, return_passes=True)
        got, n = R.thin(img, method)
        assert np.array_equal(got, want), (name, int((got != want).sum()))
        first_changed = not np.array_equal(R.one_pass(im, method), im)
        assert R.oracle_pass_count(n, first_changed, not im.any()) == want_passes, (name, n, want_passes)
        seen.add(want_passes - n)
    assert seen == {0, 1}
    odd = np.random.default_rng(8).integers(0, 256, (40, 70), dtype=np.uint8)      # `&= 1`: only bit 0 counts
    assert np.array_equal(R.thin(odd, method)[0], oracle.thin(odd, method))


@METHODS
def test_windowed_reference_equals_the_whole_page(method):
    """Every pass of a window with cut edges equals the same rows and columns of the whole page's passes, for windows that touch
    none, some and all of the page's edges."""
    rng = np.random.default_rng(11)
    for win in (R.Window(50, 300, 7, 40, 100, 170), R.Window(50, 300, 0, 50, 230, 300), R.Window(50, 300, 0, 22, 0, 64),
                R.Window(50, 300, 30, 50, 0, 300), R.whole(24, 70)):
        content = rng.random((win.y1 - win.y0, win.x1 - win.x0)) < 0.6
        content[3:12, 5:40] = True
        page = win.paste(content)
        a, b = R.passes(content, method, win.edges), R.passes(page, method)
        assert len(a) == len(b) >= 3
        for x, y in zip(a, b):
            assert np.array_equal(x, win.cut(y)) and win.outside_is_zero(y)
    # and a cut is not a page edge: with the wrong flags the result differs
    win = R.Window(50, 300, 7, 40, 100, 170)
    content = np.ones((33, 70), bool)
    assert not np.array_equal(R.one_pass(content, method, win.edges), R.one_pass(content, method))


def test_neighbourhood_page_covers_every_pattern_everywhere():
    """All 512 patterns are on the block, each as the exact neighbourhood of its centre; over the 32 x-shifts and 16 y-shifts every
    pattern's centre meets every bit of a word and every row of a 16-row segment; at the seam placement, with the cell columns
    rotated by 6 * (y-shift % 6), every pattern's centre meets word 59 and word 60, on bit 31 of the one and bit 0 of the other
    (pixels 1919 and 1920, whose neighbour words come from the halo lanes)."""
    for rot in (0, 6, 30):
        block = np.pad(R.nb_block(rot), 1)
        seen = set()
        for pattern in range(512):
            y, x = nb = (1 + (pattern // 32) * 5 + 2, 1 + R.nb_cell_column(pattern, rot) * 5 + 2)
            got = sum(int(block[y - 1 + dy, x - 1 + dx]) << (3 * dy + dx) for dy in range(3) for dx in range(3))
            assert got == pattern, (pattern, nb)
            assert not block[y - 2, x - 2:x + 3].any() and not block[y + 2, x - 2:x + 3].any()          # nothing else within reach
            assert not block[y - 2:y + 3, x - 2].any() and not block[y - 2:y + 3, x + 2].any()
            seen.add(got)
        assert len(seen) == 512
    assert R.NB_ROWS * R.NB_COLS == 512 and R.NB_PITCH == 5
    patterns, shifts = np.arange(512)[:, None], np.arange(R.NB_XSHIFTS)[None, :]
    for seam in (False, True):
        bits, rows = np.zeros((512, 32), bool), np.zeros((512, 16), bool)      # [pattern, bit of the word / row of the segment] met
        at = {x: np.zeros(512, bool) for x in (1919, 1920)}                    # [pattern] centre met on this pixel
        for ys in range(R.NB_YSHIFTS):
            width, x_origin, rot = R.nb_placement(seam, ys)
            y, x = R.nb_centre(patterns, ys, shifts, x_origin, rot)            # [512, 1], [512, 32]
            assert (1 <= y).all() and (y < R.NB_PAGE_H - 1).all() and (1 <= x).all() and (x < width - 1).all()
            bits[np.broadcast_to(patterns, x.shape), x % 32] = True
            rows[patterns, y % 16] = True
            for px in at:
                at[px] |= (x == px).any(axis=1)
        assert bits.all() and rows.all(), (seam, np.nonzero(~bits.all(axis=1))[0], np.nonzero(~rows.all(axis=1))[0])
        if seam:
            assert at[1919].all() and at[1920].all() and 1919 // 32 == 59 and 1920 // 32 == 60, (at[1919].sum(), at[1920].sum())
    # the batch really holds the block where nb_centre says, and nothing outside its window
    for seam, ys in ((False, 0), (True, 15), (True, 4)):
        win, pages = R.nb_batch(seam, ys)
        width, x_origin, rot = R.nb_placement(seam, ys)
        assert pages.shape == (32, R.NB_PAGE_H, win.x1 - win.x0) and win.width == width and win.edges == (True, True, not seam, not seam)
        for xs in (0, 17, 31):
            page = win.paste(pages[xs])
            for pattern in (0, 1, 255, 311, 511):
                y, x = R.nb_centre(pattern, ys, xs, x_origin, rot)
                assert np.array_equal(page[y - 1:y + 2, x - 1:x + 2], R.pattern_bits(pattern))
            assert page.sum() == sum(bin(p).count("1") for p in range(512))
    assert R.NB_SEAM_X + R.NB_W + 31 < R.NB_SEAM_WIDTH and R.NB_SEAM_X < 1920 < R.NB_SEAM_X + R.NB_W


@METHODS
def test_bar_pass_counts(oracle, method):
    """A solid bar of thickness 1, 2, 6, 8, 22, 24, 54, 56, 118, 120 takes 1, 2, 4, 5, 12, 13, 28, 29, 60, 61 passes, the final
    unchanged one included: one page either side of each host check of the product's loop (after 4, 12, 28 and 60 passes), odd and
    even counts.  The oracle reports the same, but for the bar of thickness 1 (see oracle_pass_count)."""
    counts = [len(R.passes(R.bar_page(t), method)) for t in R.BAR_THICKNESS]
    assert tuple(counts) == R.BAR_PASSES == (1, 2, 4, 5, 12, 13, 28, 29, 60, 61)
    checks = (4, 12, 28, 60)
    assert all(c in counts and c + 1 in counts for c in checks)
    for t, n in zip(R.BAR_THICKNESS, R.BAR_PASSES):
        img = R.bar_page(t).astype(np.uint8) * 255
        assert img.shape == (124, 420) and img[2:2 + t, 3:417].all() and img.sum() == 255 * t * 414
        want, passes = oracle.thin(img, method, return_passes=True)
        assert passes == (2 if t == 1 else n)
        assert np.array_equal(R.thin(img, method)[0], want)


def test_zigzag_wakes_tiles_from_every_side():
    """Zhang-Suen, tiles of 4 rows x 1920 columns: each of the two strokes shows a tile that changes after an unchanged pass with the
    changed neighbours in its strip only (v), in its segment only (h), diagonal only (d), and a tile that idles with its whole
    neighbourhood and changes later (react)."""
    for x_start in (32, 33):
        win, im = R.zigzag(x_start)
        assert win.x0 == 1880 and win.x0 + 40 == R.STRIP_PX and win.height == 120 and im[2:118].any(axis=1).all()
        assert (im.sum(axis=1)[2:118] == 2).all() and not im[:2].any() and not im[118:].any()
        seq, maps = R.change_maps(im, 0, win, R.ZIGZAG_RPS)
        kinds, react = R.wake_ups(maps)
        assert maps[0].shape == (30, 2) and {"v", "h", "d"} <= kinds and react, (x_start, kinds, react)
        assert len(seq) >= 15


@METHODS
def test_seam_slab_wakes_the_other_strip(method):
    """Both methods: the tiles of strip 1 first change around the 20th pass, when only tiles of strip 0 had changed (x)."""
    win, im = R.seam_slab()
    assert (win.height, win.width) == (40, 1960) and win.paste(im)[:, 1900:].all() and not win.paste(im)[:, :1900].any()
    for rps in (16, 4):
        seq, maps = R.change_maps(im, method, win, rps)
        kinds, _ = R.wake_ups(maps)
        first = min(p for p in range(len(maps)) if maps[p][:, 1].any())
        assert kinds == {"x"} and 15 <= first <= 25, (kinds, first)
        assert all(maps[p][:, 0].any() for p in range(first))


@METHODS
def test_anchored_block_wakes_tiles_from_above(method):
    """Both methods, tiles of 4 rows: the front comes down one strip (v), and tiles below it idle until it arrives (react)."""
    win, im = R.anchored_block()
    assert win.edges == R.PAGE_EDGES and im[6:].all() and not im[:6].any()
    seq, maps = R.change_maps(im, method, win, R.BLOCK_RPS)
    kinds, react = R.wake_ups(maps)
    assert "v" in kinds and len(react) >= 3 and len(seq) > 30, (kinds, react)
    assert any(later - idle >= 4 for _, idle, later in react)


def test_change_map_and_wake_ups_on_hand_made_maps():
    """The classifier itself, on maps written by hand (3 segments x 3 strips)."""
    def m(*tiles):
        a = np.zeros((3, 3), np.uint8)
        for t in tiles:
            a[t] = 1
        return a

    assert R.wake_ups([m((0, 1)), m((1, 1)), m()])[0] == {"v"}
    assert R.wake_ups([m((1, 0)), m((1, 1)), m()])[0] == {"h", "x"}
    assert R.wake_ups([m((0, 0)), m((1, 1)), m()])[0] == {"d", "x"}
    assert R.wake_ups([m((0, 0), (1, 0)), m((1, 1)), m()])[0] == {"x"}
    assert R.wake_ups([m((0, 0), (0, 1)), m((1, 1)), m()])[0] == set()
    kinds, react = R.wake_ups([m((0, 0)), m((0, 1)), m((0, 2)), m((1, 2)), m()])
    assert ((1, 2), 0, 3) in react and ((2, 2), 0, 0) not in [(t, i, l) for t, i, l in react]
    with pytest.raises(AssertionError):
        R.wake_ups([m((0, 0)), m((2, 2)), m()])
    win = R.Window(20, 4000, 4, 12, 1900, 1960)
    a = np.zeros((8, 60), bool)
    b = a.copy()
    b[3, 19] = True            # page row 7, column 1919
    assert np.array_equal(R.change_map(a, b, win, 4), np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]], np.uint8))
    b[4, 20] = True            # page row 8, column 1920
    assert R.change_map(a, b, win, 4)[2, 1] == 1 and R.change_map(a, b, win, 4).sum() == 2


def test_border_shapes_use_every_size():
    shapes = R.border_shapes()
    assert {h for h, _ in shapes} == set(R.BORDER_HEIGHTS) and {w for _, w in shapes} == set(R.BORDER_WIDTHS)
    for h, w in shapes:
        for p in R.border_pages(h, w):
            assert p[0].all() and p[-1].all() and p[:, 0].all() and p[:, -1].all()


def test_geometry_page_crosses_the_seam(oracle):
    im = R.geometry_page()
    assert im.shape == (70, 2000) and im[:, 1919].any() and im[:, 1920].any() and (im[:, 1919] & im[:, 1920]).any()
    for method in (0, 1):
        img = im.astype(np.uint8) * 255
        got, n = R.thin(img, method)
        assert n >= 8 and np.array_equal(got, oracle.thin(img, method))
