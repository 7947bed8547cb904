"""cv::pyrDown, cv::Canny (classes, linking, composed), the edge map of prl::documentContour and prl::resize on the device, every
byte against tests/edges_ref.py.  The shapes are the smallest at which the kernels can go wrong: k_pyr_down makes 256 output
columns x 32 output rows per workgroup (512 x 64 source pixels), k_canny_classes 256 columns x 64 rows, k_edge_link works on
tiles of 64 rows x 256 columns in words of 64 columns."""
import os

import numpy as np
import pytest

import edges_ref as er

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCANS = [os.path.join(ROOT, "tests", "golden", "scans", n) for n in ("0004.npz", "0010.npz")]
PYR_W = (1, 2, 3, 4, 5, 63, 64, 65, 511, 512, 513, 1023, 1025)   # 512 source columns a workgroup, +- 1, twice that +- 1
PYR_H = (1, 2, 3, 4, 5, 63, 64, 65, 127, 129)                    # 64 source rows a run
CN_W = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 513)
CN_H = (1, 2, 3, 4, 5, 63, 64, 65, 127, 129)
THRESHOLDS = [(-1, -1), (0, 0), (25, 50), (50, 25), (2039, 2040), (2040, 2041)]
LINK_SIZES = [(3 * 64 + 1, 3 * 256 + 1), (3 * 64 - 1, 3 * 256 - 1)]


def rnd(shape, seed):
    return np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)


def blocks(h, w, seed, cell=3):
    r = np.random.RandomState(seed)
    small = r.randint(0, 2, ((h + cell - 1) // cell, (w + cell - 1) // cell)).astype(np.uint8) * 255
    return np.ascontiguousarray(np.kron(small, np.ones((cell, cell), np.uint8))[:h, :w])


def dev(a, cuda_device):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda_device)


def scan_page(i, h=None, w=None):
    """scan i of the fixtures, tiled or cut to h x w"""
    g = np.load(SCANS[i])["gray"]
    if h is None:
        return g
    reps = ((h + g.shape[0] - 1) // g.shape[0], (w + g.shape[1] - 1) // g.shape[1])
    return np.ascontiguousarray(np.tile(g, reps)[:h, :w])


# ---- cv::pyrDown ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("channels", [1, 2, 3, 4])
def test_pyr_down_every_edge_size(prl, cuda_device, channels):
    """three pages of distinct content per size: a seam error shows"""
    for w in PYR_W:
        for h in PYR_H:
            pages = rnd((3, h, w, channels), 11 * w + h + channels)
            got = prl.pyr_down(dev(pages, cuda_device)).cpu().numpy()
            for i in range(3):
                assert np.array_equal(got[i], er.pyr_down(pages[i])), (w, h, channels, i)


@pytest.mark.parametrize("shape", [(37, 1027), (131, 45), (3, 2051), (1, 9), (2, 2)])
def test_pyr_down_three_levels(prl, cuda_device, shape):
    """odd sizes at every level; the levels between live in the workspace"""
    for channels in (1, 3):
        pages = rnd((2,) + shape + (channels,), shape[0] + shape[1] + channels)
        got = prl.pyr_down(dev(pages, cuda_device), 3).cpu().numpy()
        assert prl.pyr_down_size(shape[1], shape[0], 3) == (got.shape[2], got.shape[1])
        for i in range(2):
            assert np.array_equal(got[i], er.pyr_down(pages[i], 3)), (shape, channels, i)
            assert np.array_equal(got[i], er.pyr_down(er.pyr_down(er.pyr_down(pages[i]))))


def test_pyr_down_strides_and_alignments(prl, cuda_device):
    """strided rows and pages on both sides, the destination at every alignment 0 .. 7; the bytes around the result stay"""
    import torch

    h, w = 70, 333
    oh, ow = 35, 167
    for channels in (1, 3):
        pages = rnd((2, h, w, channels), 5 + channels)
        big = torch.zeros((2, h + 3, w * channels + 13), dtype=torch.uint8, device=cuda_device)
        src = big[:, 1:1 + h, 5:5 + w * channels].unflatten(2, (w, channels))
        src.copy_(dev(pages, cuda_device))
        for a in range(8):
            raw = torch.full((2 * (oh + 2) * (ow * channels + 24) + 8,), 0xAB, dtype=torch.uint8, device=cuda_device)
            out = raw[a:a + 2 * (oh + 2) * (ow * channels + 24)].view(2, oh + 2, ow * channels + 24)[:, 1:1 + oh, 3:3 + ow * channels]
            out = out.unflatten(2, (ow, channels))
            prl.pyr_down(src, 1, out=out)
            got = out.cpu().numpy()
            for i in range(2):
                assert np.array_equal(got[i], er.pyr_down(pages[i])), (channels, a, i)
            mask = torch.ones_like(raw, dtype=torch.bool)
            mask[a:a + 2 * (oh + 2) * (ow * channels + 24)].view(2, oh + 2, ow * channels + 24)[:, 1:1 + oh, 3:3 + ow * channels] = False
            assert bool((raw[mask] == 0xAB).all())
    gray = rnd((2, h, w), 1)
    assert np.array_equal(prl.pyr_down(dev(gray, cuda_device)).cpu().numpy()[1], er.pyr_down(gray[1]))   # N x H x W


# ---- cv::Canny, stage 1 ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("thr", THRESHOLDS, ids=[f"{a}_{b}" for a, b in THRESHOLDS])
def test_canny_classes_every_edge_size(prl, cuda_device, thr):
    for w in CN_W:
        for h in CN_H:
            pages = np.stack([rnd((h, w), 3 * w + h), blocks(h, w, w + 7 * h), rnd((h, w), w * h) >> 4])
            got = prl.canny_classes(dev(pages, cuda_device), *thr).cpu().numpy()
            for i in range(3):
                assert np.array_equal(got[i], er.canny_classes(pages[i], *thr)), (w, h, thr, i)


def test_canny_classes_page_seam(prl, cuda_device):
    """page 0 ends bright and page 1 starts dark: read as one image, the seam would be the strongest edge of both"""
    h, w = 66, 300
    a = np.full((h, w), 40, np.uint8)
    a[h - 3:] = 250
    a[:, 100:103] = 90
    b = np.full((h, w), 10, np.uint8)
    b[:, 200:] = 200
    pages = np.stack([a, b, a[::-1]])
    got = prl.canny_classes(dev(pages, cuda_device), 25, 50).cpu().numpy()
    for i in range(3):
        assert np.array_equal(got[i], er.canny_classes(pages[i], 25, 50)), i
    # away from the page's own vertical strokes the rows at the seam are flat: nothing there
    assert (got[0][h - 1, :95] == 1).all() and (got[0][h - 1, 108:] == 1).all() and (got[1][0, :190] == 1).all()
    full = prl.canny(dev(pages, cuda_device), 25, 50).cpu().numpy()
    for i in range(3):
        assert np.array_equal(full[i], er.canny(pages[i], 25, 50)), i


# ---- cv::Canny, stage 2 ------------------------------------------------------------------------------------------------------------

def link_pages(h, w):
    """hand-made class maps, one per case, as a batch; 1 = nothing"""
    pages = {}
    s = np.ones((h, w), np.uint8)          # a serpentine of horizontal runs: every second row, joined at alternating ends
    s[0::2] = 0
    for k, y in enumerate(range(1, h - 1, 2)):
        s[y, w - 1 if k % 2 == 0 else 0] = 0
    last = (h - 1) // 2 * 2                  # driven from its far end alone
    s[last, (w - 1) if (last // 2) % 2 == 0 else 0] = 2
    pages["serpentine_rows"] = s
    t = np.ones((h, w), np.uint8)          # the same of vertical runs: crosses the tiles' upper and lower borders both ways
    t[:, 0::2] = 0
    for k, x in enumerate(range(1, w - 1, 2)):
        t[h - 1 if k % 2 == 0 else 0, x] = 0
    lastx = (w - 1) // 2 * 2
    t[(h - 1) if (lastx // 2) % 2 == 0 else 0, lastx] = 2
    pages["serpentine_columns"] = t
    c = np.ones((h, w), np.uint8)          # diagonals through the corners where four tiles meet, both ways
    for i in range(-6, 7):
        c[64 + i, 256 + i] = 0
        c[128 + i, 512 - i] = 0
    c[64 + 6, 256 + 6] = 2
    c[128 - 6, 512 + 6] = 2
    c[10, 63], c[11, 64] = 0, 2              # a diagonal step across a word border ...
    c[20, w - 2], c[21, w - 1] = 2, 0        # ... and into the last, partly filled word
    c[30, w - 1], c[31, 0] = 0, 2            # the end of a row and the start of the next are no neighbours
    c[h - 1, 300] = 0                        # (the next page starts with a class 2 right below)
    c[150:160, 100:140] = 0                  # a component that touches no class 2
    pages["corners_words_row_ends"] = c
    up = np.ones((h, w), np.uint8)         # a staircase that runs upwards and leftwards only, against launch order
    for i in range(min(h, w // 3) - 1):      # (rows h - 1 .. 1, three columns a row)
        up[h - 1 - i, w - 3 * i - 3:w - 3 * i] = 0
    up[h - 1, w - 1] = 2
    up[0, 300] = 2                           # right below the previous page's candidate
    pages["seam_then_staircase"] = up
    full = np.zeros((h, w), np.uint8)
    full[h // 2, w // 3] = 2
    pages["all_candidates_one_edge"] = full
    pages["all_candidates_no_edge"] = np.zeros((h, w), np.uint8)
    other = rnd((h, w), 4) % 5                # 0 .. 4: values beyond 2 are no edge either
    pages["random"] = other.astype(np.uint8)
    return pages


@pytest.mark.parametrize("size", LINK_SIZES, ids=[f"{h}x{w}" for h, w in LINK_SIZES])
def test_edge_link_hand_made_maps(prl, cuda_device, size):
    h, w = size
    pages = link_pages(h, w)
    names = list(pages)
    batch = np.stack([pages[k] for k in names])
    got, passes = prl.edge_link(dev(batch, cuda_device), return_passes=True)
    got = got.cpu().numpy()
    print("linking passes:", dict(zip(names, passes.tolist())))
    for i, k in enumerate(names):   # (a serpentine is one component with its edge pixel in it: the whole path)
        want = np.where(batch[i] != 1, 255, 0).astype(np.uint8) if k.startswith("serpentine") else er.edge_link(batch[i])
        assert np.array_equal(got[i], want), k
    by = dict(zip(names, got))
    assert ((by["serpentine_rows"] == 255) == (pages["serpentine_rows"] != 1)).all()
    assert ((by["serpentine_columns"] == 255) == (pages["serpentine_columns"] != 1)).all()
    c = by["corners_words_row_ends"]
    assert c[64 - 6, 256 - 6] == 255 and c[128 + 6, 512 - 6] == 255 and c[10, 63] == 255 and c[21, w - 1] == 255
    assert c[30, w - 1] == 0 and c[31, 0] == 255 and c[h - 1, 300] == 0 and not c[150:160, 100:140].any()
    assert (by["all_candidates_one_edge"] == 255).all() and not by["all_candidates_no_edge"].any()
    p = dict(zip(names, passes.tolist()))
    assert all(1 <= v < 1 << 20 for v in p.values())
    assert p["serpentine_rows"] >= 2 and p["serpentine_columns"] >= 2     # the multi-pass path ran
    assert p["all_candidates_no_edge"] == 1                               # the first pass changed nothing
    assert len(set(p.values())) > 1                                       # pages of one batch finished in different passes


def test_edge_link_small_and_strided(prl, cuda_device):
    import torch

    for h, w in ((1, 1), (1, 70), (70, 1), (2, 129), (65, 64)):
        maps = (rnd((3, h, w), h + w) % 3).astype(np.uint8)
        big = torch.ones((3, h + 2, w + 9), dtype=torch.uint8, device=cuda_device)
        src = big[:, 1:1 + h, 4:4 + w]
        src.copy_(dev(maps, cuda_device))
        got = prl.edge_link(src).cpu().numpy()
        for i in range(3):
            assert np.array_equal(got[i], er.edge_link(maps[i])), (h, w, i)


# ---- composed -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("thr", [(25, 50), (0, 0), (-1, -1), (100, 300)])
def test_canny_equals_its_stages_and_the_restatement(prl, cuda_device, thr):
    from prlib_amd import synth

    sets = [np.stack([rnd((129, 257), 1), blocks(129, 257, 2), rnd((129, 257), 3) >> 4, blocks(129, 257, 4, cell=7)]),
            np.stack([rnd((5, 65), 5), blocks(5, 65, 6)]),
            np.stack([synth.text_page_numpy(300, 420, 3, skew_deg=1.5, shading=0.3), synth.text_page_numpy(300, 420, 4)])]
    for pages in sets:
        d = dev(pages, cuda_device)
        got = prl.canny(d, *thr).cpu().numpy()
        staged = prl.edge_link(prl.canny_classes(d, *thr)).cpu().numpy()
        for i in range(len(pages)):
            want = er.canny(pages[i], *thr)
            assert np.array_equal(got[i], want) and np.array_equal(staged[i], want), (pages.shape, thr, i)


@pytest.mark.parametrize("scan", [0, 1])
def test_canny_on_scans(prl, cuda_device, scan):
    g = scan_page(scan)
    d = dev(g[None], cuda_device)
    got = prl.canny(d, 25, 50).cpu().numpy()[0]
    want = er.canny(g, 25, 50)
    assert np.array_equal(got, want) and 0 < (want == 255).mean() < 0.5
    assert np.array_equal(prl.edge_link(prl.canny_classes(d, 25, 50)).cpu().numpy()[0], want)


@pytest.mark.parametrize("shape", [(900, 1300), (2480, 3508), (511, 300)], ids=["900x1300", "2480x3508", "511x300_no_level"])
def test_document_edges(prl, cuda_device, shape):
    w, h = shape
    pages = np.stack([er.colour_from_gray(scan_page(0, h, w)), np.roll(er.colour_from_gray(scan_page(1, h, w)), 1, axis=2)])
    maps, chosen = prl.document_edges(dev(pages, cuda_device))
    maps = maps.cpu().numpy()
    levels, ow, oh = er.document_edges_geometry(w, h)
    assert prl.document_edges_geometry(w, h) == (levels, ow, oh) and maps.shape == (2, oh, ow)
    assert (levels == 0) == (max(w, h) == 511)
    for i in range(2):
        want, ch = er.document_edges(pages[i])
        assert int(chosen[i]) == ch and np.array_equal(maps[i], want), (shape, i)


def test_document_edges_gray_and_four_channels(prl, cuda_device):
    g = scan_page(1, 700, 520)
    gray_map, ch = prl.document_edges(dev(g, cuda_device))
    assert ch == 0 and np.array_equal(gray_map.cpu().numpy(), er.document_edges(g)[0])
    tie = np.stack([g, g, g], axis=2)
    m3, ch3 = prl.document_edges(dev(tie, cuda_device))
    assert ch3 == 0 and np.array_equal(m3.cpu().numpy(), er.document_edges(tie)[0])     # an exact tie: the first channel
    bgra = er.colour_from_gray(g, 4)
    m4, ch4 = prl.document_edges(dev(bgra, cuda_device))
    want, wch = er.document_edges(bgra)
    assert ch4 == wch and np.array_equal(m4.cpu().numpy(), want)


def test_host_entries(prl, cuda_device):
    img = rnd((67, 131, 3), 9)
    assert np.array_equal(prl.pyr_down(img), er.pyr_down(img)) and np.array_equal(prl.pyr_down(img[:, :, 0], 2), er.pyr_down(img[:, :, 0], 2))
    g = blocks(67, 131, 5)
    assert np.array_equal(prl.canny(g, 25, 50), er.canny(g, 25, 50))
    page = er.colour_from_gray(scan_page(0, 600, 520))
    m, ch = prl.document_edges(page)
    want, wch = er.document_edges(page)
    assert ch == wch and np.array_equal(m, want)


def test_two_calls_back_to_back_on_one_stream(prl, cuda_device):
    import torch

    a, b = rnd((2, 200, 300), 1) >> 3, blocks(200, 300, 2)[None]
    da, db = dev(a, cuda_device), dev(b, cuda_device)
    s = torch.cuda.Stream(device=cuda_device)
    s.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(s):
        ra = prl.canny(da, 25, 50)
        pa = prl.pyr_down(da)
        rb = prl.canny(db, 25, 50)
        pb = prl.pyr_down(pa)
    s.synchronize()
    for i in range(2):
        assert np.array_equal(ra.cpu().numpy()[i], er.canny(a[i], 25, 50))
        assert np.array_equal(pb.cpu().numpy()[i], er.pyr_down(a[i], 2))
    assert np.array_equal(rb.cpu().numpy()[0], er.canny(b[0], 25, 50))


def test_cpp_dropin(prl, cuda_device, tmp_path):
    """prl::resize(cv::Mat) through include/prl/resize.h: both paths, a ROI view, factor 49 on a 2 x 1 page"""
    import subprocess

    from test_edges_cpu import build_dropin

    exe = build_dropin(str(tmp_path))
    img = er.colour_from_gray(scan_page(0, 300, 400))
    tiny = np.array([[[10, 20, 30], [200, 100, 50]]], np.uint8)
    cases = [(img, 2, 3, 0, False), (img, 0, 0, 100, True), (img, -1, 4, 399, False), (img, 0, 0, 400, False), (img, 1, 1, 0, True),
             (tiny, 49, 1, 0, False), (np.ascontiguousarray(img[:, :, 0]), 3, 1, 0, False)]
    for k, (page, fx, fy, ms, roi) in enumerate(cases):
        p3 = page if page.ndim == 3 else page[:, :, None]
        rows, cols, cn = p3.shape
        src, dst = str(tmp_path / f"in{k}.raw"), str(tmp_path / f"out{k}.raw")
        page.tofile(src)
        cmd = [exe, "run", str(rows), str(cols), str(cn), src, dst, str(fx), str(fy), str(ms)]
        r = subprocess.run(cmd + (["roi"] if roi else []), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "resize dropin run: OK" in r.stdout, r.stdout + r.stderr
        want = er.resize(np.ascontiguousarray(p3[2:rows - 3, 3:cols - 4]) if roi else p3, fx, fy, ms)
        assert f"size {want.shape[1]} {want.shape[0]}" in r.stdout, (k, r.stdout)
        assert np.array_equal(np.fromfile(dst, np.uint8).reshape(want.shape), want), k


def test_resize_both_paths(prl, cuda_device):
    tiny = np.array([[[10, 20, 30], [200, 100, 50]]], np.uint8)             # 2 x 1, three channels
    got = prl.resize(dev(tiny, cuda_device), 49, 1, 0).cpu().numpy()
    assert got.shape == (1, 98, 3) and np.array_equal(got, er.resize(tiny, 49, 1, 0))
    assert (got[0, :50] == tiny[0, 0]).all() and (got[0, 50:] == tiny[0, 1]).all()   # column 49 copies source column 0
    pages = rnd((2, 37, 53, 3), 3)
    d = dev(pages, cuda_device)
    for fx, fy in ((1, 1), (2, 3), (3, 2), (49, 1)):
        got = prl.resize(d, fx, fy, 0).cpu().numpy()
        for i in range(2):
            assert np.array_equal(got[i], er.resize(pages[i], fx, fy, 0)), (fx, fy, i)
    for max_size in (53, 52, 20, 1):
        got = prl.resize(d, 0, 0, max_size).cpu().numpy()
        for i in range(2):
            assert np.array_equal(got[i], er.resize(pages[i], 0, 0, max_size)), (max_size, i)
    g = rnd((41, 29), 8)
    assert np.array_equal(prl.resize(g, 2, 2, 0), er.resize(g, 2, 2, 0)) and np.array_equal(prl.resize(g, -1, 5, 16), er.resize(g, -1, 5, 16))
