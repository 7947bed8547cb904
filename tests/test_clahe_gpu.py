"""cv::CLAHE, cv::equalizeHist and EnhanceLocalContrastByCLAHE on the device (clahe.hip) against tests/clahe_ref.py: every byte of
every page and of every tile table equal.  Sizes sit at the edges of the kernels' geometry, named from clahe_ref's copy of their
constants: the interpolation block (BLOCK_W x BLOCK_H), the tables a block stages in LDS (STAGE_TABLES), the rows above which the
histogram kernel splits a tile (HIST_BAND_ROWS)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import clahe_ref as cr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_REF = {}


def ref_luts(page, clip, tiles):
    """clahe_ref.luts, computed once per page and setting: [C, tilesY, tilesX, 256]"""
    key = (page.shape, page.tobytes(), clip, tiles)
    if key not in _REF:
        _REF[key] = cr.luts(page, clip, tiles)
    return _REF[key]


def ref_clahe(page, clip, tiles):
    L = ref_luts(page, clip, tiles)
    if page.ndim == 2:
        return cr.plane_clahe(page, clip, tiles, L[0])
    return np.stack([cr.plane_clahe(np.ascontiguousarray(page[:, :, c]), clip, tiles, L[c]) for c in range(page.shape[2])], axis=-1)


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def check(prl, dev, page, clip=40.0, tiles=(8, 8)):
    """the tables first - a table bug must not hide behind the blend - then the page"""
    import torch

    t = torch.from_numpy(page).to(dev)
    same(prl.claheLuts(t, clip, tiles).cpu().numpy(), ref_luts(page, clip, tiles), ("luts", page.shape, clip, tiles))
    same(prl.clahe(t, clip, tiles).cpu().numpy(), ref_clahe(page, clip, tiles), ("clahe", page.shape, clip, tiles))


@pytest.mark.parametrize("h", range(1, 18))
def test_every_small_side(prl, cuda_device, h):
    """1..17 x 1..17 on the 8 x 8 grid: tile sides 1, 2 and 3, every pad, ties at tile sides 1 and 2, tables from global memory"""
    for w in range(1, 18):
        tw, th, ew, eh, _ = cr.geometry(w, h)
        assert tw in (1, 2, 3) and th in (1, 2, 3) and 0 <= ew - w <= 8
        check(prl, cuda_device, cr.noise(h, w, 1, h), 40.0 if (h + w) % 2 else 0.0)


def test_sizes_around_the_interpolation_block(prl, cuda_device):
    for w in (cr.BLOCK_W - 1, cr.BLOCK_W, cr.BLOCK_W + 1, 2 * cr.BLOCK_W + cr.LANE_PX - 1):
        check(prl, cuda_device, cr.noise(21, w, 1, 1), 3.0)
        check(prl, cuda_device, cr.paper(9, w, 3, 2), 2.0)
    for h in (cr.BLOCK_H - 1, cr.BLOCK_H, cr.BLOCK_H + 1, 2 * cr.BLOCK_H + 1):
        check(prl, cuda_device, cr.noise(h, 37, 1, 3), 3.0)
        check(prl, cuda_device, cr.paper(h, 19, 4, 4), 2.0)


def test_tables_around_the_lds_stage(prl, cuda_device):
    """a page of one block whose grid is T x 1, 1 x T or T x T tiles: the block touches every table, one below, at and above the stage"""
    s = cr.STAGE_TABLES
    for t in (s - 1, s, s + 1):
        page = cr.noise(cr.BLOCK_H, cr.BLOCK_W, 1, t)
        check(prl, cuda_device, page, 2.0, (t, 1))
        check(prl, cuda_device, page, 2.0, (1, t))
    r = int(round(s ** 0.5))
    assert r * r == s
    for t in (r, r + 1):
        check(prl, cuda_device, cr.noise(cr.BLOCK_H - 3, cr.BLOCK_W - 5, 3, t), 40.0, (t, t))
    # two blocks over one grid: one stages, one does not
    check(prl, cuda_device, cr.noise(40, 2 * cr.BLOCK_W, 1, 9), 2.0, (s + 8, 1))


def test_tile_heights_around_the_histogram_split(prl, cuda_device):
    """tile_h = HIST_BAND_ROWS - 1 (extended), HIST_BAND_ROWS (the page divides) and HIST_BAND_ROWS + 1: one band, one band, two"""
    hb = cr.HIST_BAND_ROWS
    for h, th in ((8 * hb - 9, hb - 1), (8 * hb, hb), (8 * hb + 1, hb + 1), (16 * hb + 1, 2 * hb + 1)):
        assert cr.geometry(24, h)[1] == th
        check(prl, cuda_device, cr.paper(h, 24, 1, th), 2.0)
    # a workgroup takes HIST_UNIT_PX // (pixels of a band) bands: two at half HIST_UNIT_PX and just below, one just above
    half = cr.HIST_UNIT_PX // (2 * hb)
    for w in (8 * half - 8, 8 * half, 8 * half + 8):
        assert cr.HIST_UNIT_PX // (cr.geometry(w, 8 * hb)[0] * hb) == (2 if w <= 8 * half else 1)
        check(prl, cuda_device, cr.gradient(8 * hb, w), 2.0)


@pytest.mark.parametrize("tiles", ((1, 1), (1, 8), (8, 1), (3, 5), (64, 64)), ids=str)
def test_grids(prl, cuda_device, tiles):
    for c in (1, 3):
        check(prl, cuda_device, cr.noise(67, 130, c, 5), 40.0, tiles)
    check(prl, cuda_device, cr.paper(67, 130, 1, 6), 2.0, tiles)


@pytest.mark.parametrize("clip", (0.0, 0.5, 2.0, 3.0, 40.0, 1e6))
def test_clip_limits(prl, cuda_device, clip):
    if clip == 0.5:
        assert cr.geometry(130, 67, (8, 8), clip)[4] == 1
    for page in (cr.noise(67, 130, 1, 7), cr.gradient(67, 130), cr.two_valued(67, 130), cr.flat(67, 130, 200)):
        check(prl, cuda_device, page, clip)
    check(prl, cuda_device, cr.two_valued(300, 200, c=1, seed=1), clip)   # tiles of 950 pixels: the clip bites


@pytest.mark.parametrize("kind", ("flat", "two", "noise", "gradient", "paper"))
def test_page_kinds(prl, cuda_device, kind):
    """a flat page is the same-address atomic case: every wavefront of both histogram passes takes the shortcut"""
    import torch

    for h, w in ((67, 130), (256, 520)):
        for c in (1, 3):
            page = {"flat": lambda: cr.flat(h, w, 77, c), "two": lambda: cr.two_valued(h, w, c=c), "noise": lambda: cr.noise(h, w, c, 8),
                    "gradient": lambda: cr.gradient(h, w, c), "paper": lambda: cr.paper(h, w, c, 9)}[kind]()
            check(prl, cuda_device, page, 2.0)
            t = torch.from_numpy(page).to(cuda_device)
            same(prl.equalizeHist(t).cpu().numpy(), cr.equalize(page), ("equalize", kind, h, w, c))
            same(prl.enhanceLocalContrast(t, 2.0, True).cpu().numpy(), cr.equalize(ref_clahe(page, 2.0, (8, 8))), ("enhance", kind, h, w, c))


@pytest.mark.parametrize("channels", (1, 2, 3, 4))
def test_channels(prl, cuda_device, channels):
    import torch

    for h, w in ((13, 16), (67, 130), (cr.BLOCK_H + 2, cr.BLOCK_W + 3)):
        page = cr.noise(h, w, channels, 10)
        check(prl, cuda_device, page, 3.0)
        t = torch.from_numpy(page).to(cuda_device)
        same(prl.enhanceLocalContrast(t, 3.0, False).cpu().numpy(), ref_clahe(page, 3.0, (8, 8)), ("enhance without the flag", h, w, channels))
        same(prl.enhanceLocalContrast(t, 3.0, True).cpu().numpy(), cr.equalize(ref_clahe(page, 3.0, (8, 8))), ("enhance", h, w, channels))
        same(prl.equalizeHist(t).cpu().numpy(), cr.equalize(page), ("equalize", h, w, channels))


def test_equalize_edge_cases(prl, cuda_device):
    import torch

    flat = cr.flat(40, 50, 90)
    one = flat.copy()
    one[3, 4] = 91                    # the first non-empty bin holds all but one pixel
    last = cr.flat(40, 50, 255)
    for page in (flat, one, last, cr.flat(1, 1, 0), cr.two_valued(33, 65)):
        t = torch.from_numpy(page).to(cuda_device)
        same(prl.equalizeHist(t).cpu().numpy(), cr.equalize(page), ("equalize", page.shape))
        same(prl.enhanceLocalContrast(t, 2.0, True).cpu().numpy(), cr.enhance(page, 2.0, True), ("enhance", page.shape))
    assert cr.equalize(one)[3, 4] == 255 and int(cr.equalize(one).astype(int).sum()) == 255


def test_fused_output_histogram(prl, cuda_device):
    """the histogram the interpolation pass counts is histogram(clahe(...)): equalizing the CLAHE result in a call of its own gives
    the fused call's bytes, on pages where one count off would move a table entry"""
    import torch

    for page in (cr.noise(cr.BLOCK_H + 1, cr.BLOCK_W + 1, 3, 11), cr.paper(200, 300, 1, 12), cr.flat(70, 140, 5, 4), cr.gradient(67, 130, 2)):
        t = torch.from_numpy(page).to(cuda_device)
        step1 = prl.clahe(t, 2.0)
        assert np.array_equal(prl.histogram(step1).cpu().numpy().reshape(-1, 256), cr.histogram(ref_clahe(page, 2.0, (8, 8))).reshape(-1, 256))
        same(prl.enhanceLocalContrast(t, 2.0, True).cpu().numpy(), prl.equalizeHist(step1).cpu().numpy(), ("fused == two calls", page.shape))
        same(prl.enhanceLocalContrast(t, 2.0, True).cpu().numpy(), cr.enhance(page, 2.0, True), ("fused == ref", page.shape))


def test_layouts(prl, cuda_device):
    import torch

    h, w = 67, 130
    for c in (1, 3):
        page = cr.noise(h, w, c, 13)
        want, want_eq = ref_clahe(page, 2.0, (8, 8)), cr.enhance(page, 2.0, True)
        p3 = page.reshape(h, w, c)
        # pitched rows, an odd source address, an odd destination address
        buf = torch.full((h * (w * c + 7) + 1,), 0xAB, dtype=torch.uint8, device=cuda_device)
        src = buf[1:].reshape(h, w * c + 7)[:, :w * c].unflatten(1, (w, c))
        src.copy_(torch.from_numpy(p3).to(cuda_device))
        assert src.data_ptr() % 2 == 1 and src.stride(0) == w * c + 7
        view = src if c > 1 else src[:, :, 0]
        same(prl.clahe(view, 2.0).cpu().numpy(), want, ("pitched, odd address", c))
        obuf = torch.zeros(h * (w * c + 3) + 3, dtype=torch.uint8, device=cuda_device)
        out = obuf[3:].reshape(h, w * c + 3)[:, :w * c].unflatten(1, (w, c))
        out = out if c > 1 else out[:, :, 0]
        res = prl.enhanceLocalContrast(view, 2.0, True, out=out)
        assert res.data_ptr() == out.data_ptr()
        same(out.cpu().numpy(), want_eq, ("pitched out", c))
        assert int(obuf[:3].sum()) == 0 and int(obuf[3:].reshape(h, w * c + 3)[:, w * c:].sum()) == 0   # nothing written between the rows
        assert int((buf[1:].reshape(h, w * c + 7)[:, w * c:] != 0xAB).sum()) == 0
        # in place
        t = torch.from_numpy(page).to(cuda_device)
        assert prl.clahe(t, 2.0, out=t).data_ptr() == t.data_ptr()
        same(t.cpu().numpy(), want, ("in place", c))
        t = torch.from_numpy(page).to(cuda_device)
        prl.enhanceLocalContrast(t, 2.0, True, out=t)
        same(t.cpu().numpy(), want_eq, ("in place, with the flag", c))
        t = torch.from_numpy(page).to(cuda_device)
        prl.equalizeHist(t, out=t)
        same(t.cpu().numpy(), cr.equalize(page), ("equalize in place", c))


def test_batch_of_five_different_pages(prl, cuda_device):
    """histograms must not mix between pages: five pages, a page stride that is no multiple of 4"""
    import torch

    h, w = 45, 71
    pages = np.stack([cr.noise(h, w, 1, 20), cr.flat(h, w, 9), cr.gradient(h, w), cr.two_valued(h, w), cr.paper(h, w, 1, 21)])
    stride = h * w + 3
    assert stride % 4 != 0
    buf = torch.zeros(5 * stride, dtype=torch.uint8, device=cuda_device)
    batch = buf.reshape(5, stride)[:, :h * w].unflatten(1, (h, w))
    batch.copy_(torch.from_numpy(pages).to(cuda_device))
    assert batch.stride(0) == stride
    got = prl.clahe(batch, 2.0).cpu().numpy()
    got_l = prl.claheLuts(batch, 2.0).cpu().numpy()
    got_e = prl.enhanceLocalContrast(batch, 2.0, True).cpu().numpy()
    got_q = prl.equalizeHist(batch).cpu().numpy()
    for i in range(5):
        same(got_l[i], ref_luts(pages[i], 2.0, (8, 8)), ("luts of page", i))
        same(got[i], ref_clahe(pages[i], 2.0, (8, 8)), ("page", i))
        same(got_e[i], cr.equalize(ref_clahe(pages[i], 2.0, (8, 8))), ("enhanced page", i))
        same(got_q[i], cr.equalize(pages[i]), ("equalized page", i))
    inplace = batch.clone()
    prl.enhanceLocalContrast(inplace, 2.0, True, out=inplace)
    same(inplace.cpu().numpy(), got_e, "the batch in place")


def test_second_chunk(prl, cuda_device):
    """the hooks build: PRL_HIP_STAGE_CHUNK=2 runs five pages as 2, 2, 1 - the later chunks' offsets into the pages, the workspace
    and the caller's table memory"""
    code = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from prlib_amd import _capi
_capi.use_library(_capi.HOOKS_LIB_PATH)
import torch, prlib_amd as P, clahe_ref as cr
pages = np.stack([cr.noise(33, 50, 3, k) for k in range(5)])
t = torch.from_numpy(pages).cuda()
got, luts, enh, eq = (f.cpu().numpy() for f in (P.clahe(t, 2.0), P.claheLuts(t, 2.0), P.enhanceLocalContrast(t, 2.0, True), P.equalizeHist(t)))
for i in range(5):
    assert np.array_equal(got[i], cr.clahe(pages[i], 2.0)), i
    assert np.array_equal(luts[i], cr.luts(pages[i], 2.0)), i
    assert np.array_equal(enh[i], cr.enhance(pages[i], 2.0, True)), i
    assert np.array_equal(eq[i], cr.equalize(pages[i])), i
print("clahe chunks ok")
'''
    env = dict(os.environ, PRL_HIP_STAGE_CHUNK="2")
    r = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "clahe chunks ok" in r.stdout, r.stdout + r.stderr[-3000:]


def test_large_pages(prl, cuda_device):
    """the only large case: an A4-sized page and a 1024 x 1024 page, each in a batch of 3 (paper, noise, flat)"""
    import torch

    for h, w in ((3508, 2480), (1024, 1024)):
        pages = np.stack([cr.paper(h, w, 1, 30), cr.noise(h, w, 1, 31), cr.flat(h, w, 240)])
        t = torch.from_numpy(pages).to(cuda_device)
        got, got_l, got_e = prl.clahe(t, 2.0).cpu().numpy(), prl.claheLuts(t, 2.0).cpu().numpy(), prl.enhanceLocalContrast(t, 2.0, True).cpu().numpy()
        for i in range(3):
            L = cr.luts(pages[i], 2.0)
            want = cr.plane_clahe(pages[i], 2.0, (8, 8), L[0])
            same(got_l[i], L, ("luts", h, w, i))
            same(got[i], want, ("clahe", h, w, i))
            same(got_e[i], cr.equalize(want), ("enhance", h, w, i))


def test_host_entries_and_dropin(prl, cuda_device, tmp_path):
    """numpy pages through the *_host entries, and the C++ caller of EnhanceLocalContrastByCLAHE (a Mat, a view of one, in place)"""
    from test_clahe_cpu import build_dropin

    page = cr.noise(41, 57, 3, 40)
    same(prl.clahe(page, 2.0, (3, 5)), cr.clahe(page, 2.0, (3, 5)), "clahe, host")
    same(prl.equalizeHist(page[:, :, 0]), cr.equalize(np.ascontiguousarray(page[:, :, 0])), "equalize, host")
    same(prl.enhanceLocalContrast(page, 2.0, True), cr.enhance(page, 2.0, True), "enhance, host")
    exe = build_dropin(str(tmp_path))
    src, out = str(tmp_path / "in.raw"), str(tmp_path / "out.raw")
    page.tofile(src)

    def run(*args):
        r = subprocess.run([exe, "run", "41", "57", "3", src, out] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "clahe dropin run: OK" in r.stdout, r.stdout + r.stderr
        return np.fromfile(out, np.uint8)

    same(run("enhance", 2.0, 1).reshape(41, 57, 3), cr.enhance(page, 2.0, True), "dropin")
    same(run("enhance", 40.0, 0).reshape(41, 57, 3), cr.enhance(page, 40.0, False), "dropin without the flag")
    same(run("inplace", 2.0, 1).reshape(41, 57, 3), cr.enhance(page, 2.0, True), "dropin in place")
    view = np.ascontiguousarray(page[2:38, 3:53])
    same(run("view", 2.0, 1).reshape(36, 50, 3), cr.enhance(view, 2.0, True), "dropin on a view")
    same(run("clahe", 3.0, 5, 3).reshape(41, 57, 3), cr.clahe(page, 3.0, (5, 3)), "prl::clahe")
    same(run("equalize").reshape(41, 57, 3), cr.equalize(page), "prl::equalizeHist")
