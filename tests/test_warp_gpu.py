"""prl::warpCrop / cv::warpPerspective (warp.hip) on the MI355X: every output byte against the numpy restatement of
tests/warp_ref.py, no tolerance - the result sizes where the kernel can go wrong (one row, rows that are no multiple of the
workgroup's four, one column, the 64-column and the 341-column block seams, the 256-pixel segment), two page sizes, matrices that
keystone mildly, put the horizon into the result, throw most taps outside, drive the fixed-point coordinates into both clamps,
and one that separates OpenCV's block rule from a plain walk; 1..4 channels, strided layouts, every destination alignment, both
border modes, several pages of different size in one call, warp_crop end to end on a scan, the host entry and the C++ drop-in."""
import functools
import os
import subprocess

import numpy as np
import pytest

import warp_ref as wr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE_IDS = [f"{ow}x{oh}" for ow, oh in wr.SIZES]
SRC_IDS = [f"{w}x{h}" for w, h in wr.SOURCES]
VALUE = (200.4, 7.5, 300.0, -20.0)   # rounds to 200, 8 (half to even), saturates to 255 and 0


def _mismatch(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.argwhere(got != want)
    return int(bad.shape[0]), bad[:5].tolist()


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(tensors):
    import torch

    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in tensors]


@functools.lru_cache(maxsize=None)
def _pages(source, ch):
    """the four families at one source size: N x H x W x ch"""
    w, h = source
    return np.stack([p for _, p in wr.families(w, h, ch, seed=w + ch)])


@functools.lru_cache(maxsize=None)
def _want(source, ch, size, name, border, value=VALUE):
    """the restatement's result for every family page; computed once and shared"""
    (sw, sh), (ow, oh) = source, size
    m, inv = wr.matrix_case(name, sw, sh, ow, oh)
    return [wr.warp_perspective(p, m, ow, oh, bool(inv), border, value) for p in _pages(source, ch)]


# ---- every size, every matrix -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("source", wr.SOURCES, ids=SRC_IDS)
@pytest.mark.parametrize("size", wr.SIZES, ids=SIZE_IDS)
def test_every_byte_gray(prl, cuda_device, size, source):
    (sw, sh), (ow, oh) = source, size
    pages = _cuda(_pages(source, 1)[:, :, :, 0])
    for name in wr.MATRICES:
        m, inv = wr.matrix_case(name, sw, sh, ow, oh)
        got = _host(prl.warp_perspective(pages, m, (ow, oh), inverse_map=bool(inv), border_mode=wr.BORDER_CONSTANT, border_value=VALUE))
        for g, w in zip(got, _want(source, 1, size, name, wr.BORDER_CONSTANT)):
            n, where = _mismatch(g, w[:, :, 0])
            assert n == 0, (name, n, where)


@pytest.mark.parametrize("ch", [3, 4])
@pytest.mark.parametrize("border", [wr.BORDER_CONSTANT, wr.BORDER_REPLICATE], ids=["constant", "replicate"])
@pytest.mark.parametrize("size", [(1, 1), (65, 3), (257, 17), (400, 3), (400, 16)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_byte_colour_both_borders(prl, cuda_device, size, border, ch):
    source = wr.SOURCES[0]
    (sw, sh), (ow, oh) = source, size
    pages = _cuda(_pages(source, ch))
    for name in wr.MATRICES:
        m, inv = wr.matrix_case(name, sw, sh, ow, oh)
        got = _host(prl.warp_perspective(pages, m, (ow, oh), inverse_map=bool(inv), border_mode=border, border_value=VALUE))
        for g, w in zip(got, _want(source, ch, size, name, border)):
            n, where = _mismatch(g, w)
            assert n == 0, (name, n, where)


@pytest.mark.parametrize("size", [(63, 17), (400, 16)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_replicate_gray_large_source(prl, cuda_device, size):
    source = wr.SOURCES[1]
    (sw, sh), (ow, oh) = source, size
    pages = _cuda(_pages(source, 1)[:, :, :, 0])
    for name in wr.MATRICES:
        m, inv = wr.matrix_case(name, sw, sh, ow, oh)
        got = _host(prl.warp_perspective(pages, m, (ow, oh), inverse_map=bool(inv), border_mode=wr.BORDER_REPLICATE))
        for g, w in zip(got, _want(source, 1, size, name, wr.BORDER_REPLICATE)):
            n, where = _mismatch(g, w[:, :, 0])
            assert n == 0, (name, n, where)


def test_two_channels_through_the_c_entry(prl, cuda_device):
    """the Python layer takes any channel count the entry takes; 2 channels, both borders, a size with seams"""
    source, size = wr.SOURCES[0], (257, 17)
    (sw, sh), (ow, oh) = source, size
    pages = _cuda(_pages(source, 2))
    for border in (wr.BORDER_CONSTANT, wr.BORDER_REPLICATE):
        for name in ("mild", "outside", "cancel"):
            m, inv = wr.matrix_case(name, sw, sh, ow, oh)
            got = _host(prl.warp_perspective(pages, m, (ow, oh), inverse_map=bool(inv), border_mode=border, border_value=VALUE))
            for g, w in zip(got, _want(source, 2, size, name, border)):
                assert _mismatch(g, w)[0] == 0, (name, border)


# ---- layouts ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ch", [1, 3])
def test_strided_rows_and_every_destination_alignment(prl, cuda_device, ch):
    """source rows and pages with padding; the destination begins 0..3 bytes behind a dword boundary and has padded rows.  The
    padding and everything else outside the results keeps its bytes."""
    import torch

    source, size = wr.SOURCES[0], (257, 3)
    (sw, sh), (ow, oh) = source, size
    pages = _pages(source, ch)
    n = pages.shape[0]
    big = torch.full((n, sh + 2, sw * ch + 13), 99, dtype=torch.uint8, device="cuda")
    view = big[:, 1:sh + 1, 5:5 + sw * ch].unflatten(2, (sw, ch))
    view.copy_(_cuda(pages))
    name = "mild"
    m, inv = wr.matrix_case(name, sw, sh, ow, oh)
    want = _want(source, ch, size, name, wr.BORDER_CONSTANT)
    for off in range(4):
        row = ow * ch + 7
        flat = torch.full((n * (oh + 1) * row + 8,), 171, dtype=torch.uint8, device="cuda")
        out = flat[off:off + n * (oh + 1) * row].view(n, oh + 1, row)[:, :, :ow * ch].unflatten(2, (ow, ch))
        assert out.data_ptr() % 4 == off
        got = prl.warp_perspective(view, m, (ow, oh), inverse_map=bool(inv), border_value=VALUE, out=out)
        for g, w in zip(_host(got), want):
            assert _mismatch(g, w)[0] == 0, off
        keep = flat.cpu().numpy().copy()
        body = keep[off:off + n * (oh + 1) * row].reshape(n, oh + 1, row)
        assert (body[:, :oh, ow * ch:] == 171).all() and (body[:, oh:] == 171).all() and (keep[:off] == 171).all() and (keep[off + n * (oh + 1) * row:] == 171).all()
    assert (big[:, 0] == 99).all() and (big[:, :, :5] == 99).all()


def test_pages_with_their_own_matrix_and_size(prl, cuda_device):
    """seven pages, seven matrices, seven sizes in one call; the bytes of a destination page outside its own result stay"""
    import torch

    source = wr.SOURCES[1]
    sw, sh = source
    fam = _pages(source, 3)
    sizes = [(400, 16), (1, 1), (65, 17), (257, 3), (63, 1), (64, 16), (400, 3)]
    pages = np.stack([fam[i % fam.shape[0]] for i in range(len(sizes))])
    mats, want = [], []
    for (ow, oh), name, p in zip(sizes, wr.MATRICES, pages):
        m, inv = wr.matrix_case(name, sw, sh, ow, oh)
        mats.append(m if inv else wr.invert3(m))
        want.append(wr.warp_perspective(p, mats[-1], ow, oh, True, wr.BORDER_CONSTANT, VALUE))
    out = torch.full((len(sizes), 18, 401, 3), 123, dtype=torch.uint8, device="cuda")
    got = prl.warp_perspective(_cuda(pages), np.array(mats), sizes, inverse_map=True, border_value=VALUE, out=out)
    host = out.cpu().numpy()
    for i, ((ow, oh), g, w) in enumerate(zip(sizes, _host(got), want)):
        assert _mismatch(g, w)[0] == 0, i
        rest = host[i].copy()
        rest[:oh, :ow] = 123
        assert (rest == 123).all(), i


def test_async_calls_back_to_back(prl, cuda_device):
    """two calls in a row on one stream with different records: the second call's records must not reach the first call's kernel"""
    source = wr.SOURCES[0]
    sw, sh = source
    pages = _cuda(_pages(source, 1)[:, :, :, 0])
    cases = [("mild", (400, 17)), ("outside", (257, 16)), ("mild_inverse", (65, 3))]
    outs = []
    for name, (ow, oh) in cases:
        m, inv = wr.matrix_case(name, sw, sh, ow, oh)
        outs.append(prl.warp_perspective(pages, m, (ow, oh), inverse_map=bool(inv), border_value=VALUE))
    for (name, size), got in zip(cases, outs):
        for g, w in zip(_host(got), _want(source, 1, size, name, wr.BORDER_CONSTANT)):
            assert _mismatch(g, w[:, :, 0])[0] == 0, name


# ---- warp_crop, the host entry, the drop-in ---------------------------------------------------------------------------------------

QUAD = [38, 52, 851, 21, 880, 1262, 15, 1240]   # a hand-picked keystone inside the 900 x 1300 crop


@functools.lru_cache(maxsize=None)
def _scan():
    z = np.load(os.path.join(ROOT, "tests", "golden", "stages", "chain_0004_x90_y150_900x1300.npz"))
    return np.ascontiguousarray(z["bgr"])


@functools.lru_cache(maxsize=None)
def _scan_want(ratio, border):
    return wr.warp_crop(_scan(), QUAD, ratio, border, (255, 255, 255, 0))


def test_warp_crop_on_a_scan(prl, cuda_device):
    img = _scan()
    assert img.shape == (1300, 900, 3)
    for ratio, border in ((-1.0, wr.BORDER_CONSTANT), (1.4142, wr.BORDER_REPLICATE)):
        want = _scan_want(ratio, border)
        assert prl.warp_crop_size(QUAD, ratio) == (want.shape[1], want.shape[0])
        got = _host(prl.warp_crop(_cuda(img[None]), QUAD, ratio, border, (255, 255, 255, 0)))[0]
        n, where = _mismatch(got, want)
        assert n == 0, (ratio, n, where)
    assert _scan_want(-1.0, wr.BORDER_CONSTANT).shape == (1241, 865, 3)   # sqrt(865^2 + 22^2) = 865.3, sqrt(29^2 + 1241^2) = 1241.3


def test_warp_crop_several_quads(prl, cuda_device):
    """small pages, one quad each: a quad partly outside the page, one that turns it round, one with the identity's corners"""
    source = wr.SOURCES[1]
    sw, sh = source
    pages = _pages(source, 3)
    quads = [[10, 8, 280, 3, 295, 120, 4, 126], [-30, -10, 200, 20, 350, 160, 20, 100], [sw, 0, 0, 0, 0, sh, sw, sh], [0, 0, sw, 0, sw, sh, 0, sh]]
    got = _host(prl.warp_crop(_cuda(pages), np.array(quads), -1.0, wr.BORDER_CONSTANT, VALUE))
    for p, q, g in zip(pages, quads, got):
        assert _mismatch(g, wr.warp_crop(p, q, -1.0, wr.BORDER_CONSTANT, VALUE))[0] == 0, q
    assert np.array_equal(got[3], pages[3])


def test_host_entry(prl, cuda_device):
    img = _scan()
    got = prl.warp_crop_host(img, QUAD, -1.0, wr.BORDER_CONSTANT, (255, 255, 255, 0))
    assert _mismatch(got, _scan_want(-1.0, wr.BORDER_CONSTANT))[0] == 0
    # a strided host image (a view with padded rows), one channel, replicate
    source = wr.SOURCES[0]
    sw, sh = source
    padded = np.full((sh, sw + 9), 5, np.uint8)
    padded[:, :sw] = _pages(source, 1)[0, :, :, 0]
    quad = [3, 2, 60, 5, 64, 40, 1, 43]
    got = prl.warp_crop_host(padded[:, :sw], quad, 0.5, wr.BORDER_REPLICATE)
    assert _mismatch(got, wr.warp_crop(padded[:, :sw], quad, 0.5, wr.BORDER_REPLICATE))[0] == 0


def test_cpp_dropin(prl, cuda_device, tmp_path):
    """prl::warpCrop(cv::Mat) through include/prl/warp.h: both overloads, a ROI view, both borders"""
    from test_warp_cpu import build_dropin

    exe = build_dropin(str(tmp_path))
    img = _scan()[:400, :300]
    rows, cols, cn = img.shape
    src = str(tmp_path / "in.raw")
    img.tofile(src)
    cases = [("points", -1.0, 0, (255, 254, 253, 0), [12, 9, 280, 20, 290, 380, 5, 390], False),
             ("coords", 1.5, 1, (0, 0, 0, 0), [12, 9, 280, 20, 290, 380, 5, 390], True)]
    for k, (how, ratio, border, value, quad, roi) in enumerate(cases):
        dst = str(tmp_path / f"out{k}.raw")
        cmd = [exe, "run", str(rows), str(cols), str(cn), src, dst, how, repr(ratio), str(border)] + [repr(float(v)) for v in value] + [str(q) for q in quad]
        r = subprocess.run(cmd + (["roi"] if roi else []), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "warp dropin run: OK" in r.stdout, r.stdout + r.stderr
        view = img[2:rows - 3, 3:cols - 4] if roi else img
        want = wr.warp_crop(view, quad, ratio, border, value)
        assert f"size {want.shape[1]} {want.shape[0]}" in r.stdout, r.stdout
        got = np.fromfile(dst, np.uint8).reshape(want.shape)
        assert _mismatch(got, want)[0] == 0, how
