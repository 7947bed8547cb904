"""prl::basicDeblur and the float32 cv::GaussianBlur under it on the device (deblur.hip) against tests/deblur_ref.py, bit for bit:
float planes by their bit patterns, bytes by value, every sample of every case.  Sizes sit at the edges of k_deblur's geometry,
named from deblur_ref's restatement of it: the tile width (256, 128, 64 or 32 samples, by the LDS the ring needs) and the rows a
workgroup walks."""
import os
import subprocess

import numpy as np
import pytest

import deblur_ref as dr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_REF = {}


def ref_blur(page, ksize, sx, sy):
    """deblur_ref.blur, computed once per page and kernel"""
    key = (page.shape, page.tobytes(), ksize, sx, sy)
    if key not in _REF:
        _REF[key] = dr.blur(page, ksize, sx, sy)
    return _REF[key]


def check_blur(prl, dev, page, ksize=(0, 0), sx=9.0, sy=0.0):
    import torch

    got = prl.gaussianBlurF32(torch.from_numpy(page).to(dev), ksize, sx, sy).cpu().numpy()
    want = ref_blur(page, ksize, sx, sy)
    assert got.dtype == np.float32 and got.shape == want.shape
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), (page.shape, ksize, sx, sy, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def check_deblur(prl, dev, page, k=0, sx=9.0, sy=0.0, weight=0.75):
    import torch

    got = prl.basicDeblur(torch.from_numpy(page).to(dev), k, sx, sy, weight).cpu().numpy()
    want = dr.deblur_from(page, ref_blur(page, (k, k), sx, sy), weight)
    assert got.dtype == np.uint8 and got.shape == want.shape
    bad = got != want
    assert not bad.any(), (page.shape, k, sx, sy, weight, int(bad.sum()), np.argwhere(bad)[:4].tolist())


# ---- the float entry ---------------------------------------------------------------------------------------------------------------

def test_pages_narrower_and_shorter_than_the_radius(prl, cuda_device):
    """n = 73 on sides of 1, 2, 3 and 7: the border reflects more than once"""
    for h in (1, 2, 3, 7):
        for w in (1, 2, 3, 7):
            check_blur(prl, cuda_device, dr.noise(h, w, 1, 1))
            check_blur(prl, cuda_device, dr.noise(h, w, 3 if (h + w) % 2 else 4, 2))


# a kernel per tile width: (side, sigma) -> 256, 128, 64, 32 samples on a gray page
TILE_KERNELS = [(9, 0.0), (73, 9.0), (129, 0.0), (255, 0.0)]


@pytest.mark.parametrize("n,sigma", TILE_KERNELS, ids=lambda v: str(v))
def test_widths_around_the_tile(prl, cuda_device, n, sigma):
    tw = dr.tile_width(n, n, 1)
    assert tw == {9: 256, 73: 128, 129: 64, 255: 32}[n]
    for w in (tw - 1, tw, tw + 1):
        check_blur(prl, cuda_device, dr.noise(6, w, 1, 3), (n, n), sigma)
    # interleaved: the tile counts samples, and a pixel may straddle two tiles
    for c in (3, 4):
        tw = dr.tile_width(n, n, c)
        w = (2 * tw + c - 1) // c
        check_blur(prl, cuda_device, dr.noise(4, w, c, 4), (n, n), sigma)
        check_blur(prl, cuda_device, dr.noise(4, w + 1, c, 4), (n, n), sigma)


@pytest.mark.parametrize("ny", (3, 25))
def test_heights_around_a_workgroup_s_rows(prl, cuda_device, ny):
    rows = dr.rows_per_group(ny, 1 << 20)
    assert rows == {3: 96, 25: 150}[ny]
    for h in (rows - 1, rows, rows + 1, 2 * rows + 1):
        assert dr.rows_per_group(ny, h) == min(h, rows)
        check_blur(prl, cuda_device, dr.noise(h, 37, 1, 5), (5, ny), 0.0)
    check_blur(prl, cuda_device, dr.noise(rows + 1, 21, 3, 6), (ny, ny), 2.0)


@pytest.mark.parametrize("n", (1, 3, 5, 7, 9, 73, dr.MAX_SIDE))
def test_every_row_pass_form(prl, cuda_device, n):
    """n = 3, 5: centre, then pairs; the others in ascending order; with the tables (no sigma) and without"""
    for sigma in (0.0, 1.25):
        check_blur(prl, cuda_device, dr.noise(50, 70, 1, 7), (n, n), sigma)
        check_blur(prl, cuda_device, dr.noise(20, 33, 3, 8), (n, n), sigma)
    check_blur(prl, cuda_device, dr.checkerboard(50, 70), (n, n), 0.0)


def test_sides_that_differ(prl, cuda_device):
    for c in (1, 2, 3, 4):
        page = dr.noise(40, 45, c, 9)
        check_blur(prl, cuda_device, page, (0, 0), 1.0, 3.0)      # 9 x 25, each side with its sigma
        check_blur(prl, cuda_device, page, (1, 9), 0.0, 0.0)
        check_blur(prl, cuda_device, page, (9, 1), 0.0, 0.0)
        check_blur(prl, cuda_device, page, (25, 9), 3.0, 1.0)
        check_blur(prl, cuda_device, page, (7, 7), 2.0, 2.0 + 1e-9)   # equal sides, weights not shared
    assert dr.plan(0, 0, 1.0, 3.0)[:2] == (9, 25)


# ---- the fused entry ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("channels", (1, 3, 4))
def test_deblur_weights_and_pages(prl, cuda_device, channels):
    """beta = 0 (weight 1), alpha = 1 with beta = -1 (0.5), saturation at both ends (2.0 and 0.0), the header default"""
    pages = [dr.noise(60, 70, channels, 10), dr.checkerboard(60, 70, channels), dr.flat(30, 40, 0, channels), dr.flat(30, 40, 255, channels)]
    for weight in (0.75, 0.5, 1.0, 2.0, 0.0):
        for page in pages:
            check_deblur(prl, cuda_device, page, 0, 9.0, 0.0, weight)
    check_deblur(prl, cuda_device, pages[0], 5, 0.0, 0.0, 0.75)
    check_deblur(prl, cuda_device, pages[1], 3, 1.0, 2.0, 1.5)
    check_deblur(prl, cuda_device, pages[0], 1, 0.0, 0.0, 0.75)
    # the cases do saturate: the default on noise at both ends (1.5 x - 0.5 g runs from about -64 to 319), 4 x + 2 g at 255, -2 g at 0
    want = dr.deblur(pages[0], 0, 9.0, 0.0, 0.75)
    assert want.min() == 0 and want.max() == 255 and 0 < int((want == 0).sum()) < want.size // 2
    assert dr.deblur(pages[0], 0, 9.0, 0.0, 2.0).max() == 255 and dr.deblur(pages[0], 0, 9.0, 0.0, 0.0).max() == 0


@pytest.mark.parametrize("channels", (1, 3, 4))
def test_layouts_and_a_batch_of_three(prl, cuda_device, channels):
    """pitched rows, odd base addresses, page strides larger than the page, on both sides; the bytes outside every destination row
    stay untouched, and so does the source"""
    import torch

    n, h, w, c = 3, 41, 67, channels
    sstep, dstep = w * c + 5, w * c + 9
    spage, dpage, soff, doff = h * sstep + 33, h * dstep + 77, 1, 3
    rng = np.random.default_rng(21)
    sbuf = rng.integers(0, 256, size=soff + n * spage + 16, dtype=np.uint8)
    shape = (n, h, w, c) if c > 1 else (n, h, w)
    sstr = (spage, sstep, c, 1) if c > 1 else (spage, sstep, 1)
    dstr = (dpage, dstep, c, 1) if c > 1 else (dpage, dstep, 1)
    d_s = torch.from_numpy(sbuf).to(cuda_device)
    src = torch.as_strided(d_s, shape, sstr, storage_offset=soff)
    d_d = torch.full((doff + n * dpage + 16,), 0xA5, dtype=torch.uint8, device=cuda_device)
    dst = torch.as_strided(d_d, shape, dstr, storage_offset=doff)
    assert src.data_ptr() % 2 == 1 and dst.data_ptr() % 2 == 1
    host = np.lib.stride_tricks.as_strided(sbuf[soff:], shape, sstr)
    want = np.stack([dr.deblur(np.ascontiguousarray(host[i]), 9, 2.0, 0.0, 0.75) for i in range(n)])
    assert len({p.tobytes() for p in want}) == n
    before = d_s.clone()
    assert prl.basicDeblur(src, 9, 2.0, 0.0, 0.75, out=dst) is dst
    assert np.array_equal(dst.cpu().numpy(), want)
    assert torch.equal(d_s, before), "the source was written"
    outside = torch.ones_like(d_d, dtype=torch.bool)
    torch.as_strided(outside, shape, dstr, storage_offset=doff).fill_(False)
    assert bool((d_d[outside] == 0xA5).all()), "bytes outside the destination rows were written"
    for i in (0, 2):   # a page alone, at its own odd address
        assert np.array_equal(prl.basicDeblur(src[i], 9, 2.0, 0.0, 0.75).cpu().numpy(), want[i])
    # the float entry into a pitched plane
    fbuf = torch.full((n * (h * (w * c + 3) + 5),), -1.0, dtype=torch.float32, device=cuda_device)
    fstr = (h * (w * c + 3) + 5, w * c + 3, c, 1) if c > 1 else (h * (w * c + 3) + 5, w * c + 3, 1)
    fdst = torch.as_strided(fbuf, shape, fstr)
    prl.gaussianBlurF32(src, (9, 9), 2.0, 0.0, out=fdst)
    wantf = np.stack([dr.blur(np.ascontiguousarray(host[i]), (9, 9), 2.0, 0.0) for i in range(n)])
    assert dr.same_bits(fdst.cpu().numpy(), wantf)
    fout = torch.ones_like(fbuf, dtype=torch.bool)
    torch.as_strided(fout, shape, fstr).fill_(False)
    assert bool((fbuf[fout] == -1.0).all())


def test_no_pages_and_statuses_before_any_launch(prl, cuda_device):
    import torch

    from prlib_amd import _capi

    L = _capi.lib()
    src = torch.from_numpy(dr.noise(20, 32, 1, 11)).to(cuda_device)
    dst = torch.full((20, 32), 7, dtype=torch.uint8, device=cuda_device)
    fdst = torch.full((20, 32), -3.0, dtype=torch.float32, device=cuda_device)
    s, d, fd = src.data_ptr(), dst.data_ptr(), fdst.data_ptr()

    def fused(n=1, c=1, k=0, sx=9.0, sy=0.0, wt=0.75, sp=s, ss=32, w=32, h=20, dp=d, ds=32):
        return L.prl_hip_basic_deblur_batch_device(n, c, k, sx, sy, wt, sp, ss * h, ss, w, h, dp, ds * h, ds, None)

    def blur(n=1, c=1, k=0, sx=9.0, sy=0.0, sp=s, ss=32, w=32, h=20, dp=fd, ds=128):
        return L.prl_hip_gaussian_blur_f32_batch_device(n, c, k, k, sx, sy, sp, ss * h, ss, w, h, dp, ds * h, ds, None)

    E, W, A = _capi.PRL_ERR_EMPTY, _capi.PRL_ERR_BAD_WINDOW, _capi.PRL_ERR_BAD_ARG
    for f in (fused, blur):
        assert f(n=0) == 0                                            # no pages: nothing happens
        assert f(w=0) == E and f(k=4) == W and f(k=0, sx=0.0) == W and f(k=257) == W
        assert f(c=5) == A and f(n=-1) == A and f(ss=31) == A and f(sp=None) == A and f(k=3, sx=float("nan")) == A
        assert f(dp=s, ds=32 if f is fused else 128) == A             # in place
    assert fused(wt=float("inf")) == A and blur(dp=fd + 2) == A
    torch.cuda.synchronize()
    assert bool((dst == 7).all()) and bool((fdst == -3.0).all())
    assert fused() == 0 and blur() == 0
    torch.cuda.synchronize()
    page = src.cpu().numpy()
    assert np.array_equal(dst.cpu().numpy(), dr.deblur(page)) and dr.same_bits(fdst.cpu().numpy(), dr.blur(page))


def test_host_entries_equal_the_device_entries(prl, cuda_device):
    import torch

    for c in (1, 3, 4):
        page = dr.noise(45, 52, c, 12)
        t = torch.from_numpy(page).to(cuda_device)
        assert np.array_equal(prl.basicDeblur(page), prl.basicDeblur(t).cpu().numpy())
        assert dr.same_bits(prl.gaussianBlurF32(page, (0, 0), 1.0, 3.0), prl.gaussianBlurF32(t, (0, 0), 1.0, 3.0).cpu().numpy())
        view = page[3:40, 5:47]   # a view with pitched rows through the host entry
        assert np.array_equal(prl.basicDeblur(view, 7, 0.0, 0.0, 1.25), dr.deblur(np.ascontiguousarray(view), 7, 0.0, 0.0, 1.25))
    assert np.array_equal(prl.basicDeblur(page), dr.deblur(page))


def test_the_largest_case_with_the_defaults(prl, cuda_device):
    """one 300 x 520 page: several tiles across, the rows of one workgroup down, 73 x 73"""
    page = dr.noise(300, 520, 1, 13)
    check_blur(prl, cuda_device, page)
    check_deblur(prl, cuda_device, page)
    colour = dr.noise(120, 173, 3, 14)
    check_deblur(prl, cuda_device, colour)


# ---- the C++ layer -----------------------------------------------------------------------------------------------------------------

def test_dropin_caller_agrees_with_python_on_the_defaults(prl, cuda_device, tmp_path):
    from test_deblur_cpu import build_dropin

    exe = build_dropin(str(tmp_path))

    def run(page, *how):
        h, w, c = page.shape if page.ndim == 3 else page.shape + (1,)
        src, out = os.path.join(str(tmp_path), "in.raw"), os.path.join(str(tmp_path), "out.raw")
        page.tofile(src)
        r = subprocess.run([exe, "run", str(h), str(w), str(c), src, out] + [str(v) for v in how], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "deblur dropin run: OK" in r.stdout, r.stdout + r.stderr
        return np.fromfile(out, np.uint8)

    gray, bgra = dr.noise(40, 50, 1, 15), dr.noise(40, 50, 4, 16)
    for page in (gray, dr.noise(40, 50, 3, 17), bgra):
        want = prl.basicDeblur(page)
        assert np.array_equal(want, dr.deblur(page))
        assert np.array_equal(run(page, "defaults").reshape(page.shape), want)
        assert np.array_equal(run(page, "inplace").reshape(page.shape), want)       # the output Mat is the input Mat
    view = np.ascontiguousarray(bgra[2:37, 3:46])                                    # Rect(3, 2, cols - 7, rows - 5) of four channels
    assert np.array_equal(run(bgra, "view").reshape(view.shape), dr.deblur(view))
    assert np.array_equal(run(gray, 5, 1.5, 0.0, 1.0).reshape(gray.shape), dr.deblur(gray, 5, 1.5, 0.0, 1.0))
