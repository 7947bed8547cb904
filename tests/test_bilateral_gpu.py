"""cv::bilateralFilter on the device (bilateral.hip) against tests/fbcitb_ref.py, byte for byte: no tolerance and no excluded pixel.
The filter is a fixed float32 sequence per pixel, so a fused multiply-add, a reciprocal multiply in place of the division or another
tap order shows on the pages of test_bilateral_cpu.SENSITIVE, which that file proves sensitive to each."""
import numpy as np
import pytest

import fbcitb_ref as fr
from test_bilateral_cpu import SENSITIVE, sensitive_page

pytestmark = pytest.mark.gpu

# the tile is 64 x 16 pixels, a lane owns 4 adjacent ones
WIDTHS = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129)
HEIGHTS = (1, 2, 15, 16, 17, 33)


def dev_of(page, device):
    import torch

    return torch.from_numpy(np.ascontiguousarray(page)).to(device)


def check(prl, device, page, d, sc, ss):
    got = prl.bilateralFilter(dev_of(page, device), d, sc, ss).cpu().numpy()
    want = fr.bilateral(page, d, sc, ss)
    bad = got != want
    assert got.shape == want.shape and not bad.any(), (page.shape, d, sc, ss, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def test_the_sensitive_pages_and_the_defaults(prl, cuda_device):
    for gen, seed in SENSITIVE:
        check(prl, cuda_device, sensitive_page(gen, seed), 5, 150.0, 150.0)
    check(prl, cuda_device, fr.noise(37, 53, 1, 1), 5, 150.0, 150.0)
    check(prl, cuda_device, fr.smooth_noise(37, 53, 2), 9, 25.0, 4.0)


def test_widths_and_heights_round_the_tile(prl, cuda_device):
    for i, w in enumerate(WIDTHS):
        for j, h in enumerate(HEIGHTS):
            check(prl, cuda_device, fr.smooth_noise(h, w, 100 * i + j), (3, 5, 9)[(i + j) % 3], 30.0, 3.0)


def test_pages_smaller_than_the_radius(prl, cuda_device):
    check(prl, cuda_device, fr.noise(2, 3, 1, 3), 9, 50.0, 3.0)
    check(prl, cuda_device, fr.noise(1, 1, 1, 4), 31, 50.0, 9.0)
    check(prl, cuda_device, fr.noise(3, 2, 3, 5), 31, 50.0, 9.0)
    check(prl, cuda_device, fr.noise(1, 70, 1, 6), 15, 50.0, 9.0)
    check(prl, cuda_device, fr.noise(40, 1, 1, 7), 15, 50.0, 9.0)


@pytest.mark.parametrize("d", range(3, 32, 2))
def test_every_side(prl, cuda_device, d):
    check(prl, cuda_device, fr.smooth_noise(21, 70, d), d, 40.0, 0.4 * d)


def test_d_from_sigma_space_and_the_colour_sigmas(prl, cuda_device):
    page = fr.smooth_noise(37, 53, 11, spread=3)
    for ss in (0.5, 1.0, 2.0, 3.0):   # radius 1, 2, 3, 4 (1.5 * 3 = 4.5 rounds to even)
        check(prl, cuda_device, page, 0, 20.0, ss)
        check(prl, cuda_device, page, -7, 20.0, ss)
    for sc in (-1.0, 0.0, 1.0, 3.0, 150.0):   # <= 0 counts as 1; at 1 the weights of |v - c| >= 14 are denormal or zero
        check(prl, cuda_device, page, 5, sc, 2.0)
        check(prl, cuda_device, fr.noise(37, 53, 1, 12), 5, sc, 2.0)
    check(prl, cuda_device, page, 5, 20.0, -3.0)


@pytest.mark.parametrize("channels", (1, 3, 4))
def test_layouts_and_a_batch_of_three(prl, cuda_device, channels):
    """three different pages with pitched rows, page strides larger than the page and odd base addresses, on both sides; the bytes
    outside every destination row stay untouched, and so does the source"""
    import torch

    n, h, w, c = 3, 37, 53, channels
    sstep, dstep = w * c + 5, w * c + 9
    spage, dpage, soff, doff = h * sstep + 33, h * dstep + 77, 1, 3
    rng = np.random.default_rng(21)
    sbuf = (128 + rng.integers(-20, 21, size=soff + n * spage + 16)).astype(np.uint8)
    shape = (n, h, w, c) if c > 1 else (n, h, w)
    sstr = (spage, sstep, c, 1) if c > 1 else (spage, sstep, 1)
    dstr = (dpage, dstep, c, 1) if c > 1 else (dpage, dstep, 1)
    d_s = torch.from_numpy(sbuf).to(cuda_device)
    src = torch.as_strided(d_s, shape, sstr, storage_offset=soff)
    d_d = torch.full((doff + n * dpage + 16,), 0xA5, dtype=torch.uint8, device=cuda_device)
    dst = torch.as_strided(d_d, shape, dstr, storage_offset=doff)
    host = np.lib.stride_tricks.as_strided(sbuf[soff:], shape, sstr)
    want = np.stack([fr.bilateral(np.ascontiguousarray(host[i]), 7, 12.0, 2.5) for i in range(n)])
    assert len({p.tobytes() for p in want}) == n
    before = d_s.clone()
    assert prl.bilateralFilter(src, 7, 12.0, 2.5, out=dst) is dst
    assert np.array_equal(dst.cpu().numpy(), want)
    assert torch.equal(d_s, before), "the source was written"
    outside = torch.ones_like(d_d, dtype=torch.bool)
    torch.as_strided(outside, shape, dstr, storage_offset=doff).fill_(False)
    assert bool((d_d[outside] == 0xA5).all()), "bytes outside the destination rows were written"
    assert np.array_equal(prl.bilateralFilter(src[2], 7, 12.0, 2.5).cpu().numpy(), want[2]), "a page alone"
    view = host[1][3:30, 5:50]   # the host entry on a view with pitched rows
    assert np.array_equal(prl.bilateralFilter(view, 5, 12.0, 2.5), fr.bilateral(np.ascontiguousarray(view), 5, 12.0, 2.5))


def test_all_255_the_tie_page_and_the_denormal_page(prl, cuda_device):
    for c in (1, 3):
        page = np.full((37, 53, c) if c > 1 else (37, 53), 255, np.uint8)
        assert (prl.bilateralFilter(dev_of(page, cuda_device), 9, 1.0, 3.0).cpu().numpy() == 255).all()
    tie = fr.tie_page()
    got = prl.bilateralFilter(dev_of(tie, cuda_device), 3, fr.TIE_SIGMA_COLOR, fr.TIE_SIGMA_SPACE).cpu().numpy()
    assert got[2, 2] == 10 and got[6, 6] == 12, "10.5 and 11.5 go to the even byte"
    assert np.array_equal(got, fr.bilateral(tie, 3, fr.TIE_SIGMA_COLOR, fr.TIE_SIGMA_SPACE))
    steps = (np.arange(37)[:, None] * 14 + np.arange(53)[None, :] * 12) % 256   # neighbours 12 and 14 apart: denormal weights at both sigmas
    check(prl, cuda_device, steps.astype(np.uint8), 5, fr.TIE_SIGMA_COLOR, 2.0)
    check(prl, cuda_device, steps.astype(np.uint8), 5, 1.0, 2.0)


def test_refused_on_the_device(prl, cuda_device):
    from prlib_amd import _capi

    page = dev_of(fr.noise(8, 8, 1, 1), cuda_device)
    for bad in ((33, 1.0, 1.0), (0, 1.0, 11.0), (5, float("nan"), 1.0)):
        with pytest.raises(_capi.PrlError) as e:
            prl.bilateralFilter(page, *bad)
        assert e.value.status == _capi.PRL_ERR_BAD_ARG
    with pytest.raises(_capi.PrlError) as e:
        prl.bilateralFilter(page, 5, 1.0, 1.0, out=page)
    assert e.value.status == _capi.PRL_ERR_BAD_ARG, "src == dst"
