"""prl::rotate's kernels (rotate.hip: k_warp, k_rot90) at the smallest shapes that reach each of their seams, against oracle.rotate,
which tests/test_rotate_cpu.py pins to the independent model of tests/rotate_ref.py on these very pages: 0 differing bytes."""
import ctypes as C

import numpy as np
import pytest

import rotate_cases as rc

pytestmark = pytest.mark.gpu

WARP = rc.warp_cases()
ROT90 = rc.rot90_cases()


def _run(prl, oracle, cuda_device, p, angles):
    """one batch of len(angles) copies of p, one angle per page, through prlib_amd.rotate"""
    import torch

    t = torch.from_numpy(np.stack([p] * len(angles))).to(cuda_device)
    outs = prl.rotate(t, angles)
    for a, o in zip(angles, outs):
        want = oracle.rotate(p, a)
        got = o.cpu().numpy()
        assert got.shape == want.shape, (a, got.shape, want.shape)
        assert np.array_equal(got, want), (a, int((got != want).sum()))


@pytest.mark.parametrize("case", WARP, ids=[x[0] for x in WARP])
def test_warp_segments_and_rows(prl, oracle, cuda_device, case):
    """k_warp over one to four 256-column workgroups, every residue of the canvas side modulo its 4 rows, 1 to 4 channels, landscape
    and portrait pages (the source bounds differ from the canvas on both axes), pages one pixel thin."""
    _, h, w, c, angles, seed, text = case
    _run(prl, oracle, cuda_device, rc.page(h, w, c, seed, text), angles)


@pytest.mark.parametrize("case", ROT90, ids=[x[0] for x in ROT90])
def test_rot90_tiles_and_half_turn(prl, oracle, cuda_device, case):
    """k_rot90's 32 x 32 tiles, ragged on either axis or both, and the half turn inside k_warp"""
    _, h, w, c, angles, seed = case
    _run(prl, oracle, cuda_device, rc.page(h, w, c, seed), angles)


@pytest.mark.parametrize("dst_off", [0, 1, 2, 3])
@pytest.mark.parametrize("c", [1, 3])
def test_views_and_guard_bytes(prl, oracle, cuda_device, c, dst_off):
    """Five pages of 300 x 77 with the angles 2, 90, 180, 270, -33 in one call of prl_hip_rotate_batch_device: results of 300 x 300,
    77 x 300, 300 x 77, 77 x 300 and 300 x 300 inside one grid sized by the largest.  The source is a view at a byte offset into a
    larger buffer of random bytes with a pitch of w * c + 5, the destination a view at byte offset 0 .. 3 with an odd pitch into a
    buffer of 7s: every page equals the oracle's, and every byte outside each page's own oh x ow * c rectangle is still 7."""
    import torch

    from prlib_amd import _capi

    w, h, n = rc.VIEW_W, rc.VIEW_H, len(rc.VIEW_ANGLES)
    src_off = (3 * dst_off + 1) % 4
    pages = rc.view_pages(c)
    rng = np.random.default_rng(40 + dst_off)
    s_step, ln = w * c + 5, max(w, h)
    s_page = h * s_step + 11
    src = rng.integers(0, 256, src_off + n * s_page + 64, dtype=np.uint8)
    for i, p in enumerate(pages):
        rows = np.lib.stride_tricks.as_strided(src[src_off + i * s_page:], (h, w * c), (s_step, 1))
        rows[:] = p.reshape(h, w * c)
    d_step = ln * c + 7
    assert d_step % 2 == 1 and s_step % 4 != 0
    d_page = ln * d_step + 13
    want = np.full(dst_off + n * d_page + 64, 7, np.uint8)
    for i, (p, a) in enumerate(zip(pages, rc.VIEW_ANGLES)):
        r = oracle.rotate(p, a)
        oh, ow = r.shape[:2]
        np.lib.stride_tricks.as_strided(want[dst_off + i * d_page:], (oh, ow * c), (d_step, 1))[:] = r.reshape(oh, ow * c)
    tsrc = torch.from_numpy(src).to(cuda_device)
    tdst = torch.full((len(want),), 7, dtype=torch.uint8, device=cuda_device)
    assert tsrc.data_ptr() % 4 == 0 and tdst.data_ptr() % 4 == 0
    ang = np.array(rc.VIEW_ANGLES, np.float64)
    L = _capi.lib()
    _capi.check(L.prl_hip_rotate_batch_device(n, c, ang.ctypes.data, tsrc.data_ptr() + src_off, s_page, s_step, w, h,
                                              tdst.data_ptr() + dst_off, d_page, d_step, torch.cuda.current_stream().cuda_stream))
    got = tdst.cpu().numpy()
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(tsrc.cpu().numpy(), src)
    assert int((want != 7).sum()) > n * h * w * c // 2


def test_host_entry_with_two_channels(prl, oracle, cuda_device):
    from prlib_amd import _capi

    L = _capi.lib()
    for p, a in rc.host_cases():
        h, w, c = p.shape
        want = oracle.rotate(p, a)
        out = np.full(want.shape, 7, np.uint8)
        _capi.check(L.prl_hip_rotate_host(c, a, p.ctypes.data, p.strides[0], w, h, out.ctypes.data, out.strides[0]))
        assert np.array_equal(out, want), (a, int((out != want).sum()))


def test_argument_errors_of_the_batch_entry(prl, cuda_device):
    import torch

    from prlib_amd import _capi

    L = _capi.lib()
    w, h = 40, 24
    s = torch.zeros((h, w * 4), dtype=torch.uint8, device=cuda_device)
    d = torch.zeros((w, w * 4), dtype=torch.uint8, device=cuda_device)
    ang = np.array([3.0], np.float64)
    quarter = np.array([90.0], np.float64)
    sp, dp, ap = s.data_ptr(), d.data_ptr(), ang.ctypes.data

    def call(channels=1, angles=ap, src=sp, dst=dp, width=w, height=h, src_step=w * 4, dst_step=w * 4):
        return L.prl_hip_rotate_batch_device(1, channels, angles, src, h * w * 4, src_step, width, height, dst, w * w * 4, dst_step, None)

    assert call() == _capi.PRL_OK
    assert call(channels=0) == _capi.PRL_ERR_BAD_CHANNELS
    assert call(channels=5, src_step=w * 5, dst_step=w * 5) == _capi.PRL_ERR_BAD_CHANNELS
    assert call(angles=None) == _capi.PRL_ERR_BAD_ARG
    assert call(dst=sp) == _capi.PRL_ERR_BAD_ARG
    # the destination's rows are compared with the page's own result width: 40 for the general angle, 24 for the quarter turn
    assert call(dst_step=w - 1) == _capi.PRL_ERR_BAD_ARG
    assert call(angles=quarter.ctypes.data, dst_step=h) == _capi.PRL_OK
    assert call(angles=quarter.ctypes.data, dst_step=h - 1) == _capi.PRL_ERR_BAD_ARG
    assert call(width=0) == _capi.PRL_ERR_EMPTY
    assert call(width=32768, src_step=32768, dst_step=32768) == _capi.PRL_ERR_BAD_ARG
    assert call(height=32768, dst_step=32768) == _capi.PRL_ERR_BAD_ARG
    ow, oh = C.c_int(0), C.c_int(0)
    assert L.prl_hip_rotate_out_size(w, h, 3.0, None, C.byref(oh)) == _capi.PRL_ERR_BAD_ARG
    assert L.prl_hip_rotate_out_size(w, h, 3.0, C.byref(ow), None) == _capi.PRL_ERR_BAD_ARG
    assert L.prl_hip_rotate_out_size(w, h, 3.0, C.byref(ow), C.byref(oh)) == _capi.PRL_OK and (ow.value, oh.value) == (w, w)
    torch.cuda.synchronize()
