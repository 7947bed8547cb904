"""The focus sums and measures on the device (focus.hip) against tests/focus_ref.py: int64 equality for the sums, bit equality for
the measures (NaN equal to NaN), every pixel of every case.  Sizes sit at the edges of k_focus's geometry, named from its
constants: a lane's 4 pixels, a tile's 256 columns and 64 rows, a workgroup's 4 tiles."""
import os
import subprocess
import sys

import numpy as np
import pytest

import focus_ref as fr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_REF = {}


def ref_sums(key, page, ks):
    """focus_ref.sums, computed once per page and Sobel size"""
    if (key, ks) not in _REF:
        _REF[key, ks] = fr.sums(page, ks)
    return _REF[key, ks]


def check(prl, torch, dev, page, ks=3, key=None):
    """one page H x W [x C] through focusSums"""
    t = torch.from_numpy(page).to(dev)
    got = prl.focusSums(t, ks).cpu().numpy()
    want = fr.sums(page, ks) if key is None else ref_sums(key, page, ks)
    assert got.dtype == np.int64 and got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want), (page.shape, ks, got.tolist(), want.tolist())


def test_every_small_side(prl, cuda_device):
    import torch

    for h in (1, 2, 3, 5):
        for w in (1, 2, 3, 5):
            for c in (1, 3, 4):
                for ks in (1, 3):
                    check(prl, torch, cuda_device, fr.noise(h, w, c, 1), ks)
            check(prl, torch, cuda_device, fr.extremes(h, w, 2))


@pytest.mark.parametrize("width", [63, 64, 65, fr.STRIP_PX - 1, fr.STRIP_PX, fr.STRIP_PX + 1, 1021] + [fr.LANE_PX * k + d for k in (2, 3) for d in (-1, 0, 1)])
def test_widths(prl, cuda_device, width):
    """around a wavefront's 64 pixels, a tile's STRIP_PX columns, 1021 = 3 strips and a ragged last group of 4, and around the
    8 and 12 pixels below which a row has no lane on the dword path"""
    import torch

    for h in (3, fr.TILE_ROWS + 2):
        check(prl, torch, cuda_device, fr.noise(h, width, 1, 3), 3)
        check(prl, torch, cuda_device, fr.extremes(h, width, 4), 1)
    for c in (3, 4):
        check(prl, torch, cuda_device, fr.noise(7, width, c, 5), 3)


# the rows of a tile; a workgroup's TILES_PER_GROUP tiles stacked on a page of one strip; two strips: the workgroup's tiles are
# two rows of tiles, and the last workgroup has tiles beyond the page
ROW_EDGES = sorted({e + d for e in (fr.TILE_ROWS, 2 * fr.TILE_ROWS, fr.TILES_PER_GROUP * fr.TILE_ROWS) for d in (-1, 0, 1)})


@pytest.mark.parametrize("height", ROW_EDGES)
def test_heights(prl, cuda_device, height):
    import torch

    for w in (37, fr.STRIP_PX + 44, 2 * fr.STRIP_PX + fr.LANE_PX + 1):   # 1, 2 and 3 strips
        check(prl, torch, cuda_device, fr.noise(height, w, 1, 6), 3)
    check(prl, torch, cuda_device, fr.noise(height, fr.STRIP_PX + 44, 3, 7), 1)
    check(prl, torch, cuda_device, fr.noise(height, 37, 4, 8), 3)


@pytest.mark.parametrize("channels", (1, 3, 4))
def test_layouts_and_a_batch_of_five(prl, cuda_device, channels):
    """pitched rows, a source at an odd address, a page stride that is no multiple of 4; five different pages whose sums must not
    mix; `out`; the source unchanged"""
    import torch

    n, h, w, c = 5, 70, 261, channels
    step = w * c + 5 + ((w * c + 5) % 4 == 0)
    page_stride, offset = h * step + 3 + ((h * step + 3) % 4 == 0), 1
    assert page_stride % 4 != 0 and step % 4 != 0
    rng = np.random.default_rng(12)
    buf = rng.integers(0, 256, size=offset + n * page_stride + 16, dtype=np.uint8)
    dbuf = torch.from_numpy(buf).to(cuda_device)
    shape, strides = ((n, h, w, c), (page_stride, step, c, 1)) if c > 1 else ((n, h, w), (page_stride, step, 1))
    pages = torch.as_strided(dbuf, shape, strides, storage_offset=offset)
    assert pages.data_ptr() % 2 == 1
    host = np.lib.stride_tricks.as_strided(buf[offset:], shape, strides)
    for i in range(n):   # different pages: page i is darker by 20 i
        host[i] //= (i + 1)
    dbuf.copy_(torch.from_numpy(buf))
    before = dbuf.clone()
    want = np.stack([fr.sums(np.ascontiguousarray(host[i])) for i in range(n)])
    assert len({w_.tobytes() for w_ in want}) == n
    got = prl.focusSums(pages)
    assert tuple(got.shape) == ((n, c, 6) if c > 1 else (n, 6)) and got.dtype == torch.int64 and got.is_contiguous()
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(dbuf, before), "the source was written"
    out = torch.full_like(got, -1)
    assert prl.focusSums(pages, 3, out=out) is out and np.array_equal(out.cpu().numpy(), want)
    for i in (0, 4):   # a page alone, at its own odd address
        assert np.array_equal(prl.focusSums(pages[i]).cpu().numpy(), want[i])
    want1 = np.stack([fr.sums(np.ascontiguousarray(host[i]), 1) for i in range(n)])
    assert np.array_equal(prl.focusSums(pages, 1).cpu().numpy(), want1)
    with pytest.raises(TypeError):
        prl.focusSums(pages, out=torch.zeros(got.shape, dtype=torch.int32, device=cuda_device))


def test_worst_case_magnitudes(prl, cuda_device):
    """1024 x 1024: the largest S_TENG, S_LAP2 and S_LAPM4 a page of that size can have, and a flat 255 page, in one batch"""
    import torch

    h = w = 1024
    pages = np.stack([fr.stripes4(h, w), fr.checkerboard(h, w), fr.stripes2(h, w), fr.flat(h, w, 255)])
    t = torch.from_numpy(pages).to(cuda_device)
    for ks in (3, 1):
        want = np.stack([ref_sums(("worst", i), pages[i], ks) for i in range(4)])
        assert np.array_equal(prl.focusSums(t, ks).cpu().numpy(), want), ks
    want = np.stack([ref_sums(("worst", i), pages[i], 3) for i in range(4)])
    assert want[0, fr.SUM_TENG] >= (h - 2) * (w - 2) * 1020 ** 2 and want[1, fr.SUM_LAP2] == h * w * fr.MAX_L ** 2
    assert want[2, fr.SUM_LAPM4] == h * w * fr.MAX_XY and want[3].tolist() == [255 * h * w, 65025 * h * w, 0, 0, 0, 0]
    m = prl.focusMeasures(t)
    assert fr.same_bits(m, fr.from_sums(want, w, h)) and m[3].tolist() == [0.0, 0.0, 0.0, 0.0]


@pytest.mark.parametrize("shape", [(64, fr.MAX_SIDE), (fr.MAX_SIDE, 64)], ids=lambda s: "%dx%d" % s)
def test_longest_sides(prl, cuda_device, shape):
    import torch

    page = fr.noise(shape[0], shape[1], 1, 9)
    for ks in (1, 3):
        check(prl, torch, cuda_device, page, ks, key=("long", shape))


def test_reference_scan(prl, cuda_device):
    import torch

    gray = np.load(os.path.join(ROOT, "tests", "golden", "scans", "0010.npz"))["gray"]
    check(prl, torch, cuda_device, gray, 3, key="scan")
    check(prl, torch, cuda_device, gray, 1, key="scan")
    t = torch.from_numpy(gray).to(cuda_device)
    want = fr.from_sums(ref_sums("scan", gray, 3), gray.shape[1], gray.shape[0])
    assert fr.same_bits(prl.focusMeasures(t), want)
    assert fr.same_bits(prl.focusMeasures(gray), want)   # the host entry
    assert np.all(want > 0)


def test_measures_equal_the_reference_finalisation(prl, cuda_device):
    import ctypes

    import torch

    from prlib_amd import _capi

    L = _capi.lib()
    for c in (1, 3, 4):
        for h, w in ((1, 1), (5, 3), (67, 300)):
            page = fr.noise(h, w, c, 10)
            for ks in (1, 3):
                want_s = fr.sums(page, ks)
                want = fr.from_sums(want_s, w, h)
                assert fr.same_bits(prl.focusMeasures(page, ks), want), (c, h, w, ks)                         # numpy: the host entry
                assert fr.same_bits(prl.focusMeasures(torch.from_numpy(page).to(cuda_device), ks), want)     # torch: sums, then the host
                # the host entry's optional sums, on a pitched page
                buf = np.full((h, w * c + 3), 0x5A, np.uint8)
                buf[:, :w * c] = page.reshape(h, w * c)
                m, s = np.zeros((c, 4)), np.zeros((c, 6), np.int64)
                assert L.prl_hip_focus_measures_host(c, ks, buf.ctypes.data, buf.strides[0], w, h, m.ctypes.data, s.ctypes.data) == 0
                assert np.array_equal(s, want_s.reshape(c, 6)) and fr.same_bits(m, want.reshape(c, 4))
    batch = np.stack([fr.noise(40, 50, 3, 11), np.zeros((40, 50, 3), np.uint8), np.full((40, 50, 3), 255, np.uint8)])
    batch[1, :, :, 2] = fr.noise(40, 50, 1, 12)    # the all-zero page has one channel that is not
    got = prl.focusMeasures(torch.from_numpy(batch).to(cuda_device))
    assert got.shape == (3, 3, 4) and fr.same_bits(got, fr.from_sums(fr.batch_sums(batch), 50, 40))
    assert np.isnan(got[1, 0, fr.GLVN]) and np.isnan(got[1, 1, fr.GLVN]) and not np.isnan(got[1, 2]).any()
    assert got[2].tolist() == [[0.0] * 4] * 3
    assert np.isnan(prl.focusMeasures(np.zeros((9, 9), np.uint8))[fr.GLVN])
    zero = ctypes.c_void_p(0)
    assert L.prl_hip_focus_sums_batch_device(0, 1, 3, zero, 0, 0, 4, 4, zero, None) == _capi.PRL_ERR_BAD_ARG


def test_two_chunks(prl, cuda_device):
    """the hooks build: PRL_HIP_STAGE_CHUNK=2 runs five pages as 2, 2, 1, each chunk at its own offset into the pages and the sums"""
    code = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from prlib_amd import _capi
_capi.use_library(_capi.HOOKS_LIB_PATH)
import torch, prlib_amd as P, focus_ref as fr
for c, h, w in ((1, 130, 600), (3, 70, 261), (4, 5, 9), (1, 300, 37)):
    pages = np.stack([fr.noise(h, w, c, 20 + i) // (i + 1) for i in range(5)])
    for ks in (1, 3):
        got = P.focusSums(torch.from_numpy(pages).cuda(), ks).cpu().numpy()
        assert np.array_equal(got, fr.batch_sums(pages, ks)), (c, h, w, ks)
print("focus chunks ok")
'''
    env = dict(os.environ, PRL_HIP_STAGE_CHUNK="2")
    r = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "focus chunks ok" in r.stdout, r.stdout + r.stderr[-3000:]


def test_dropin_caller(prl, cuda_device, tmp_path):
    """tests/cpp/test_focus_dropin.cpp keeps `#include "blurDetection.h"`: prl::focusMeasures returns channel 0, also of a view"""
    import shutil

    from test_focus_cpu import build_dropin

    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    exe = build_dropin(str(tmp_path))
    for cn, ks, roi in ((1, 0, False), (3, 1, True), (4, 3, False)):
        rows, cols = 45, 83
        img = fr.noise(rows, cols, cn, 30).reshape(rows, cols, cn)
        path = os.path.join(str(tmp_path), "in.raw")
        img.tofile(path)
        r = subprocess.run([exe, "run", str(ks), str(rows), str(cols), str(cn), path] + (["roi"] if roi else []), capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0 and "focus dropin run: OK" in r.stdout, r.stdout + r.stderr
        view = np.ascontiguousarray(img[2:rows - 3, 3:cols - 4] if roi else img)
        got = np.array([int(v, 16) for v in r.stdout.split("\n")[0].split()], np.uint64).view(np.float64)
        assert fr.same_bits(got, fr.measures(view[:, :, 0], ks or 3)), (cn, ks, roi)
