"""prl::denoiseSaltPepper on the MI355X: every path (k = 3 / 5 networks, the histogram kernel, 16- and 32-bit counters),
layouts, the reference's photographs, user-sized batches, the C++ drop-in and the torch path on its own stream, all
against the restatement of tests/median_ref.py."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

import median_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(h, w, c, seed):
    """uniform random; synth pages with 5 % and 20 % impulses; all 0; all 255; one-pixel stripes"""
    from prlib_amd import synth

    rng = np.random.default_rng(seed)
    pages = [rng.integers(0, 256, size=(h, w, c), dtype=np.uint8)]
    base = synth.page_numpy(h, w, index=seed % 11)
    for frac in (0.05, 0.20):
        p = np.repeat(base[:, :, None], c, axis=2).copy()
        m = rng.random((h, w, c)) < frac
        p[m] = np.where(rng.random(int(m.sum())) < 0.5, 0, 255).astype(np.uint8)
        pages.append(p)
    pages.append(np.zeros((h, w, c), np.uint8))
    pages.append(np.full((h, w, c), 255, np.uint8))
    yy, xx = np.mgrid[0:h, 0:w]
    pages.append(np.repeat((((yy + xx) % 2) * 255).astype(np.uint8)[:, :, None], c, axis=2))
    return np.stack(pages)


def _dev(prl, pages, k, times, out=None):
    import torch

    t = torch.from_numpy(pages).cuda()
    r = prl.denoiseSaltPepper(t, k, times, out=out)
    torch.cuda.synchronize()
    return r.cpu().numpy()


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_parity_grid(prl, cuda_device, c):
    h, w = 37, 53
    big = 2 * max(h, w) + 1
    pages = _inputs(h, w, c, 3 + c)
    for k in (1, 3, 5, 7, 9, 15, 31, big):
        if c == 2 and k >= 7:
            continue
        want = [pages]
        for _ in range(3):
            want.append(np.stack([median_ref.denoise_salt_pepper(p, k, 1) for p in want[-1]]))
        for times in (0, 1, 2, 3):
            got = _dev(prl, pages, k, times)
            bad = np.argwhere(got != want[times])
            assert bad.size == 0, (k, c, times, bad[:5].tolist())


def test_generic_kernel_beyond_16_bit_counters(prl, cuda_device):
    rng = np.random.default_rng(5)
    page = rng.integers(0, 256, size=(300, 280), dtype=np.uint8)
    page[::7] = 255
    for k in (257, 601):
        got = _dev(prl, page, k, 1)
        assert np.array_equal(got, median_ref.denoise_salt_pepper(page, k, 1)), k


def test_layouts(prl, cuda_device):
    import torch

    h, w, c = 41, 29, 3
    pages = _inputs(h, w, c, 17)
    n = pages.shape[0]
    for k in (3, 5, 7):
        # source rows of 97 bytes (odd: the unaligned variant), pages 50 rows apart; destination rows of 100, pages of 45 rows
        sb = torch.full((n, 50, 97), 7, dtype=torch.uint8, device="cuda")
        sv = sb[:, :h, :w * c].unflatten(2, (w, c))
        sv.copy_(torch.from_numpy(pages))
        db = torch.full((n, 45, 100), 201, dtype=torch.uint8, device="cuda")
        dv = db[:, :h, :w * c].unflatten(2, (w, c))
        for times in (1, 2):
            prl.denoiseSaltPepper(sv, k, times, out=dv)
            torch.cuda.synchronize()
            want = np.stack([median_ref.denoise_salt_pepper(p, k, times) for p in pages])
            assert np.array_equal(dv.cpu().numpy(), want), (k, times)
            d = db.cpu().numpy()
            assert (d[:, h:] == 201).all() and (d[:, :, w * c:] == 201).all(), "padding bytes of the destination written"
            s = sb.cpu().numpy()
            assert np.array_equal(s[:, :h, :w * c].reshape(n, h, w, c), pages) and (s[:, h:] == 7).all() and (s[:, :, w * c:] == 7).all()
            # in place
            ip = torch.from_numpy(pages).cuda()
            prl.denoiseSaltPepper(ip, k, times, out=ip)
            torch.cuda.synchronize()
            assert np.array_equal(ip.cpu().numpy(), want), ("in place", k, times)
        # a batch of different pages equals one call per page
        batch = _dev(prl, pages, k, 2)
        for i in range(n):
            assert np.array_equal(batch[i], _dev(prl, pages[i], k, 2))


def test_host_entry_numpy(prl, cuda_device):
    rng = np.random.default_rng(8)
    for shape in ((19, 23), (19, 23, 1), (19, 23, 3), (19, 23, 4), (1, 1), (3, 200, 2)):
        img = rng.integers(0, 256, size=shape, dtype=np.uint8)
        for k, times in ((3, 1), (5, 2), (9, 1), (1, 1), (3, 0)):
            if len(shape) == 3 and shape[2] == 2 and k >= 7:
                continue
            got = prl.denoiseSaltPepper(img, k, times)
            assert got.shape == img.shape and np.array_equal(got, median_ref.denoise_salt_pepper(img, k, times)), (shape, k, times)
    view = rng.integers(0, 256, size=(30, 40, 3), dtype=np.uint8)[2:25, 3:31]   # strided rows
    assert np.array_equal(prl.denoiseSaltPepper(view, 3, 1), median_ref.denoise_salt_pepper(view, 3, 1))


PHOTOS = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "stages", "denoise_*.npz")))


@pytest.mark.parametrize("path", PHOTOS, ids=[os.path.basename(p)[8:-4] for p in PHOTOS])
def test_reference_photographs(prl, cuda_device, path):
    img = np.load(path)["bgr"]
    for k, times in ((3, 1), (5, 2), (7, 1)):
        got = prl.denoiseSaltPepper(img, k, times)
        assert np.array_equal(got, median_ref.denoise_salt_pepper(img, k, times)), (k, times)
        assert np.array_equal(_dev(prl, img, k, times), got)


def test_sizes_users_run(prl, cuda_device):
    import torch

    from prlib_amd import synth

    rng = np.random.default_rng(21)
    base = synth.page_numpy(3508, 2480, index=3)
    pages = np.stack([base] * 16)
    for i in range(16):
        m = rng.random(base.shape) < 0.05
        pages[i][m] = rng.integers(0, 2, size=int(m.sum()), dtype=np.uint8) * 255
    got = _dev(prl, pages, 3, 1)
    for i in (0, 9, 15):
        assert np.array_equal(got[i], median_ref.denoise_salt_pepper(pages[i], 3, 1)), i
    for i in range(16):
        assert np.array_equal(got[i], _dev(prl, pages[i], 3, 1)), i
    del pages, got
    big = rng.integers(0, 256, size=(4, 4096, 4096, 3), dtype=np.uint8)
    t = torch.from_numpy(big).cuda()
    got = prl.denoiseSaltPepper(t, 5, 2)
    torch.cuda.synchronize()
    g = got.cpu().numpy()
    for i in range(4):
        assert np.array_equal(g[i], prl.denoiseSaltPepper(t[i], 5, 2).cpu().numpy()), i
    for y0, y1 in ((0, 64), (2000, 2064), (4032, 4096)):
        assert np.array_equal(g[2, y0:y1], median_ref.denoise_salt_pepper_rows(big[2], 5, 2, y0, y1)), (y0, y1)


def test_torch_path_on_a_side_stream(prl, cuda_device):
    import torch

    pages = _inputs(64, 96, 1, 30)[..., 0]
    t = torch.from_numpy(pages).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out = prl.denoiseSaltPepper(t, 5, 3)
        out2 = prl.denoiseSaltPepper(t, 9, 1)
    s.synchronize()
    assert np.array_equal(out.cpu().numpy(), np.stack([median_ref.denoise_salt_pepper(p, 5, 3) for p in pages]))
    assert np.array_equal(out2.cpu().numpy(), np.stack([median_ref.denoise_salt_pepper(p, 9, 1) for p in pages]))


def test_cpp_dropin_on_device(prl, cuda_device, tmp_path):
    from test_median_cpu import build_dropin

    exe = build_dropin(str(tmp_path))
    photo = np.load(os.path.join(ROOT, "tests", "golden", "stages", "denoise_butterfly_sp.npz"))["bgr"]
    gray = np.ascontiguousarray(np.load(PHOTOS[0])["bgr"][:, :, 1])
    for name, img, roi in (("bgr", photo, False), ("gray", gray, True)):
        src = tmp_path / f"{name}.raw"
        dst = tmp_path / f"{name}.out"
        src.write_bytes(np.ascontiguousarray(img).tobytes())
        h, w = img.shape[:2]
        c = img.shape[2] if img.ndim == 3 else 1
        r = subprocess.run([exe, "run", "3", "1", str(h), str(w), str(c), str(src), str(dst)] + (["roi"] if roi else []),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "median dropin run: OK" in r.stdout, r.stdout + r.stderr
        view = img[2:h - 3, 3:w - 4] if roi else img
        got = np.frombuffer(dst.read_bytes(), np.uint8).reshape(view.shape)
        assert np.array_equal(got, median_ref.denoise_salt_pepper(np.ascontiguousarray(view), 3, 1)), name


def test_forced_generic_kernel_at_small_windows(prl, cuda_device):
    """The histogram kernel (hooks build, PRL_HIP_MEDIAN_GENERIC=1) gives the k = 3 / 5 networks' answers."""
    code = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from prlib_amd import _capi
_capi.use_library(_capi.HOOKS_LIB_PATH)
import torch, prlib_amd, median_ref
rng = np.random.default_rng(4)
for c in (1, 2, 3, 4):
    pages = rng.integers(0, 256, size=(3, 45, 38, c), dtype=np.uint8)
    for k in (3, 5):
        got = prlib_amd.denoiseSaltPepper(torch.from_numpy(pages).cuda(), k, 2).cpu().numpy()
        want = np.stack([median_ref.denoise_salt_pepper(p, k, 2) for p in pages])
        assert np.array_equal(got, want), (c, k)
print("generic ok")
'''
    env = dict(os.environ, PRL_HIP_MEDIAN_GENERIC="1")
    r = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "generic ok" in r.stdout, r.stdout + r.stderr[-3000:]
