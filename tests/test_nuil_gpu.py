"""prl::correctNUIL and the flat-element morphology (gmorph.hip) on the MI355X: every operator, shape and size class, layouts,
in-place calls, the by-the-definition kernel against the span kernel, the reference's scans, a user-sized batch, the C++
drop-in and the torch path on its own stream - every byte against the restatement of tests/nuil_ref.py."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

import nuil_ref as nr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (15, 15), (16, 16), (31, 31), (32, 32), (63, 63), (101, 101), (255, 255), (7, 3),
         (4, 9), (70, 1), (1, 49)]


def _inputs(h, w, c, seed):
    """uniform random; synth pages with 5 % and 20 % impulses; all 0; all 255; one-pixel stripes (test_median_gpu's families)"""
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


def _fold(pages):
    """N x H x W x C -> H x W x (N C): channels are independent, so a batch is one page with more of them"""
    n, h, w, c = pages.shape
    return np.ascontiguousarray(pages.transpose(1, 2, 0, 3).reshape(h, w, n * c))


def _unfold(a, n, c):
    h, w = a.shape[:2]
    return np.ascontiguousarray(a.reshape(h, w, n, c).transpose(2, 0, 1, 3))


def _want_all_ops(pages, shape, kw, kh):
    """the six operators' results for a batch, from four passes of the restatement"""
    n, _, _, c = pages.shape
    a = _fold(pages)
    e, d = nr.erode(a, shape, kw, kh), nr.dilate(a, shape, kw, kh)
    o, cl = nr.dilate(e, shape, kw, kh), nr.erode(d, shape, kw, kh)
    res = {nr.ERODE: e, nr.DILATE: d, nr.OPEN: o, nr.CLOSE: cl, nr.TOPHAT: nr._sat_sub(a, o), nr.BLACKHAT: nr._sat_sub(cl, a)}
    return {k: _unfold(v, n, c) for k, v in res.items()}


def _want_nuil(pages, size):
    n, _, _, c = pages.shape
    return _unfold(nr.correct_nuil(_fold(pages), size), n, c)


def _mismatch(got, want):
    bad = np.argwhere(got != want)
    return int(bad.shape[0]), bad[:5].tolist()


def _dev(fn, pages, *args, **kw):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(pages)).cuda()
    r = fn(t, *args, **kw)
    torch.cuda.synchronize()
    return r.cpu().numpy()


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_morphology_grid(prl, cuda_device, c):
    pages = _inputs(37, 53, c, 3 + c)
    for shape in nr.SHAPES:
        for kw, kh in SIZES:
            want = _want_all_ops(pages, shape, kw, kh)
            for op in nr.OPS:
                n_bad, where = _mismatch(_dev(prl.morphologyEx, pages, op, shape, (kw, kh)), want[op])
                print(f"c={c} shape={shape} k={kw}x{kh} op={op}: {n_bad} mismatching bytes")
                assert n_bad == 0, (c, shape, kw, kh, op, where)


def _nuil_pages(h, w, c, seed):
    """the input families, and darker copies of them so that some channels of some pages are inverted"""
    pages = _inputs(h, w, c, seed)
    dark = (pages // 3).astype(np.uint8)
    mixed = pages.copy()
    mixed[..., 0] = dark[..., 0]
    return np.concatenate([pages, dark, mixed])


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_correct_nuil_sizes(prl, cuda_device, c):
    pages = _nuil_pages(45, 61, c, 20 + c)
    flags = [nr.channel_inverted(p) for p in pages]
    assert any(any(f) for f in flags) and any(not all(f) for f in flags)
    for size in (1, 2, 3, 15, 31, 51, 101):
        n_bad, where = _mismatch(_dev(prl.correctNUIL, pages, size), _want_nuil(pages, size))
        print(f"correctNUIL c={c} size={size}: {n_bad} mismatching bytes")
        assert n_bad == 0, (c, size, where)
    assert np.array_equal(_dev(prl.correctNUIL, pages), _want_nuil(pages, 31))   # the header default


def test_mean_threshold_on_the_device(prl, cuda_device):
    at = np.full((4, 8), 128, np.uint8)
    at[0, 0], at[0, 1] = 100, 156
    below = at.copy()
    below[3, 7] = 127
    two = np.dstack([at, below, at, below])
    for img in (at, below, two):
        assert np.array_equal(prl.correctNUIL(img, 3), nr.correct_nuil(img, 3))
        assert np.array_equal(_dev(prl.correctNUIL, img, 3), nr.correct_nuil(img, 3))
    for v in (0, 127, 128, 255):
        assert (_dev(prl.correctNUIL, np.full((40, 50, 3), v, np.uint8), 31) == 255).all()


def test_pages_smaller_than_the_element(prl, cuda_device):
    rng = np.random.default_rng(12)
    for shape_ in ((5, 40), (40, 5), (1, 1), (3, 200), (2, 3)):
        for c in (1, 3):
            pages = rng.integers(0, 256, size=(3,) + shape_ + (c,), dtype=np.uint8)
            pages[1] //= 4
            for size in (31, 63, 255):
                assert np.array_equal(_dev(prl.correctNUIL, pages, size), _want_nuil(pages, size)), (shape_, c, size)
            want = _want_all_ops(pages, nr.ELLIPSE, 31, 63)
            for op in nr.OPS:
                assert np.array_equal(_dev(prl.morphologyEx, pages, op, nr.ELLIPSE, (31, 63)), want[op]), (shape_, c, op)


def test_layouts_and_in_place(prl, cuda_device):
    import torch

    h, w, c = 41, 29, 3
    pages = _nuil_pages(h, w, c, 17)
    n = pages.shape[0]
    cases = [("nuil", 31), ("nuil", 5)] + [("morph", op, shape, k) for op, shape, k in (
        (nr.ERODE, nr.ELLIPSE, (9, 9)), (nr.DILATE, nr.RECT, (5, 7)), (nr.DILATE, nr.RECT, (1, 6)), (nr.OPEN, nr.CROSS, (4, 5)),
        (nr.CLOSE, nr.RECT, (6, 3)), (nr.TOPHAT, nr.ELLIPSE, (15, 15)), (nr.BLACKHAT, nr.RECT, (8, 8)), (nr.ERODE, nr.RECT, (1, 1)))]
    for case in cases:
        if case[0] == "nuil":
            fn = lambda t, out=None: prl.correctNUIL(t, case[1], out=out)                         # noqa: E731
            want = _want_nuil(pages, case[1])
        else:
            fn = lambda t, out=None: prl.morphologyEx(t, case[1], case[2], case[3], out=out)      # noqa: E731
            want = _want_all_ops(pages, case[2], *case[3])[case[1]]
        # source rows of 97 bytes, pages 50 rows apart; destination rows of 101 bytes, pages of 45 rows: nothing a multiple of 4
        sb = torch.full((n, 50, 97), 7, dtype=torch.uint8, device="cuda")
        sv = sb[:, :h, :w * c].unflatten(2, (w, c))
        sv.copy_(torch.from_numpy(pages))
        db = torch.full((n, 45, 101), 201, dtype=torch.uint8, device="cuda")
        dv = db[:, :h, :w * c].unflatten(2, (w, c))
        fn(sv, out=dv)
        torch.cuda.synchronize()
        assert np.array_equal(dv.cpu().numpy(), want), case
        d = db.cpu().numpy()
        assert (d[:, h:] == 201).all() and (d[:, :, w * c:] == 201).all(), "padding bytes of the destination written"
        s = sb.cpu().numpy()
        assert np.array_equal(s[:, :h, :w * c].reshape(n, h, w, c), pages) and (s[:, h:] == 7).all() and (s[:, :, w * c:] == 7).all()
        # exact aliasing dst == src, dense and strided
        ip = torch.from_numpy(pages).cuda()
        fn(ip, out=ip)
        torch.cuda.synchronize()
        assert np.array_equal(ip.cpu().numpy(), want), ("in place", case)
        fn(sv, out=sv)
        torch.cuda.synchronize()
        assert np.array_equal(sv.cpu().numpy(), want), ("in place, strided", case)
        assert (sb.cpu().numpy()[:, h:] == 7).all()
        # a batch of different pages equals one call per page
        for i in (0, n - 1):
            assert np.array_equal(_dev(fn, pages[i]), want[i])


def test_host_entry_numpy(prl, cuda_device):
    rng = np.random.default_rng(8)
    for shape_ in ((19, 23), (19, 23, 1), (19, 23, 3), (19, 23, 4), (1, 1), (3, 200, 2)):
        img = (rng.integers(0, 256, size=shape_, dtype=np.uint8) // (1 + len(shape_) % 2)).astype(np.uint8)
        for size in (1, 4, 31):
            got = prl.correctNUIL(img, size)
            assert got.shape == img.shape and np.array_equal(got, nr.correct_nuil(img, size)), (shape_, size)
        got = prl.morphologyEx(img, nr.TOPHAT, nr.ELLIPSE, (5, 8))
        assert np.array_equal(got, nr.morphology_ex(img, nr.TOPHAT, nr.ELLIPSE, 5, 8))
    view = rng.integers(0, 256, size=(30, 40, 3), dtype=np.uint8)[2:25, 3:31]   # strided rows
    assert np.array_equal(prl.correctNUIL(view, 7), nr.correct_nuil(np.ascontiguousarray(view), 7))


def test_span_kernel_equals_the_definition_kernel(prl, cuda_device, tmp_path):
    """The by-the-definition kernel (hooks build, PRL_HIP_GMORPH_LITERAL=1) in a child process; the product library here."""
    code = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from prlib_amd import _capi
_capi.use_library(_capi.HOOKS_LIB_PATH)
import torch, prlib_amd
z = np.load(sys.argv[2])
out = {}
for key in z.files:
    t = torch.from_numpy(z[key]).cuda()
    for size in (5, 31, 32):
        out[f"nuil_{key}_{size}"] = prlib_amd.correctNUIL(t, size).cpu().numpy()
    for op in (0, 1, 2, 3, 5, 6):
        for shape, k in ((0, (31, 31)), (1, (6, 9)), (2, (16, 31)), (0, (40, 1))):
            out[f"m_{key}_{op}_{shape}_{k[0]}_{k[1]}"] = prlib_amd.morphologyEx(t, op, shape, k).cpu().numpy()
np.savez(sys.argv[3], **out)
print("literal ok")
'''
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    pages = {f"c{c}": _nuil_pages(70, 90, c, 40 + c)[::3] for c in (1, 3, 4)}
    np.savez(src, **pages)
    env = dict(os.environ, PRL_HIP_GMORPH_LITERAL="1")
    r = subprocess.run([sys.executable, "-c", code, ROOT, src, dst], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "literal ok" in r.stdout, r.stdout + r.stderr[-3000:]
    lit = np.load(dst)
    for key, p in pages.items():
        for size in (5, 31, 32):
            fast = _dev(prl.correctNUIL, p, size)
            assert np.array_equal(fast, lit[f"nuil_{key}_{size}"]), ("nuil", key, size)
            assert np.array_equal(fast, _want_nuil(p, size)), ("nuil vs restatement", key, size)
        for shape, k in ((0, (31, 31)), (1, (6, 9)), (2, (16, 31)), (0, (40, 1))):
            want = _want_all_ops(p, shape, *k)
            for op in nr.OPS:
                fast = _dev(prl.morphologyEx, p, op, shape, k)
                assert np.array_equal(fast, lit[f"m_{key}_{op}_{shape}_{k[0]}_{k[1]}"]), (key, op, shape, k)
                assert np.array_equal(fast, want[op]), ("vs restatement", key, op, shape, k)


COLOUR = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "stages", "*.npz")))
GRAY = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "scans", "*.npz")))


@pytest.mark.parametrize("path", COLOUR, ids=[os.path.basename(p)[:-4] for p in COLOUR])
def test_reference_colour_scans(prl, cuda_device, path):
    img = np.load(path)["bgr"]
    want = nr.correct_nuil(img, 31)
    n_bad, where = _mismatch(prl.correctNUIL(img), want)
    print(f"{os.path.basename(path)}: {n_bad} mismatching bytes of {want.size}")
    assert n_bad == 0, where
    assert np.array_equal(_dev(prl.correctNUIL, img, 31), want)


@pytest.mark.parametrize("path", GRAY, ids=[os.path.basename(p)[:-4] for p in GRAY])
def test_reference_gray_scans(prl, cuda_device, path):
    img = np.load(path)["gray"]
    want = nr.correct_nuil(img, 31)
    for src in (img, 255 - img):   # a scan and its negative: the same answer
        n_bad, where = _mismatch(_dev(prl.correctNUIL, src, 31), want)
        print(f"{os.path.basename(path)}: {n_bad} mismatching bytes of {want.size}")
        assert n_bad == 0, where


def test_sizes_users_run(prl, cuda_device):
    import torch

    from prlib_amd import synth

    rng = np.random.default_rng(21)
    n = 64
    pages = np.empty((n, 3508, 2480), np.uint8)
    for i in range(n):
        base = synth.page_numpy(3508, 2480, index=i % 7)
        shade = np.linspace(1.0, 0.45 + 0.5 * rng.random(), 2480)[None, :]     # a shadow across the page
        pages[i] = (base * shade).astype(np.uint8)
        if i % 5 == 4:
            pages[i] = 255 - pages[i]
    t = torch.from_numpy(pages).cuda()
    got = prl.correctNUIL(t, 31)
    torch.cuda.synchronize()
    g = got.cpu().numpy()
    for i in (0, 4, 33, 63):
        for y0, y1 in ((0, 48), (1730, 1770), (3460, 3508)):
            n_bad, where = _mismatch(g[i, y0:y1], nr.correct_nuil_rows(pages[i], 31, y0, y1))
            print(f"A4 page {i} rows {y0}-{y1}: {n_bad} mismatching bytes")
            assert n_bad == 0, (i, y0, where)
    for i in (1, 4, 62):   # the batch equals one call per page
        assert np.array_equal(g[i], prl.correctNUIL(t[i], 31).cpu().numpy()), i


def test_torch_path_on_a_side_stream(prl, cuda_device):
    import torch

    pages = _nuil_pages(64, 96, 1, 30)[..., 0]
    t = torch.from_numpy(pages).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out = prl.correctNUIL(t, 31)
        out2 = prl.morphologyEx(t, nr.CLOSE, nr.RECT, (9, 5))
        out3 = prl.correctNUIL(out2, 15)
    s.synchronize()
    p4 = pages[..., None]
    assert np.array_equal(out.cpu().numpy(), _want_nuil(p4, 31)[..., 0])
    closed = _want_all_ops(p4, nr.RECT, 9, 5)[nr.CLOSE]
    assert np.array_equal(out2.cpu().numpy(), closed[..., 0])
    assert np.array_equal(out3.cpu().numpy(), _want_nuil(closed, 15)[..., 0])


def test_cpp_dropin_on_device(prl, cuda_device, tmp_path):
    from test_nuil_cpu import build_dropin

    exe = build_dropin(str(tmp_path))
    photo = np.load(os.path.join(ROOT, "tests", "golden", "stages", "denoise_butterfly_sp.npz"))["bgr"]
    gray = np.ascontiguousarray(np.load(COLOUR[0])["bgr"][:400, :300, 1])
    for name, img, size, roi in (("bgr", photo, 0, False), ("gray", gray, 15, True), ("dark", (photo // 3).astype(np.uint8), 31, True)):
        src = tmp_path / f"{name}.raw"
        dst = tmp_path / f"{name}.out"
        src.write_bytes(np.ascontiguousarray(img).tobytes())
        h, w = img.shape[:2]
        c = img.shape[2] if img.ndim == 3 else 1
        r = subprocess.run([exe, "run", str(size), str(h), str(w), str(c), str(src), str(dst)] + (["roi"] if roi else []),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "nuil dropin run: OK" in r.stdout, r.stdout + r.stderr
        view = np.ascontiguousarray(img[2:h - 3, 3:w - 4] if roi else img)
        got = np.frombuffer(dst.read_bytes(), np.uint8).reshape(view.shape)
        assert np.array_equal(got, nr.correct_nuil(view, size or 31)), name
