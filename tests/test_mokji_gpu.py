"""prl::binarizeMokji (mokji.hip) on the MI355X: every bin of the co-occurrence primitive and every threshold and output byte of
the binarizer against the restatement of tests/mokji_ref.py - all page families at the sizes where the kernels can go wrong, the
parameter sets that reach the widest element, no pair and no interior, 1 / 3 / 4 channels, strided layouts, in place, two of the
reference's scans, the numpy host entry and the C++ drop-in.  No tolerance: equality on all pixels and all bins."""
import functools
import os
import subprocess

import numpy as np
import pytest

import mokji_ref as mr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE_IDS = [f"{w}x{h}" for w, h in mr.SIZES]
N_IDX, M_IDX = np.mgrid[0:256, 0:256]


def _mismatch(got, want):
    bad = np.argwhere(got != want)
    return int(bad.shape[0]), bad[:5].tolist()


@functools.lru_cache(maxsize=None)
def _pages(size):
    w, h = size
    return np.stack([p for _, p in mr.families(w, h, seed=3)])


@functools.lru_cache(maxsize=None)
def _matrices(size, e):
    """the Mokji matrix of every family page (it depends on E alone); computed once and shared"""
    return [mr.mokji_matrix(p, e) for p in _pages(size)]


def _want(size, e, m):
    ts = [mr.threshold_double(mat, m) for mat in _matrices(size, e)]
    return np.stack([mr.apply_threshold(p, t) for p, t in zip(_pages(size), ts)]), ts


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cooc(prl, a, b, border, md, **kw):
    import torch

    r = prl.cooccurrence(a, b, border, md, **kw)
    torch.cuda.synchronize()
    return r.cpu().numpy().view(np.uint32).astype(np.int64)


# ---- the co-occurrence primitive ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", mr.SIZES, ids=SIZE_IDS)
def test_cooccurrence_every_bin(prl, cuda_device, size):
    """all families of a size in one call, against planes that give b >= a (their dilation: flat and two-level pages take the
    wavefront-uniform shortcut, noise the scattered path) and planes that do not (the next family's page)"""
    import torch

    w, h = size
    a = _pages(size)
    n = a.shape[0]
    planes = {"dilated": np.stack([mr.dilate_shifts(p, 1) for p in a]), "rolled": np.roll(a, 1, axis=0)}
    ta = _cuda(a)
    out = torch.empty((n, 256, 256), dtype=torch.int32, device="cuda")
    for key, b in planes.items():
        tb = _cuda(b)
        below = 0
        for border in mr.BORDERS:
            full = [mr.cooccurrence(a[i], b[i], border, 0) for i in range(n)]
            below += sum(int(np.triu(f, 1).sum()) for f in full)
            area = max(0, w - 2 * border) * max(0, h - 2 * border)
            for md in mr.MIN_DIFFS:
                out.fill_(-559038737)   # garbage: the call overwrites it
                got = _cooc(prl, ta, tb, border, md, out=out)
                for i in range(n):
                    want = full[i] if md == 0 else np.where(N_IDX - M_IDX >= md, full[i], 0)
                    n_bad, where = _mismatch(got[i], want)
                    assert n_bad == 0, (size, key, border, md, i, where)
                    if md == 0:
                        assert int(got[i].sum()) == area, (size, key, border, i)
        assert (below > 0) == (key == "rolled")   # pairs with b < a were there to be counted, and only there
    one = _cooc(prl, ta[4], _cuda(planes["rolled"][4]), 1, 0)          # a single H x W page
    assert one.shape == (256, 256) and np.array_equal(one, mr.cooccurrence(a[4], planes["rolled"][4], 1, 0))


def test_cooccurrence_strided_pages(prl, cuda_device):
    """rows of W + 1 bytes, spare rows between pages; the padding stays as it was"""
    import torch

    w, h = 203, 117
    a = _pages((w, h))[3:8]
    b = np.roll(a, 2, axis=0)
    n = a.shape[0]
    bufs = []
    for src, fill in ((a, 7), (b, 9)):
        buf = torch.full((n, h + 3, w + 1), fill, dtype=torch.uint8, device="cuda")
        buf[:, :h, :w].copy_(torch.from_numpy(src))
        bufs.append(buf)
    got = _cooc(prl, bufs[0][:, :h, :w], bufs[1][:, :h, :w], 1, 1)
    for i in range(n):
        assert np.array_equal(got[i], mr.cooccurrence(a[i], b[i], 1, 1)), i
    for buf, src, fill in ((bufs[0], a, 7), (bufs[1], b, 9)):
        host = buf.cpu().numpy()
        assert np.array_equal(host[:, :h, :w], src) and (host[:, h:] == fill).all() and (host[:, :, w:] == fill).all()


# ---- thresholds and masks -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", mr.SIZES, ids=SIZE_IDS)
def test_thresholds_and_masks(prl, cuda_device, size):
    import torch

    w, h = size
    pages = _pages(size)
    t = _cuda(pages)
    for e, m in mr.params_of(size):
        want, ts = _want(size, e, m)
        thr = prl.mokjiThresholds(t, e, m)
        got = prl.binarizeMokji(t, e, m)
        torch.cuda.synchronize()
        print(f"{w}x{h} E = {e} M = {m}: thresholds {thr.cpu().tolist()}")
        assert thr.cpu().tolist() == ts, (size, e, m)
        n_bad, where = _mismatch(got.cpu().numpy(), want)
        assert n_bad == 0, (size, e, m, where)
        if (e, m) in ((3, 256), (2, 20)):
            assert set(ts) == {-1} and (want == 255).all()
    one = prl.binarizeMokji(t[7])                                        # a single H x W page, the defaults
    assert np.array_equal(one.cpu().numpy(), _want(size, 3, 20)[0][7])
    assert int(prl.mokjiThresholds(t[7]).cpu()) == _want(size, 3, 20)[1][7]


@pytest.mark.parametrize("c", [3, 4])
def test_colour_pages(prl, cuda_device, c):
    import torch

    for w, h in mr.SIZES:
        imgs = np.stack([mr.colour_page(w, h, s, c) for s in (1, 2, 3)])
        for e, m in ((3, 20), (1, 1)) + (((127, 20),) if (w, h) == mr.BIG else ()):
            want = [mr.mokji(img, e, m) for img in imgs]
            got = prl.binarizeMokji(_cuda(imgs), e, m)
            thr = prl.mokjiThresholds(_cuda(imgs), e, m)
            torch.cuda.synchronize()
            assert got.shape == (3, h, w) and thr.cpu().tolist() == [t for _, t in want], (w, h, c, e, m)
            n_bad, where = _mismatch(got.cpu().numpy(), np.stack([mask for mask, _ in want]))
            assert n_bad == 0, (w, h, c, e, m, where)
        one = prl.binarizeMokji(_cuda(imgs[1]))                           # H x W x C
        assert one.shape == (h, w) and np.array_equal(one.cpu().numpy(), mr.mokji(imgs[1])[0])


def test_in_place(prl, cuda_device):
    import torch

    size = (203, 117)
    w, h = size
    want, _ = _want(size, 3, 20)
    ip = _cuda(_pages(size))
    assert prl.binarizeMokji(ip, out=ip) is ip
    torch.cuda.synchronize()
    assert np.array_equal(ip.cpu().numpy(), want)
    sb = torch.full((want.shape[0], h + 2, w + 5), 9, dtype=torch.uint8, device="cuda")
    sv = sb[:, :h, :w]
    sv.copy_(torch.from_numpy(_pages(size)))
    prl.binarizeMokji(sv, out=sv)
    torch.cuda.synchronize()
    assert np.array_equal(sv.cpu().numpy(), want)
    s = sb.cpu().numpy()
    assert (s[:, h:] == 9).all() and (s[:, :, w:] == 9).all()


@pytest.mark.parametrize("c", [1, 3])
def test_strided_source_and_destination(prl, cuda_device, c):
    import torch

    w, h = 203, 117
    pages = _pages((w, h))[4:8] if c == 1 else np.stack([mr.colour_page(w, h, s) for s in (4, 5, 6, 7)])
    n = pages.shape[0]
    want = np.stack([mr.mokji(p, 3, 20)[0] for p in pages])
    # source rows of w c + 5 bytes, pages 9 rows apart; destination rows of w + 3 bytes, 4 spare rows: nothing a multiple of 4
    sb = torch.full((n, h + 9, w * c + 5), 7, dtype=torch.uint8, device="cuda")
    sv = sb[:, :h, :w * c]
    sv = sv.unflatten(2, (w, c)) if c == 3 else sv
    sv.copy_(torch.from_numpy(pages))
    db = torch.full((n, h + 4, w + 3), 201, dtype=torch.uint8, device="cuda")
    dv = db[:, :h, :w]
    prl.binarizeMokji(sv, out=dv)
    torch.cuda.synchronize()
    n_bad, where = _mismatch(dv.cpu().numpy(), want)
    assert n_bad == 0, where
    d = db.cpu().numpy()
    assert (d[:, h:] == 201).all() and (d[:, :, w:] == 201).all(), "padding bytes of the destination written"
    s = sb.cpu().numpy()
    assert np.array_equal(s[:, :h, :w * c].reshape(pages.shape), pages) and (s[:, h:] == 7).all() and (s[:, :, w * c:] == 7).all()


def test_edge_width_above_the_element_limit(prl, cuda_device):
    import torch

    from prlib_amd import _capi

    big = _cuda(_pages(mr.BIG)[6:8])
    marker = torch.full(big.shape, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(_capi.PrlError) as err:
        prl.binarizeMokji(big, 128, 20, out=marker)
    assert err.value.status == _capi.PRL_ERR_BAD_ARG
    with pytest.raises(_capi.PrlError) as err:
        prl.mokjiThresholds(big, 128, 20)
    assert err.value.status == _capi.PRL_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert (marker.cpu().numpy() == 3).all()
    small = _cuda(_pages((64, 64)))                                       # 64 <= 2 * 128: no interior, all 255
    got = prl.binarizeMokji(small, 128, 20)
    thr = prl.mokjiThresholds(small, 128, 20)
    torch.cuda.synchronize()
    assert (got.cpu().numpy() == 255).all() and set(thr.cpu().tolist()) == {-1}
    colour = prl.binarizeMokji(_cuda(mr.colour_page(64, 64, 1)), 32, 20)   # 64 <= 2 * 32, 3 channels
    assert (colour.cpu().numpy() == 255).all()


# ---- real data ------------------------------------------------------------------------------------------------------------------

def test_reference_scans(prl, cuda_device):
    gray = np.load(os.path.join(ROOT, "tests", "golden", "scans", "0018_x1000_y400_1536x1024.npz"))["gray"]
    bgr = np.load(os.path.join(ROOT, "tests", "golden", "stages", "chain_0004_x90_y150_900x1300.npz"))["bgr"]
    for name, img in (("gray scan", gray), ("colour scan", bgr)):
        want, t = mr.mokji(img)
        got = prl.binarizeMokji(_cuda(img)).cpu().numpy()
        thr = int(prl.mokjiThresholds(_cuda(img)).cpu())
        n_bad, where = _mismatch(got, want)
        print(f"{name} {img.shape}: t = {t} (device {thr}), {n_bad} mismatching bytes of {want.size}, {int((want == 0).sum())} ink pixels")
        assert thr == t and 0 < t < 255 and n_bad == 0, (name, where)


# ---- the other entry points -------------------------------------------------------------------------------------------------------

def test_host_entry_numpy(prl, cuda_device):
    w, h = 203, 117
    doc = _pages((w, h))[7]
    for img in (doc, doc[:, :, None], mr.colour_page(w, h, 3), mr.colour_page(w, h, 4, 4)):
        got = prl.binarizeMokji(img)
        assert got.shape == (h, w) and np.array_equal(got, mr.mokji(img)[0])
    view = mr.colour_page(240, 160, 9)[5:140, 7:231]   # strided rows
    assert np.array_equal(prl.binarizeMokji(view, 2, 30), mr.mokji(np.ascontiguousarray(view), 2, 30)[0])
    out = np.full((h, w), 3, np.uint8)
    assert prl.binarizeMokji(doc, 7, 40, out=out) is out and np.array_equal(out, mr.mokji(doc, 7, 40)[0])
    assert (prl.binarizeMokji(doc, 3, 300) == 255).all() and (prl.binarizeMokji(doc, 59, 20) == 255).all()


def test_cpp_dropin_on_device(prl, cuda_device, tmp_path):
    from test_mokji_cpu import build_dropin

    exe = build_dropin(str(tmp_path))
    for name, img, e, m, roi in (("bgr", mr.colour_page(333, 211, 4), 0, 0, False), ("bgr_roi", mr.colour_page(260, 190, 6), 2, 30, True),
                                 ("bgra", mr.colour_page(203, 117, 5, 4), 7, 40, False)):
        src = tmp_path / f"{name}.raw"
        dst = tmp_path / f"{name}.out"
        src.write_bytes(np.ascontiguousarray(img).tobytes())
        h, w, c = img.shape
        r = subprocess.run([exe, "run", str(e), str(m), str(h), str(w), str(c), str(src), str(dst)] + (["roi"] if roi else []),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "mokji dropin run: OK" in r.stdout, r.stdout + r.stderr
        view = np.ascontiguousarray(img[2:h - 3, 3:w - 4] if roi else img)
        got = np.frombuffer(dst.read_bytes(), np.uint8).reshape(view.shape[:2])
        want = mr.mokji(view, e or 3, m or 20)[0]
        assert np.array_equal(got, want), name
