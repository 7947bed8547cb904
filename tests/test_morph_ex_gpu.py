"""cv::morphologyEx with an anchor and iterations (prl_hip_morphology_ex_*, gmorph.hip) on the MI355X: every byte against the
numpy definition of tests/contour_ref.py (n real passes with the anchor as written), for the span kernel and, through the hooks
build in a child process, for the by-the-definition kernel."""
import os
import subprocess
import sys

import numpy as np
import pytest

import contour_ref as cr
import nuil_ref as nr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = [1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511]
HEIGHTS = [1, 2, 3, 17, 64, 65]
# every width with the heights in turn, then every height once more with another width: all of both lists, 21 shapes
SHAPES = [(w, HEIGHTS[i % len(HEIGHTS)]) for i, w in enumerate(WIDTHS)] + [(WIDTHS[(3 * i + 5) % len(WIDTHS)], h) for i, h in enumerate(HEIGHTS)]
CORNERS = lambda kw, kh: [(0, 0), (kw - 1, 0), (0, kh - 1), (kw - 1, kh - 1)]   # noqa: E731
ELEMENTS = ([(nr.RECT, 2, 2, -1, -1, n) for n in (1, 2, 3, 4)] +
            [(nr.RECT, 3, 2, ax, ay, 1) for ax, ay in CORNERS(3, 2)] + [(nr.RECT, 2, 5, ax, ay, 1) for ax, ay in CORNERS(2, 5)] +
            [(nr.RECT, 255, 1, 0, 0, 1), (nr.RECT, 255, 1, 254, 0, 1), (nr.CROSS, 3, 3, -1, -1, 3), (nr.ELLIPSE, 5, 5, 0, 4, 2)])


def pages_of(w, h, c, seed):
    """three pages: noise; set pixels in the first and last row and column on black; the same on white, cleared"""
    rng = np.random.default_rng(seed)
    p = np.zeros((3, h, w, c), np.uint8)
    p[0] = rng.integers(0, 256, size=(h, w, c))
    p[2] = 255
    for page, v in ((p[1], 255), (p[2], 0)):
        page[0, rng.integers(0, w)] = v
        page[h - 1, rng.integers(0, w)] = v
        page[rng.integers(0, h), 0] = v
        page[rng.integers(0, h), w - 1] = v
        page[0, 0, 0] = page[h - 1, w - 1, c - 1] = v
    return p


def _fold(pages):
    n, h, w, c = pages.shape
    return np.ascontiguousarray(pages.transpose(1, 2, 0, 3).reshape(h, w, n * c))


def _unfold(a, n, c):
    h, w = a.shape[:2]
    return np.ascontiguousarray(a.reshape(h, w, n, c).transpose(2, 0, 1, 3))


def want_all_ops(pages, el):
    """the six operators from four runs of the definition (channels and pages are independent: one page of N C channels)"""
    shape, kw, kh, ax, ay, n = el
    a = _fold(pages)
    run = lambda x, op: cr.morphology_ex(x, op, shape, kw, kh, ax, ay, n)   # noqa: E731
    e, d = run(a, nr.ERODE), run(a, nr.DILATE)
    o, cl = run(e, nr.DILATE), run(d, nr.ERODE)
    res = {nr.ERODE: e, nr.DILATE: d, nr.OPEN: o, nr.CLOSE: cl, nr.TOPHAT: nr._sat_sub(a, o), nr.BLACKHAT: nr._sat_sub(cl, a)}
    return {k: _unfold(v, pages.shape[0], pages.shape[3]) for k, v in res.items()}


def run_grid(prl, c, shapes=SHAPES, elements=ELEMENTS):
    """every shape x element x operator for `c` channels; returns the number of device calls"""
    import torch

    calls = 0
    for w, h in shapes:
        pages = pages_of(w, h, c, 7 * w + h + c)
        t = torch.from_numpy(pages).cuda()
        for el in elements:
            want = want_all_ops(pages, el)
            for op in nr.OPS:
                got = prl.morphology_ex(t, op, el[0], (el[1], el[2]), (el[3], el[4]), el[5]).cpu().numpy()
                bad = np.argwhere(got != want[op])
                assert bad.shape[0] == 0, (w, h, c, el, op, bad[:5].tolist())
                calls += 1
    return calls


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_grid_against_the_definition(prl, cuda_device, c):
    print(run_grid(prl, c), "calls")


def test_definition_agrees_with_the_loop_version():
    """the numpy definition itself, against a pixel loop with the anchor written out (no device)"""
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, size=(7, 9, 1), dtype=np.uint8)
    for shape, kw, kh, ax, ay in ((nr.RECT, 3, 2, 2, 0), (nr.RECT, 2, 2, 1, 1), (nr.CROSS, 3, 3, 0, 2)):
        mask = nr.element_mask(shape, kw, kh)
        for erode in (False, True):
            want = np.empty_like(a)
            for y in range(7):
                for x in range(9):
                    v = [int(a[y + i - ay, x + j - ax, 0]) for i in range(kh) for j in range(kw)
                         if mask[i, j] and 0 <= y + i - ay < 7 and 0 <= x + j - ax < 9]
                    want[y, x, 0] = (min(v) if erode else max(v)) if v else (255 if erode else 0)
            got = cr.morphology_ex(a, nr.ERODE if erode else nr.DILATE, shape, kw, kh, ax, ay, 1)
            assert np.array_equal(got, want), (shape, kw, kh, ax, ay, erode)
    # a full rectangle n times is the grown rectangle once, the anchor n times as far
    for n in (2, 3):
        assert np.array_equal(cr.morphology_ex(a, nr.DILATE, nr.RECT, 2, 3, 1, 0, n), cr.morphology_ex(a, nr.DILATE, nr.RECT, 1 + n, 1 + 2 * n, n, 0, 1))


def test_default_arguments_are_the_existing_entry(prl, cuda_device):
    import torch

    pages = pages_of(65, 33, 3, 5)
    t = torch.from_numpy(pages).cuda()
    for shape, k in ((nr.RECT, (2, 2)), (nr.ELLIPSE, (9, 5)), (nr.CROSS, (4, 7)), (nr.RECT, (31, 1))):
        for op in nr.OPS:
            a = prl.morphology_ex(t, op, shape, k, (-1, -1), 1).cpu().numpy()
            b = prl.morphologyEx(t, op, shape, k).cpu().numpy()
            assert np.array_equal(a, b), (shape, k, op)
            assert np.array_equal(a, want_all_ops(pages, (shape, k[0], k[1], -1, -1, 1))[op])
    img = pages[0]
    assert np.array_equal(prl.morphology_ex(img, nr.CLOSE, nr.RECT, 2, (-1, -1), 2), want_all_ops(img[None], (nr.RECT, 2, 2, -1, -1, 2))[nr.CLOSE][0])


def test_in_place_strided_and_page_seams(prl, cuda_device):
    import torch

    h, w, c = 19, 43, 3
    pages = pages_of(w, h, c, 11)
    n = pages.shape[0]
    for el in ((nr.RECT, 2, 2, -1, -1, 2), (nr.RECT, 3, 2, 2, 1, 1), (nr.RECT, 2, 5, 0, 4, 3), (nr.CROSS, 3, 3, -1, -1, 3), (nr.RECT, 2, 1, 0, 0, 1)):
        want = want_all_ops(pages, el)
        for op in nr.OPS:
            call = lambda t, out=None: prl.morphology_ex(t, op, el[0], (el[1], el[2]), (el[3], el[4]), el[5], out=out)   # noqa: E731
            # rows of 131 bytes from an odd address, pages 23 rows apart: nothing a multiple of 4
            sb = torch.full((n * 23 * 131 + 1,), 7, dtype=torch.uint8, device="cuda")
            sv = sb[1:].view(n, 23, 131)[:, :h, :w * c].unflatten(2, (w, c))
            sv.copy_(torch.from_numpy(pages))
            db = torch.full((n * 21 * 133 + 3,), 201, dtype=torch.uint8, device="cuda")
            dv = db[3:].view(n, 21, 133)[:, :h, :w * c].unflatten(2, (w, c))
            call(sv, out=dv)
            assert np.array_equal(dv.cpu().numpy(), want[op]), (el, op)
            d = db[3:].view(n, 21, 133).cpu().numpy()
            assert (d[:, h:] == 201).all() and (d[:, :, w * c:] == 201).all() and (db[:3] == 201).all(), "padding written"
            call(sv, out=sv)   # in place, strided
            assert np.array_equal(sv.cpu().numpy(), want[op]), ("in place", el, op)
            s = sb[1:].view(n, 23, 131).cpu().numpy()
            assert (s[:, h:] == 7).all() and (s[:, :, w * c:] == 7).all()
            ip = torch.from_numpy(pages).cuda()
            call(ip, out=ip)   # in place, dense
            assert np.array_equal(ip.cpu().numpy(), want[op]), ("in place, dense", el, op)
    # two pages back to back in memory, one black and one white: a halo read from the neighbour would show at the seam
    seam = np.zeros((2, 5, 8, 1), np.uint8)
    seam[1] = 255
    t = torch.from_numpy(seam).cuda()
    for ay in (0, 4):
        for op in (nr.DILATE, nr.ERODE):
            got = prl.morphology_ex(t, op, nr.RECT, (2, 5), (0, ay), 2).cpu().numpy()
            assert np.array_equal(got, seam), (ay, op)


def test_definition_kernel(prl, cuda_device):
    """k_gm_literal forced for every element (hooks build, PRL_HIP_GMORPH_LITERAL=1) in a child process: the same grid for 1 and 3
    channels on the shapes up to 65 columns and the two 255-wide row elements on 257 columns"""
    code = r'''
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from prlib_amd import _capi
_capi.use_library(_capi.HOOKS_LIB_PATH)
import torch, prlib_amd
import test_morph_ex_gpu as t
small = [s for s in t.SHAPES if s[0] <= 65]
calls = sum(t.run_grid(prlib_amd, c, small, [e for e in t.ELEMENTS if e[1] < 255]) for c in (1, 3))
calls += t.run_grid(prlib_amd, 4, [(257, 3)], [e for e in t.ELEMENTS if e[1] == 255])
print("literal ok", calls)
'''
    env = dict(os.environ, PRL_HIP_GMORPH_LITERAL="1")
    r = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "literal ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    print(r.stdout.strip())
