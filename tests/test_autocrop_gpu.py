"""prl::documentContour and prl::autoCrop on the MI355X against the restatement (tests/contour_ref.py fed with tests/edges_ref.py's
map): synthetic photographs of three sizes and three classes - found at once, found after the closing, not found -, a batch that
mixes the classes, gray and four-channel pages, two calls on one stream, the reference's photographs and the C++ drop-in.  Corners
are compared as float32 bits, crops byte for byte against tests/warp_ref.py on the truncated corners."""
import functools
import glob
import os
import subprocess

import numpy as np
import pytest

import autocrop_cases as ac
import contour_ref as cr
import warp_ref as wr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (width, height) -> the pages of that size: (kind, bridge, lean)
SIZES = {
    (900, 1300): [("found", None, 0.04), ("bridged", 10, 0.04), ("flat", None, 0.04)],
    (511, 300): [("found", None, 0.0), ("bridged", 2, 0.0), ("flat", None, 0.0)],      # no pyramid level
    (2480, 3508): [("found", None, 0.04), ("bridged", 16, 0.04)],
}
PHOTOS = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "autocrop", "*.npz")))


@functools.lru_cache(maxsize=None)
def case(w, h, kind, bridge, lean, channels=3):
    """(page, the restatement's quad as 8 float32 or None, try): computed once, shared, never written"""
    page = ac.page(w, h, kind, channels, bridge, lean=lean)
    quad, tries = cr.document_contour(page)
    page.setflags(write=False)
    return page, quad, tries


def klass(quad, tries):
    return "none" if quad is None else ("first", "closing")[tries]


def check(got, wants, where):
    quads, found, tries = got
    for i, (_page, quad, t) in enumerate(wants):
        print(where, i, "want", klass(quad, t), "got", bool(found[i]), int(tries[i]), quads[i].reshape(8).tolist())
        assert bool(found[i]) == (quad is not None) and int(tries[i]) == t, (where, i)
        want = np.zeros(8, np.float32) if quad is None else quad
        assert np.array_equal(quads[i].reshape(8).view(np.uint32), want.view(np.uint32)), (where, i, quads[i], want)


@pytest.mark.parametrize("size", sorted(SIZES), ids=lambda s: "%dx%d" % s)
def test_sizes_against_the_restatement(prl, cuda_device, size):
    import torch

    wants = [case(*size, *k) for k in SIZES[size]]
    t = torch.from_numpy(np.stack([w[0] for w in wants])).cuda()
    check(prl.document_contour(t), wants, size)
    one = prl.document_contour(t[0])   # a tensor without a page axis
    check(([one[0]], [one[1]], [one[2]]), wants[:1], (size, "one page"))


def test_the_restatement_alone_puts_pages_in_each_class():
    seen = {}
    for size, kinds in SIZES.items():
        if size[0] > 1000:
            continue   # (the A4 pages are classified where they are compared)
        for k in kinds:
            _p, quad, tries = case(*size, *k)
            seen.setdefault(klass(quad, tries), []).append((size, k[0]))
    print(seen)
    assert set(seen) == {"first", "closing", "none"}
    assert all(kind == {"first": "found", "closing": "bridged", "none": "flat"}[c] for c, v in seen.items() for _s, kind in v)


def test_a4_classes(prl, cuda_device):
    assert [klass(*case(2480, 3508, *k)[1:]) for k in SIZES[(2480, 3508)]] == ["first", "closing"]


def test_mixed_batch_closes_a_subset_and_crops(prl, cuda_device):
    import torch

    kinds = SIZES[(900, 1300)]
    order = [0, 1, 2, 1, 0, 2, 2, 1]
    wants = [case(900, 1300, *kinds[i]) for i in order]
    pages = np.stack([w[0] for w in wants])
    t = torch.from_numpy(pages).cuda()
    crops, contour = prl.auto_crop(t, return_contour=True)
    check(contour, wants, "mixed")
    assert len(crops) == len(order)
    done = {}
    for i, (page, quad, _t) in enumerate(wants):
        if quad is None:
            assert crops[i] is None, i
            continue
        q = quad.astype(np.int32)   # (int)float
        if order[i] not in done:
            done[order[i]] = wr.warp_crop(page, [int(v) for v in q])
        want = done[order[i]]
        got = crops[i].cpu().numpy()
        assert got.shape == want.shape == tuple(prl.warp_crop_size(q)[::-1]) + (3,), (i, got.shape, want.shape)
        assert np.array_equal(got, want), (i, int((got != want).sum()))
    assert torch.equal(t.cpu(), torch.from_numpy(pages)), "the pages are not written"


def test_chunks_of_three_pages(prl, cuda_device, tmp_path):
    """the hooks build with PRL_HIP_STAGE_CHUNK=3 in a child process: eight pages in three chunks, the closing's subset in each"""
    import sys

    code = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from prlib_amd import _capi
_capi.use_library(_capi.HOOKS_LIB_PATH)
import torch, prlib_amd
quads, found, tries = prlib_amd.document_contour(torch.from_numpy(np.load(sys.argv[2])).cuda())
np.savez(sys.argv[3], quads=quads, found=found, tries=tries)
print("chunks ok")
'''
    kinds = SIZES[(511, 300)]
    order = [1, 0, 2, 2, 1, 1, 0, 1]
    wants = [case(511, 300, *kinds[i]) for i in order]
    src, dst = str(tmp_path / "pages.npy"), str(tmp_path / "out.npz")
    np.save(src, np.stack([w[0] for w in wants]))
    r = subprocess.run([sys.executable, "-c", code, ROOT, src, dst], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, PRL_HIP_STAGE_CHUNK="3"))
    assert r.returncode == 0 and "chunks ok" in r.stdout, r.stdout + r.stderr[-3000:]
    z = np.load(dst)
    check((z["quads"], z["found"], z["tries"]), wants, "chunks of 3")


@pytest.mark.parametrize("channels", [1, 4])
def test_gray_and_four_channel_pages(prl, cuda_device, channels):
    import torch

    wants = [case(511, 300, *k, channels) for k in SIZES[(511, 300)]] + [case(900, 1300, "found", None, 0.04, channels)]
    assert {klass(q, t) for _p, q, t in wants} == {"first", "closing", "none"}
    for group in (wants[:3], wants[3:]):
        t = torch.from_numpy(np.stack([w[0] for w in group])).cuda()
        check(prl.document_contour(t), group, ("channels", channels))
    got = prl.document_contour(np.asarray(wants[1][0]))   # one host image
    check(([got[0]], [got[1]], [got[2]]), wants[1:2], ("host", channels))


def test_two_calls_back_to_back_on_one_stream(prl, cuda_device):
    import torch

    a = [case(511, 300, *k) for k in SIZES[(511, 300)]]
    b = [case(900, 1300, *k) for k in SIZES[(900, 1300)]][::-1]
    ta, tb = (torch.from_numpy(np.stack([w[0] for w in g])).cuda() for g in (a, b))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ga = prl.document_contour(ta)
        gb = prl.document_contour(tb)
        ga2 = prl.document_contour(ta)
    s.synchronize()
    check(ga, a, "first call")
    check(gb, b, "second call")
    check(ga2, a, "third call")


def test_strided_pages(prl, cuda_device):
    import torch

    wants = [case(511, 300, *k) for k in SIZES[(511, 300)]]
    buf = torch.full((3, 307, 511 * 3 + 5), 9, dtype=torch.uint8, device="cuda")
    view = buf[:, :300, :511 * 3].unflatten(2, (511, 3))
    view.copy_(torch.from_numpy(np.stack([w[0] for w in wants])))
    check(prl.document_contour(view), wants, "strided")


@pytest.mark.parametrize("path", PHOTOS, ids=[os.path.basename(p)[:-4] for p in PHOTOS])
def test_reference_photographs(prl, cuda_device, path):
    import torch

    z = np.load(path)
    bgr, quad, found, tries = z["bgr"], z["quad"], int(z["found"]), int(z["tries"])
    crops, contour = prl.auto_crop(torch.from_numpy(bgr).cuda()[None], return_contour=True)
    check(contour, [(bgr, quad if found else None, tries)], os.path.basename(path))
    if not found:
        assert crops == [None]
        return
    want = wr.warp_crop(bgr, [int(v) for v in quad.astype(np.int32)])
    got = crops[0].cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want), (got.shape, want.shape)


def test_photograph_fixtures_are_there():
    assert len(PHOTOS) >= 3 and any(int(np.load(p)["found"]) for p in PHOTOS) and not all(int(np.load(p)["found"]) for p in PHOTOS)


def test_cpp_dropin_on_device(prl, cuda_device, tmp_path):
    from test_autocrop_cpu import build_dropin

    exe = build_dropin(str(tmp_path))
    found_photo = [p for p in PHOTOS if int(np.load(p)["found"])][0]
    z = np.load(found_photo)
    gray_page, gray_quad, _t = case(511, 300, "found", None, 0.0, 1)
    for name, img, quad in (("photo", z["bgr"], z["quad"]), ("gray", np.asarray(gray_page), gray_quad),
                            ("flat", np.asarray(case(511, 300, "flat", None, 0.0)[0]), None)):
        src, dst = tmp_path / f"{name}.raw", tmp_path / f"{name}.out"
        src.write_bytes(np.ascontiguousarray(img).tobytes())
        h, w = img.shape[:2]
        c = img.shape[2] if img.ndim == 3 else 1
        r = subprocess.run([exe, "run", str(h), str(w), str(c), str(src), str(dst)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "autocrop dropin run: OK" in r.stdout, r.stdout + r.stderr
        assert ("found 1" in r.stdout) == (quad is not None), r.stdout
        if quad is None:
            continue
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("quad")][0]
        assert np.array_equal(np.array(line.split()[1:], np.float64).astype(np.float32), quad), (line, quad)
        bgr = img if img.ndim == 3 else np.repeat(img[:, :, None], 3, axis=2)   # a gray input is cropped as BGR
        want = wr.warp_crop(bgr, [int(v) for v in quad.astype(np.int32)])
        got = np.frombuffer(dst.read_bytes(), np.uint8).reshape(want.shape)
        assert np.array_equal(got, want), name
