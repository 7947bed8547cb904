"""cv::HoughLines(rho 1, theta pi / 180) and prl::findHoughLineContour on the MI355X against the restatement
(tests/houghline_ref.py): every accumulator cell, every line as float32 bits and in order, every pixel of the edge map, every
corner.  The references are computed once per case (functools.lru_cache) and shared."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import houghline_cases as hc
import houghline_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_CELLS = 12288   # rho cells one workgroup of k_hough_vote keeps (hough.hip): numrho = 12287 is the widest row in one range


def bits(lines):
    return np.ascontiguousarray(lines, np.float32).view(np.uint32).reshape(-1, 2)


def thin_map(w, h):
    """a handful of points on a long thin page, the far ends included: rho runs over the whole row"""
    m = np.zeros((h, w), np.uint8)
    for x, y in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, 1 % h), (w // 3, 0), (w - 2, h - 1), (5, h - 1)):
        m[y, x] = 255
    return m


ACC_MAPS = {
    "1x1": lambda: np.full((1, 1), 9, np.uint8), "1x7": lambda: hc.sparse_map(1, 7, 1, 3), "7x1": lambda: hc.sparse_map(7, 1, 2, 3),
    "64x48": lambda: hc.sparse_map(64, 48, 3), "65x63": lambda: hc.sparse_map(65, 63, 4), "257x3": lambda: hc.sparse_map(257, 3, 5),
    "thin_one_range": lambda: thin_map(6140, 3), "thin_two_ranges": lambda: thin_map(6141, 3), "thin_split_in_the_middle": lambda: thin_map(9001, 2),
    "corners_64x48": lambda: hc.corner_map(64, 48), "corners_1x2": lambda: hc.corner_map(1, 2), "corners_300x7": lambda: hc.corner_map(300, 7),
}


@functools.lru_cache(maxsize=None)
def acc_case(name):
    m = ACC_MAPS[name]()
    m.setflags(write=False)
    acc = ref.accumulator(m)
    acc.setflags(write=False)
    return m, acc


@functools.lru_cache(maxsize=None)
def designed():
    return {k: (v, {t: ref.hough_lines(v, t) for t in (0, 1, 50)}) for k, v in hc.designed_maps().items()}


@pytest.mark.parametrize("name", list(ACC_MAPS))
def test_accumulator_every_cell(prl, cuda_device, name):
    import torch

    m, want = acc_case(name)
    h, w = m.shape
    numrho = 2 * (w + h) + 1
    if name == "thin_one_range":
        assert numrho == LDS_CELLS - 1
    if name == "thin_two_ranges":
        assert numrho == LDS_CELLS + 1
    got = prl.hough_accumulator(torch.from_numpy(np.array(m)).to(cuda_device))
    assert got.shape == (182, numrho + 2) and got.dtype == torch.int32
    got = got.cpu().numpy()
    assert int(want.sum()) == 180 * int((m != 0).sum())
    assert np.array_equal(got, want), (name, int((got != want).sum()))


@pytest.mark.parametrize("name", ["empty", "row", "last_column", "diagonal", "ones"])
def test_designed_maps_lines_in_order(prl, cuda_device, name):
    import torch

    m, wants = designed()[name]
    t = torch.from_numpy(m).to(cuda_device)
    for thr in (0, 1, 50):
        got, count = prl.hough_lines(t, thr, return_counts=True)
        want = wants[thr]
        assert count == len(want) == len(got), (name, thr, count, len(want))
        assert np.array_equal(bits(got), bits(want)), (name, thr)
    if name == "empty":
        assert len(wants[0]) == 0
    if name == "ones":
        assert len(wants[0]) > 4 and len(wants[50]) == 0   # many equal counts: the order falls to the cell index


def test_mixed_batch(prl, cuda_device):
    import torch

    w, h = 33, 29
    one = np.zeros((h, w), np.uint8)
    one[11, 20] = 1
    pages = np.stack([np.zeros((h, w), np.uint8), hc.sparse_map(w, h, 8, points=w * h // 2), one, hc.corner_map(w, h)])
    t = torch.from_numpy(pages).to(cuda_device)
    acc = prl.hough_accumulator(t).cpu().numpy()
    for i in range(len(pages)):
        assert np.array_equal(acc[i], ref.accumulator(pages[i])), i
    for thr in (0, 3):
        got, counts = prl.hough_lines(t, thr, return_counts=True)
        for i in range(len(pages)):
            want = ref.hough_lines(pages[i], thr)
            assert counts[i] == len(want) and np.array_equal(bits(got[i]), bits(want)), (thr, i)
    assert len(got[0]) == 0 and len(ref.hough_lines(one, 0)) > 0


def test_pitched_and_odd_addressed_views(prl, cuda_device):
    import torch

    w, h, n = 65, 63, 3
    pages = np.stack([hc.sparse_map(w, h, 20 + i) for i in range(n)])
    step, page = w + 6, (w + 6) * h + 11
    buf = torch.full((1 + n * page + 64,), 255, dtype=torch.uint8, device=cuda_device)   # what lies between the rows is non-zero
    view = torch.as_strided(buf, (n, h, w), (page, step, 1), storage_offset=1)
    view.copy_(torch.from_numpy(pages).to(cuda_device))
    assert view.data_ptr() % 2 == 1 and not view.is_contiguous()
    acc = prl.hough_accumulator(view).cpu().numpy()
    lines = prl.hough_lines(view, 2)
    # strided accumulator pages: every second page of a larger tensor
    out = torch.full((2 * n, 182, 2 * (w + h) + 3), -7, dtype=torch.int32, device=cuda_device)
    prl.hough_accumulator(view, out=out[::2])
    out = out.cpu().numpy()
    for i in range(n):
        want = ref.accumulator(pages[i])
        assert np.array_equal(acc[i], want) and np.array_equal(out[2 * i], want) and (out[2 * i + 1] == -7).all(), i
        assert np.array_equal(bits(lines[i]), bits(ref.hough_lines(pages[i], 2))), i


def test_two_calls_on_one_stream(prl, cuda_device):
    """the second call reuses the first one's workspace while the first may still run: the stream orders them"""
    import torch

    a, b = hc.sparse_map(300, 200, 31, points=9000), hc.sparse_map(64, 48, 32)
    ta, tb = torch.from_numpy(a).to(cuda_device), torch.from_numpy(b).to(cuda_device)
    s = torch.cuda.Stream(device=cuda_device)
    s.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(s):
        acc_a = prl.hough_accumulator(ta)
        acc_b = prl.hough_accumulator(tb)
        acc_a2 = prl.hough_accumulator(ta)
        lines_b = prl.hough_lines(tb, 1)
    s.synchronize()
    want_a = ref.accumulator(a)
    assert np.array_equal(acc_a.cpu().numpy(), want_a) and np.array_equal(acc_a2.cpu().numpy(), want_a)
    assert np.array_equal(acc_b.cpu().numpy(), ref.accumulator(b))
    assert np.array_equal(bits(lines_b), bits(ref.hough_lines(b, 1)))


def test_room_for_fewer_lines_than_found(prl, cuda_device):
    import torch

    pages = np.stack([hc.sparse_map(64, 48, 40), np.zeros((48, 64), np.uint8), hc.designed_maps()["ones"].repeat(6, 0).repeat(8, 1)])
    t = torch.from_numpy(pages).to(cuda_device)
    wants = [ref.hough_lines(p, 1) for p in pages]
    assert len(wants[0]) > 5 and len(wants[1]) == 0 and len(wants[2]) > 5
    got, counts = prl.hough_lines(t, 1, max_lines=5, return_counts=True)
    for i in range(3):
        assert counts[i] == len(wants[i]), (i, counts[i], len(wants[i]))        # the totals, not what fitted
        assert np.array_equal(bits(got[i]), bits(wants[i][:5])), i              # and the first five of the order
    _none, counts = prl.hough_lines(t, 1, max_lines=0, return_counts=True)
    assert counts.tolist() == [len(w) for w in wants]
    # the one-page host entry
    got, count = prl.hough_lines(pages[0], 1, max_lines=3, return_counts=True)
    assert count == len(wants[0]) and np.array_equal(bits(got), bits(wants[0][:3]))
    assert np.array_equal(bits(prl.hough_lines(pages[2], 1)), bits(wants[2]))


@functools.lru_cache(maxsize=None)
def edge_case(w, h, kind, channels):
    img = hc.edge_page(w, h, kind, channels, seed=5)
    img.setflags(write=False)
    want = ref.hough_edges(img)
    want.setflags(write=False)
    return img, want


@pytest.mark.parametrize("channels", [1, 3, 4])
@pytest.mark.parametrize("size", [(65, 63), (300, 200)])
def test_edge_map(prl, cuda_device, size, channels):
    import torch

    w, h = size
    cases = [edge_case(w, h, kind, channels) for kind in ("random", "stroke")]
    if channels > 1:   # (tests/test_houghline_cpu.py chose the seed: every channel gives a gradient, two channels tie)
        for img, _want in cases:
            _dx, _dy, mp, best, tied = ref.colour_gradients(ref.blurred(img))
            assert set(np.unique(best)) == set(range(channels)) and (tied & (mp[1:-1, 1:-1] > 0)).any()
    assert any(want.any() for _img, want in cases)
    pages = np.stack([np.array(img) for img, _want in cases])
    t = torch.from_numpy(pages).to(cuda_device)
    got = prl.hough_edges(t)
    assert got.shape == (2, h, w) and got.dtype == torch.uint8
    got = got.cpu().numpy()
    for i, (_img, want) in enumerate(cases):
        assert set(np.unique(got[i])) <= {0, 255}
        assert np.array_equal(got[i], want), (size, channels, i, int((got[i] != want).sum()))
    assert torch.equal(t.cpu(), torch.from_numpy(pages)), "the pages are not written"
    # one page: a tensor without a page axis, and a host image
    one = prl.hough_edges(t[1]).cpu().numpy()
    assert one.shape == (h, w) and np.array_equal(one, cases[1][1])
    if size == (65, 63):
        assert np.array_equal(prl.hough_edges(np.array(cases[0][0])), cases[0][1])


PHOTOS = {(511, 300): (3, ("found", "flat", "broken", "stripes", "found")), (900, 1300): (1, ("broken", "stripes", "found", "flat"))}


@functools.lru_cache(maxsize=None)
def photo_case(w, h, kind, channels):
    img = hc.photo(w, h, kind, channels)
    img.setflags(write=False)
    quad, n_lines = ref.hough_line_contour(img)
    print(f"photo {w} x {h} {kind} c{channels}: {n_lines} lines, quad {None if quad is None else quad.tolist()}")
    assert n_lines < 500   # the Python filter stays no long pole
    return img, quad, n_lines


def check_contour(got, wants, what):
    quads, found, lines = got
    for i, (_img, quad, n_lines) in enumerate(wants):
        assert bool(found[i]) == (quad is not None), (what, i)
        assert int(lines[i]) == n_lines, (what, i, int(lines[i]), n_lines)
        assert np.array_equal(quads[i], quad if quad is not None else np.zeros((4, 2), np.int32)), (what, i, quads[i].tolist())


@pytest.mark.parametrize("size", list(PHOTOS))
def test_contour_mixed_batch(prl, cuda_device, size):
    import torch

    w, h = size
    channels, kinds = PHOTOS[size]
    wants = [photo_case(w, h, kind, channels) for kind in kinds]
    classes = {want[1] is not None for want in wants}
    assert classes == {True, False}
    assert any(want[1] is None and want[2] >= 4 for want in wants)   # lines enough and still no quad
    pages = np.stack([np.array(want[0]) for want in wants])
    t = torch.from_numpy(pages).to(cuda_device)
    got = prl.hough_line_contour(t)
    assert got[0].dtype == np.int32 and got[0].shape == (len(kinds), 4, 2)
    check_contour(got, wants, size)
    assert torch.equal(t.cpu(), torch.from_numpy(pages)), "the pages are not written"


@pytest.mark.parametrize("channels", [1, 4])
def test_contour_one_page(prl, cuda_device, channels):
    import torch

    for kind in ("found", "flat"):
        want = photo_case(511, 300, kind, channels)
        img = np.array(want[0])
        quad, found, lines = prl.hough_line_contour(torch.from_numpy(img).to(cuda_device))
        check_contour((quad[None], [found], [lines]), [want], ("tensor", kind))
        quad, found, lines = prl.hough_line_contour(img)   # the host entry
        check_contour((quad[None], [found], [lines]), [want], ("host", kind))


def test_contour_equals_its_stages(prl, cuda_device):
    """hough_line_contour is hough_edges, hough_lines(50) and hough_line_quad in a row"""
    import torch

    want = photo_case(511, 300, "broken", 3)
    t = torch.from_numpy(np.array(want[0])).to(cuda_device)
    edges = prl.hough_edges(t)
    assert np.array_equal(edges.cpu().numpy(), ref.hough_edges(want[0]))
    lines = prl.hough_lines(edges, 50)
    assert len(lines) == want[2] and np.array_equal(bits(lines), bits(ref.hough_lines(edges.cpu().numpy(), 50)))
    assert np.array_equal(prl.hough_line_quad(lines, 511, 300), want[1])


def test_chunks_of_two_pages(prl, cuda_device, tmp_path):
    """the hooks build with PRL_HIP_STAGE_CHUNK=2 in a child process: five pages run as 2, 2, 1 through every batch entry"""
    code = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from prlib_amd import _capi
_capi.use_library(_capi.HOOKS_LIB_PATH)
import torch, prlib_amd
z = np.load(sys.argv[2])
maps, photos = torch.from_numpy(z["maps"]).cuda(), torch.from_numpy(z["photos"]).cuda()
acc = prlib_amd.hough_accumulator(maps).cpu().numpy()
lines, counts = prlib_amd.hough_lines(maps, 1, return_counts=True)
edges = prlib_amd.hough_edges(photos).cpu().numpy()
quads, found, n_lines = prlib_amd.hough_line_contour(photos)
np.savez(sys.argv[3], acc=acc, counts=counts, lines=np.concatenate(lines), edges=edges, quads=quads, found=found, n_lines=n_lines)
print("chunks ok")
'''
    maps = np.stack([hc.sparse_map(64, 48, 50 + i, points=20 + 300 * (i % 3)) for i in range(5)])
    kinds = ("flat", "found", "stripes", "broken", "found")
    wants = [photo_case(511, 300, kind, 3) for kind in kinds]
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, maps=maps, photos=np.stack([np.array(w[0]) for w in wants]))
    r = subprocess.run([sys.executable, "-c", code, ROOT, src, dst], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, PRL_HIP_STAGE_CHUNK="2"))
    assert r.returncode == 0 and "chunks ok" in r.stdout, r.stdout + r.stderr[-3000:]
    z = np.load(dst)
    want_lines = [ref.hough_lines(m, 1) for m in maps]
    for i in range(5):
        assert np.array_equal(z["acc"][i], ref.accumulator(maps[i])), i
        assert np.array_equal(z["edges"][i], ref.hough_edges(wants[i][0])), i
    assert z["counts"].tolist() == [len(w) for w in want_lines]
    assert np.array_equal(bits(z["lines"]), bits(np.concatenate(want_lines)))
    check_contour((z["quads"], z["found"], z["n_lines"]), wants, "chunks of 2")


def test_cpp_dropin_on_device(prl, cuda_device, tmp_path):
    from test_houghline_cpu import build_dropin

    exe = build_dropin(str(tmp_path))
    for kind, channels in (("found", 3), ("flat", 1), ("broken", 1)):
        img, quad, _n = photo_case(511, 300, kind, channels)
        src = tmp_path / f"{kind}.raw"
        src.write_bytes(np.ascontiguousarray(img).tobytes())
        r = subprocess.run([exe, "run", "300", "511", str(channels), str(src)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "houghline dropin run: OK" in r.stdout, r.stdout + r.stderr[-3000:]
        out = r.stdout.splitlines()
        assert out[0] == f"found {0 if quad is None else 1}", (kind, out)
        if quad is not None:
            assert [int(v) for v in out[1].split()[1:]] == quad.reshape(8).tolist(), kind
