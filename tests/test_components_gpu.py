"""components.hip on the device: prl_hip_external_rects_batch_device against the library's host scan prl_hip_external_rects (the
yardstick: rectangles, their order, found and kept), and prl_hip_connected_components_batch_device (labels and statistics at
connectivity 4 and 8) against the flood fills of tests/components_ref.py.  No expected value comes from the code under test.
T = 32 is the side of the labeller's tile; the pages are chosen around it: every side at which a seam appears or vanishes, every
direction a component can cross one, the longest ways round a page of (4 T + 1)^2, and the capacity rules.  Every comparison is an
equality."""
import os
import subprocess
import sys

import numpy as np
import pytest

import components_ref as cr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 32


def host_answer(prl, m):
    rects, found = prl.externalRects(np.ascontiguousarray(m))   # the host scan (localotsu.externalRects)
    return [tuple(r) for r in rects.tolist()], found


def check_rects(prl, dev, pages, name=""):
    """the device rectangles of a list of equally sized pages (one call) against the host scan; returns the host's answers"""
    import torch

    from prlib_amd import components

    batch = torch.from_numpy(np.stack(pages)).to(dev)
    rects, found = components.externalRects(batch)
    want = [host_answer(prl, m) for m in pages]
    for i, m in enumerate(pages):
        got = ([tuple(r) for r in rects[i].tolist()], int(found[i]))
        assert got == want[i], (name, i, got[1], want[i][1], got[0][:6], want[i][0][:6])
    return want


def check_labels(prl, dev, pages, name=""):
    import torch

    batch = torch.from_numpy(np.stack(pages)).to(dev)
    for conn in (8, 4):
        labels, counts, stats = prl.connectedComponents(batch, conn, with_stats=True)
        labels = labels.cpu().numpy()
        for i, m in enumerate(pages):
            want_labels, want_stats = cr.components(m, conn)
            assert int(counts[i]) == len(want_stats), (name, conn, i, int(counts[i]), len(want_stats))
            assert np.array_equal(labels[i], want_labels), (name, conn, i)
            assert np.array_equal(stats[i].cpu().numpy(), want_stats), (name, conn, i)


def check(prl, dev, pages, name=""):
    want = check_rects(prl, dev, pages, name)
    check_labels(prl, dev, pages, name)
    return want


def rnd(h, w, density, seed):
    return ((np.random.default_rng(seed).random((h, w)) < density) * 255).astype(np.uint8)


def test_every_4x4_map_on_one_page(prl, cuda_device):
    """all 65 536 maps as cells at a pitch of 5 on a 1280 x 1280 page"""
    maps = cr.all_maps(4, 4).reshape(256, 256, 4, 4)
    page = np.zeros((256, 5, 256, 5), np.uint8)
    page[:, :4, :, :4] = maps.transpose(0, 2, 1, 3)
    page = page.reshape(1280, 1280)
    assert np.array_equal(page[5:9, 10:14], cr.all_maps(4, 4)[258])
    (rects, found), = check(prl, cuda_device, [page], "4 x 4 cells")
    print("found", found, "kept", len(rects))
    assert found > 65536


@pytest.mark.parametrize("side", [1, 2, 3, T - 1, T, T + 1, 2 * T + 1])
def test_page_sizes_around_the_tile(prl, cuda_device, side):
    for h, w in ((side, side), (1, side), (side, 1)):
        for k, density in enumerate((0.1, 0.5, 0.9)):
            check(prl, cuda_device, [rnd(h, w, density, 100 * side + 10 * k + (h == 1) + 2 * (w == 1))], (h, w, density))


def seam_pages():
    z = lambda: np.zeros((3 * T, 3 * T), np.uint8)
    out = {}
    for name, (dx, dy) in (("right", (1, 0)), ("left", (-1, 0)), ("down", (0, 1)), ("up", (0, -1))):
        m = z()   # a hook that starts in the middle tile and ends in the neighbour, so that the first pixel is on either side
        x, y = T + T // 2, T + T // 2
        for i in range(T):
            m[y + dy * i, x + dx * i] = 255
        m[y + dy * (T - 1) + (1 if dx else 0), x + dx * (T - 1) + (1 if dy else 0)] = 255
        out["across a seam " + name] = m
    m = z()
    m[T - 3:T, T - 3:T] = 255
    m[T:T + 3, T:T + 3] = 255          # touch at the corner of four tiles only
    out["diagonal touch"] = m
    m = z()
    m[T - 3:T, T:T + 3] = 255
    m[T:T + 3, T - 3:T] = 255
    out["anti-diagonal touch"] = m
    m = z()                            # a ring with one corner cut: its hole touches the outside diagonally only; a blob inside
    m[T - 4:T + 5, T - 4] = m[T - 4:T + 5, T + 4] = m[T - 4, T - 4:T + 5] = m[T + 4, T - 4:T + 5] = 255
    m[T - 4, T - 4] = 0
    m[T - 1:T + 2, T - 1:T + 2] = 255
    out["diagonal pocket"] = m
    m = z()
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = 255
    m[T:T + 5, T:T + 5] = 255
    out["ring on the page border"] = m
    m = z()
    m[T - 1, T - 1:2 * T + 1] = m[2 * T, T - 1:2 * T + 1] = m[T - 1:2 * T + 1, T - 1] = m[T - 1:2 * T + 1, 2 * T] = 255
    m[T + 10:T + 14, T + 10:T + 14] = 255
    out["ring on the seams, outside"] = m
    m = z()
    m[T, T:2 * T] = m[2 * T - 1, T:2 * T] = m[T:2 * T, T] = m[T:2 * T, 2 * T - 1] = 255
    m[T + 10:T + 14, T + 10:T + 14] = 255
    out["ring on the seams, inside"] = m
    return out


def test_seams(prl, cuda_device):
    import torch

    pages = seam_pages()
    want = dict(zip(pages, check(prl, cuda_device, list(pages.values()), "seams")))
    for name in ("diagonal touch", "anti-diagonal touch"):
        assert want[name] == ([(T - 3, T - 3, 6, 6)], 1), name
        for conn, k in ((8, 1), (4, 2)):
            assert prl.connectedComponents(torch.from_numpy(pages[name]).to(cuda_device), conn)[1] == k, (name, conn)
    assert want["diagonal pocket"] == ([(T - 4, T - 4, 9, 9)], 1), "the blob in the pocket is not external"
    assert want["ring on the page border"] == ([(0, 0, 3 * T, 3 * T)], 1)
    assert want["ring on the seams, outside"][1] == 1 and want["ring on the seams, inside"][1] == 1


def long_pages():
    n = 4 * T + 1
    spiral = np.zeros((n, n), np.uint8)
    x0, y0, x1, y1 = 0, 0, n - 1, n - 1
    spiral[0, :] = 255
    while x1 - x0 >= 2 and y1 - y0 >= 2:      # a one-pixel path winding inwards, one background pixel between its turns
        spiral[y0:y1 + 1, x1] = 255
        spiral[y1, x0:x1 + 1] = 255
        spiral[y0 + 2:y1 + 1, x0] = 255
        spiral[y0 + 2, x0:x1 - 1] = 255
        x0, y0, x1, y1 = x0 + 2, y0 + 2, x1 - 2, y1 - 2
    comb = np.zeros((n, n), np.uint8)
    comb[::2, :] = 255
    comb[1::4, 0] = 255
    comb[3::4, n - 1] = 255                    # a serpentine: the rows joined at alternating ends
    board = ((np.add.outer(np.arange(n), np.arange(n)) % 2 == 0) * 255).astype(np.uint8)
    return {"spiral": spiral, "comb": comb, "checkerboard": board, "inverse checkerboard": 255 - board,
            "zero": np.zeros((n, n), np.uint8), "full": np.full((n, n), 255, np.uint8)}


def test_the_long_ways_round(prl, cuda_device):
    import torch

    pages = long_pages()
    n = 4 * T + 1
    for name in ("spiral", "comb"):
        assert cr.components(pages[name], 8)[1].tolist() == cr.components(pages[name], 4)[1].tolist() and \
            cr.components(pages[name], 4)[1][0, 4] == (pages[name] != 0).sum(), name + " is one path"
    want = dict(zip(pages, check(prl, cuda_device, list(pages.values()), "long")))
    assert want["zero"] == ([], 0) and want["full"] == ([(0, 0, n, n)], 1)
    assert want["checkerboard"] == ([(0, 0, n, n)], 1)
    counts = prl.connectedComponents(torch.from_numpy(pages["checkerboard"]).to(cuda_device), 4)[1]
    assert counts == (n * n + 1) // 2, "the most components a page can have"


def test_nesting(prl, cuda_device):
    for wall in (1, 7):
        blob = np.full((3, 3), 255, np.uint8)
        m = cr.framed(cr.nested_rings(3, wall, gap=4, core=cr.framed(blob, 2)), 5)
        assert m.shape[0] > T
        # a blob in every hole, beside the next ring
        size = m.shape[0]
        for d in range(3):
            at = 5 + d * (wall + 4) + wall + 1
            m[at:at + 2, size // 2:size // 2 + 2] = 255
        (rects, found), = check(prl, cuda_device, [m], f"nested, wall {wall}")
        assert (rects, found) == ([(5, 5, size - 10, size - 10)], 1), "only the outermost ring is reported"
        assert cr.components(m, 8)[1].shape[0] == 7


def test_straight_lines_are_found_and_not_kept(prl, cuda_device):
    pages, kinds = [], []
    for length in (1, 2, T + 1):
        for kind in ("horizontal", "vertical", "diagonal", "anti-diagonal"):
            m = np.zeros((2 * T + 8, 2 * T + 8), np.uint8)
            for i in range(length):
                y, x = {"horizontal": (20, 20 + i), "vertical": (20 + i, 20), "diagonal": (20 + i, 20 + i), "anti-diagonal": (20 + i, 60 - i)}[kind]
                m[y, x] = 255
            pages.append(m)
            kinds.append((kind, length))
    el = np.zeros((2 * T + 8, 2 * T + 8), np.uint8)
    el[T - 1, T - 1] = el[T, T - 1] = el[T, T] = 255
    pages.append(el)
    want = check(prl, cuda_device, pages, "lines")
    for kind, (rects, found) in zip(kinds, want[:-1]):
        assert (rects, found) == ([], 1), kind
    assert want[-1] == ([(T - 1, T - 1, 2, 2)], 1), "an L of 3 pixels is kept"


def test_a_batch_of_three_and_pitched_views(prl, cuda_device):
    import torch

    from prlib_amd import components

    h, w = 2 * T + 5, 3 * T - 7
    pages = [rnd(h, w, 0.3, 1), cr.dilate(rnd(h, w, 0.02, 2), 3), rnd(h, w, 0.7, 3)]
    want = check(prl, cuda_device, pages, "batch")
    assert len({f for _r, f in want}) == 3
    buf = torch.full((3, h + 3, w + 9), 255, dtype=torch.uint8, device=cuda_device)   # the pad bytes are foreground, were they read
    buf[:, :h, :w] = torch.from_numpy(np.stack(pages)).to(cuda_device)
    view = buf[:, :h, :w]
    assert view.stride(1) > w and view.stride(0) > h * view.stride(1)
    rects, found = components.externalRects(view)
    for i in range(3):
        assert ([tuple(r) for r in rects[i].tolist()], int(found[i])) == want[i], i
    labels, counts = prl.connectedComponents(view, 8)
    for i in range(3):
        assert np.array_equal(labels[i].cpu().numpy(), cr.components(pages[i], 8)[0]), i
    assert (buf[:, h:, :] == 255).all() and (buf[:, :, w:] == 255).all()


def test_capacity(prl, cuda_device):
    import torch

    from prlib_amd import components

    pages = [cr.dilate(rnd(70, 90, 0.02, 5), 1), cr.dilate(rnd(70, 90, 0.03, 6), 1)]
    want = [host_answer(prl, m) for m in pages]
    kept = sum(len(r) for r, _f in want)
    assert kept > 4
    batch = torch.from_numpy(np.stack(pages)).to(cuda_device)
    rects, offsets, found, n_kept = components.externalRectsDevice(batch, room=kept - 1)
    assert rects is None and offsets.tolist() == [0, len(want[0][0]), kept] and found.tolist() == [f for _r, f in want]
    assert n_kept.tolist() == [len(r) for r, _f in want]
    L, _capi = components._capi.lib(), components._capi
    room = torch.full((kept, 4), -7, dtype=torch.int32, device=cuda_device)
    off, f, k = np.zeros(3, np.int32), np.zeros(2, np.int32), np.zeros(2, np.int32)
    args = (2, batch.data_ptr(), batch.stride(0), batch.stride(1), 90, 70, room.data_ptr())
    tail = (off.ctypes.data, f.ctypes.data, k.ctypes.data, _capi.stream_on(batch))
    assert L.prl_hip_external_rects_batch_device(*args, kept - 1, *tail) == 0
    assert off[2] == kept and (room == -7).all(), "too little room: the counts alone, the array untouched"
    assert L.prl_hip_external_rects_batch_device(*args, kept, *tail) == 0
    assert [tuple(r) for r in room.cpu().numpy().tolist()] == want[0][0] + want[1][0]
    rects, offsets, _found, _kept = components.externalRectsDevice(batch, room=kept + 5)
    assert rects.shape == (kept, 4)


CHILD = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from prlib_amd import _capi
_capi.use_library(_capi.HOOKS_LIB_PATH)
import torch, prlib_amd as P
from prlib_amd import components
pages = np.load(sys.argv[2])
dev = torch.device("cuda:0")
if sys.argv[3] == "passes":      # the statistics in passes of 100 components; five pages in chunks of two
    import components_ref as cr
    batch = torch.from_numpy(pages).to(dev)
    rects, found = components.externalRects(batch)
    labels, counts, stats = P.connectedComponents(batch, 4, with_stats=True)
    for i, m in enumerate(pages):
        want, want_found = P.externalRects(m)
        assert found[i] == want_found and np.array_equal(rects[i], want), i
        want_labels, want_stats = cr.components(m, 4)
        assert np.array_equal(labels[i].cpu().numpy(), want_labels) and np.array_equal(stats[i].cpu().numpy(), want_stats), i
    np.save(sys.argv[4], np.asarray(found))
else:                            # the whole call on whichever path the environment selects
    mask, found, kept = P.binarizeLocalOtsu(torch.from_numpy(pages).to(dev), with_counts=True)
    np.savez(sys.argv[4], mask=mask.cpu().numpy(), found=found, kept=kept)
print("components child ok")
'''


def run_child(tmp_path, pages, mode, env):
    src, out = str(tmp_path / "pages.npy"), str(tmp_path / ("out_" + mode + (".npy" if mode == "passes" else ".npz")))
    np.save(src, pages)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, src, mode, out], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, **env))
    assert r.returncode == 0 and "components child ok" in r.stdout, r.stdout + r.stderr[-3000:]
    return np.load(out)


def test_statistics_in_passes_and_pages_in_chunks(prl, cuda_device, tmp_path):
    """the hooks build: PRL_HIP_CC_PASS=100 cuts the statistics of a page's thousands of components into passes of 100,
    PRL_HIP_STAGE_CHUNK=2 runs five pages as 2, 2, 1; the child compares with the host scan and the restatement"""
    n = 2 * T + 1
    board = ((np.add.outer(np.arange(n), np.arange(n)) % 2 == 0) * 255).astype(np.uint8)
    pages = np.stack([rnd(n, n, 0.3, 11), board, np.zeros((n, n), np.uint8), cr.dilate(rnd(n, n, 0.05, 12), 1), rnd(n, n, 0.15, 13)])
    found = run_child(tmp_path, pages, "passes", dict(PRL_HIP_CC_PASS="100", PRL_HIP_STAGE_CHUNK="2"))
    assert found.tolist() == [host_answer(prl, m)[1] for m in pages] and found[0] > 200 and found[2] == 0


def composed_pages():
    from prlib_amd import synth

    text = synth.text_page_numpy(150, 200, 31, skew_deg=1.0, shading=0.3)
    crop = np.load(os.path.join(ROOT, "tests", "golden", "scans", "0004.npz"))["gray"][400:550, 300:500]
    return [np.ascontiguousarray(text), np.ascontiguousarray(crop)]


def test_the_composed_call_stage_by_stage(prl, cuda_device):
    """cannyEdgeDetection -> dilate 7 x 7 -> the device rectangles -> rectOtsu equals, byte for byte and in found / kept, the same
    chain with the host externalRects"""
    import torch

    from prlib_amd import components, morphology

    for page in composed_pages():
        assert page.shape == (150, 200)
        gray = torch.from_numpy(page).to(cuda_device)
        edges = prl.cannyEdgeDetection(gray)
        maps = morphology.morphologyEx(edges, morphology.MORPH_DILATE, morphology.MORPH_RECT, 7)
        host_rects, host_found = prl.externalRects(maps.cpu().numpy())
        rects, found = components.externalRects(maps)
        assert found == host_found and np.array_equal(rects, host_rects) and len(rects) > 3
        want = prl.rectOtsu(gray, host_rects)
        got = prl.rectOtsu(gray, rects)
        assert torch.equal(got, want)
        mask, n_found, n_kept = prl.binarizeLocalOtsu(gray, with_counts=True)
        assert (n_found, n_kept) == (host_found, len(host_rects)) and torch.equal(mask, want)


def test_the_whole_call_on_both_paths(prl, cuda_device, tmp_path):
    """binarizeLocalOtsu(with_counts=True) with its rectangles from the host scan (the default: the device path measured no
    faster) and, through the hooks build's PRL_HIP_LO_HOST_RECTS=0, from the device: the same masks and counts on the same pages"""
    import torch

    pages = np.stack(composed_pages())
    device = run_child(tmp_path, pages, "device", dict(PRL_HIP_LO_HOST_RECTS="0"))
    host = run_child(tmp_path, pages, "host", dict(PRL_HIP_LO_HOST_RECTS="1"))
    for key in ("mask", "found", "kept"):
        assert np.array_equal(device[key], host[key]), key
    mask, found, kept = prl.binarizeLocalOtsu(torch.from_numpy(pages).to(cuda_device), with_counts=True)
    assert np.array_equal(mask.cpu().numpy(), host["mask"]) and np.array_equal(found, host["found"]) and np.array_equal(kept, host["kept"])
    assert (host["found"] > 3).all() and 0 < (host["mask"] == 0).mean() < 0.9
