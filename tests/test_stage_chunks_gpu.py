"""The stage entries with more than one chunk of pages.  A second chunk normally needs 65 536 pages or 4 GiB of scratch; the
hooks build's PRL_HIP_STAGE_CHUNK=2 caps every entry's chunk (stage_chunk, prl_internal.h), so five small pages run as 2, 2, 1
and the per-chunk offsets of every entry - pages, thresholds, histograms, tables, page records - are exercised."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_five_pages_in_chunks_of_two(prl, cuda_device):
    """Every batched result is byte for byte the stack of the five single-page calls of the same process (one page is one chunk
    whatever the knob says); median, removeLines, the tone functions, cv::Canny with its two stages, cv::pyrDown and the edge map
    of prl::documentContour (with the channel it chose per page) also equal their restatements.  Thinning, the
    local-variance binarizers, denoise, backgroundNormalization, the mask morphology (fused and large radius) and rotate go
    through their C entries on the strided pages, on inputs whose results are neither constant nor equal between pages.  All outputs are integers: zero differing bytes, no tolerance."""
    code = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from prlib_amd import _capi
_capi.use_library(_capi.HOOKS_LIB_PATH)
import torch, prlib_amd as P, median_ref, lines_ref, tone_ref
from prlib_amd import morphology as M

N, H, W = 5, 80, 64    # the smallest page removeLines takes (its elements are W / 50 and H / 50 long)
rng = np.random.default_rng(9)

def cut(c):
    """five pages out of a larger buffer: page stride and step exceed the dense ones; random content and a few ruled lines"""
    buf = rng.integers(0, 256, size=(N, H + 16, W + 16) + ((c,) if c > 1 else ()), dtype=np.uint8)
    for i in range(N):
        buf[i, 3 + 10 + 7 * i, 5:5 + W] = 10 + i      # a horizontal rule, another row on every page
        buf[i, 3:3 + H, 5 + 20 + 5 * i] = 20 + i      # a vertical rule
        buf[i, 3 + 60 - 3 * i, 5 + 4:5 + W - 4] = 0
    t = torch.from_numpy(buf).cuda()[:, 3:3 + H, 5:5 + W]
    assert t.stride(0) > H * W * c and t.stride(1) > W * c
    return t

gray, colour = cut(1), cut(3)
host = {1: gray.cpu().numpy(), 3: colour.cpu().numpy()}
checked = []

def same(name, batched, singles, ref=None):
    """batched: N x ...; singles: the N results of the one-page calls; ref: the N pages of a restatement"""
    got = batched.cpu().numpy()
    want = np.stack([s.cpu().numpy() for s in singles])
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape)
    assert np.array_equal(got, want), (name, "batched != single pages", int((got != want).sum()))
    if ref is not None:
        assert np.array_equal(got, np.stack(ref)), (name, "!= restatement", int((got != np.stack(ref)).sum()))
    checked.append(name)

def each(name, fn, channels, ref=None):
    for c in channels:
        pages = gray if c == 1 else colour
        same("%s c=%d" % (name, c), fn(pages), [fn(pages[i]) for i in range(N)], None if ref is None else [ref(p) for p in host[c]])

each("denoiseSaltPepper", lambda p: P.denoiseSaltPepper(p, 3, 2), (1, 3), lambda p: median_ref.denoise_salt_pepper(p, 3, 2))
each("binarizeNativeAdaptive", lambda p: P.binarizeNativeAdaptive(p), (1, 3))
each("binarizeAT", lambda p: P.binarizeAT(p, 5, 255, 19, 9), (3,))
each("morphologyEx", lambda p: P.morphologyEx(p, M.MORPH_OPEN, M.MORPH_ELLIPSE, 5), (1, 3))
each("correctNUIL", lambda p: P.correctNUIL(p, 7), (1, 3))
each("removeLines", lambda p: P.removeLines(p), (1, 3), lines_ref.remove_lines)
each("gammaCorrection", lambda p: P.gammaCorrection(p, 1.2, 0.8), (1, 3), lambda p: tone_ref.gamma_model(p, 1.2, 0.8))
each("simpleWhiteBalance", lambda p: P.simpleWhiteBalance(p, 0.01), (3,), lambda p: tone_ref.swb_model(p, 0.01))
each("grayWorld p=1", lambda p: P.grayWorldWhiteBalance(p, 1, False), (3,), lambda p: tone_ref.gw_model(p, 1.0, False))   # device tables
each("grayWorld p=2", lambda p: P.grayWorldWhiteBalance(p, 2, False), (3,), lambda p: tone_ref.gw_model(p, 2.0, False))   # host tables
each("cleanBackgroundToWhite", lambda p: P.cleanBackgroundToWhite(p), (1, 3))
each("histogram", lambda p: P.histogram(p), (1, 3), lambda p: tone_ref.histograms(p).astype(np.int32))
each("binarizeMokji", lambda p: P.binarizeMokji(p), (1, 3))
each("mokjiThresholds", lambda p: P.mokjiThresholds(p), (1, 3))

import edges_ref
from prlib_amd import edges as E
each("canny", lambda p: E.canny(p, 25, 50), (1,), lambda p: edges_ref.canny(p, 25.0, 50.0))
each("canny_classes", lambda p: E.canny_classes(p, 25, 50), (1,), lambda p: edges_ref.canny_classes(p, 25.0, 50.0))
each("edge_link", lambda p: E.edge_link(E.canny_classes(p, 25, 50)), (1,), lambda p: edges_ref.edge_link(edges_ref.canny_classes(p, 25.0, 50.0)))
each("pyr_down", lambda p: E.pyr_down(p, 1), (1, 3), lambda p: edges_ref.pyr_down(p, 1))

# document_edges: 520 / 2 >= 256, the smallest page that takes a pyramid level (the map is 260 x 20).  Smooth blobs, others on
# every page, under a little noise; on the colour pages channel i % 3 has the full contrast, the others a quarter of it
DW, DH = 520, 40
yy, xx = np.mgrid[0:DH, 0:DW]
for c in (1, 3):
    buf = np.zeros((N, DH + 8, DW + 24) + ((c,) if c > 1 else ()), np.uint8)
    for i in range(N):
        g = (128 + 100 * np.sin(xx / (9.0 + 2 * i)) * np.cos(yy / (5.0 + i)) + rng.integers(-6, 7, size=(DH, DW))).astype(np.uint8)
        g[8 + 3 * i:20 + 3 * i, 40 + 50 * i:200 + 50 * i] = 250 - 40 * i
        buf[i, 2:2 + DH, 7:7 + DW] = g if c == 1 else np.stack([g if k == i % 3 else (g >> 2) + 90 for k in range(3)], axis=2)
    pages = torch.from_numpy(buf).cuda()[:, 2:2 + DH, 7:7 + DW]
    assert pages.stride(0) > DH * DW * c and pages.stride(1) > DW * c
    hp = pages.cpu().numpy()
    want = [edges_ref.document_edges(p) for p in hp]
    if c == 3:
        chosen = [edges_ref.most_informative_channel(edges_ref.pyr_down(p, 1)) for p in hp]
        assert chosen == [w[1] for w in want] and len(set(chosen)) > 1, chosen
    maps, channels = E.document_edges(pages)
    singles = [E.document_edges(pages[i]) for i in range(N)]
    assert maps.shape == (N, 20, 260) and len({m.cpu().numpy().tobytes() for m, _ in singles}) == N
    same("document_edges c=%d" % c, maps, [m for m, _ in singles], [w[0] for w in want])
    assert channels.dtype == np.int32 and list(channels) == [ch for _, ch in singles] == [w[1] for w in want], (c, channels)

for c in (1, 3):   # a table set per page
    pages = gray if c == 1 else colour
    tables =rng.integers(0, 256, size=(N, c, 256), dtype=np.uint8)
    td = torch.from_numpy(tables).cuda()
    same("lut c=%d" % c, P.lut(pages, td), [P.lut(pages[i], td[i]) for i in range(N)], [tone_ref.apply_luts(host[c][i], tables[i]) for i in range(N)])

quads = np.array([[3 + i, 4, 55 + i, 6 + i, 58, 70 - i, 5, 66 + i] for i in range(N)], dtype=np.int32)   # another quad on every page
for c in (1, 3):
    pages = gray if c == 1 else colour
    got = P.warp_crop(pages, quads)
    sizes = set()
    for i in range(N):
        one = P.warp_crop(pages[i:i + 1], quads[i])[0]
        assert got[i].shape == one.shape and torch.equal(got[i], one), ("warp_crop", c, i)
        sizes.add(tuple(one.shape[:2]))
    assert len(sizes) > 1   # the pages' results differ in size
    checked.append("warp_crop c=%d" % c)

# The older entries, straight through the C ABI (some of their Python wrappers take dense tensors only): thinning, the
# local-variance binarizers, denoise, backgroundNormalization, the mask morphology and rotate.
L = _capi.lib()

def entry(fn, head, pages, out_channels):
    """fn(*head(n), src, page stride, step, w, h, dst, page stride, step, stream) on n strided pages -> n x H x W x out_channels"""
    n, h, w = pages.shape[:3]
    out = torch.zeros((n, h, w, out_channels), dtype=torch.uint8, device="cuda")
    _capi.check(fn(*head(n), pages.data_ptr(), pages.stride(0), pages.stride(1), w, h, out.data_ptr(), out.stride(0), out.stride(1),
                   _capi.stream_on(pages)))
    return out

def each_entry(name, fn, head, pages, out_channels, varied=True):
    """varied: no page's result is constant and no two pages' results are equal, so a chunk that read another page, or another
    page's thresholds or work plane, cannot give the same bytes"""
    assert pages.stride(0) > H * pages.stride(1) and pages.stride(1) > W * (pages.shape[3] if pages.dim() == 4 else 1)
    singles = [entry(fn, head, pages[i:i + 1], out_channels)[0] for i in range(N)]
    if varied:
        assert all(int(r.min()) != int(r.max()) for r in singles), (name, "a constant result")
        assert len({r.cpu().numpy().tobytes() for r in singles}) == N, (name, "two pages with the same result")
    same(name, entry(fn, head, pages, out_channels), singles)

def recut(t):
    """the same pages inside a larger buffer again"""
    big = torch.zeros((N, H + 16, W + 16) + tuple(t.shape[3:]), dtype=torch.uint8, device="cuda")
    big[:, 3:3 + H, 5:5 + W] = t
    return big[:, 3:3 + H, 5:5 + W]

colour4 = cut(4)
black_white = recut(torch.where(gray > 127, 255, 0).to(torch.uint8))   # the rules of cut() are black: another skeleton on every page
for c, pages in ((3, colour), (4, colour4)):
    each_entry("denoise c=%d" % c, L.prl_hip_denoise_batch_device, lambda n: (n, c, 10.0), pages, c)
for method, name in ((0, "thinZhangSuen"), (1, "thinGuoHall")):
    each_entry(name, L.prl_hip_thin_batch_device, lambda n: (method, n), black_white, 1)
each_entry("binarizeByLocalVariances", L.prl_hip_binarize_lv_batch_device, lambda n: (n, 1, 0.125, 25, 2.0), colour, 1)
# (on the noise of cut() every pixel passes the unfiltered variant's two tests: five white masks, which show a wrong destination only)
each_entry("binarizeByLocalVariancesWithoutFilters", L.prl_hip_binarize_lv_batch_device, lambda n: (n, 0, 0.125, 10, 2.0), colour, 1, varied=False)
import lv_ref
text = recut(torch.from_numpy(np.stack([lv_ref.colour(H, W, 40 + i) for i in range(N)])).cuda())   # smooth paper and strokes: masks of both values
each_entry("binarizeByLocalVariances, text", L.prl_hip_binarize_lv_batch_device, lambda n: (n, 1, 0.125, 25, 2.0), text, 1)
each_entry("binarizeByLocalVariancesWithoutFilters, text", L.prl_hip_binarize_lv_batch_device, lambda n: (n, 0, 0.125, 10, 2.0), text, 1)
for c, pages in ((1, gray), (3, colour)):
    each_entry("backgroundNormalization c=%d" % c, L.prl_hip_bgnorm_batch_device, lambda n: (n, c), pages, c)

def blobs():
    """masks that are mostly 0, another on every page: two 20 x 30 rectangles 2, 6, ... 18 columns apart (a closing of radius 2 or 9
    bridges some of the gaps), a hole, squares of 3 and 7 and a rule 1 ... 5 rows thick (an opening of radius 9 removes them)"""
    m = np.zeros((N, H, W), np.uint8)
    for i in range(N):
        gap = 2 + 4 * i
        m[i, 4 + 2 * i:34 + 2 * i, 2:22] = 255
        m[i, 4 + 2 * i:34 + 2 * i, 22 + gap:42 + gap] = 255
        m[i, 10 + 2 * i:11 + 3 * i, 8:9 + i] = 0
        m[i, 50 + i:53 + i, 5 + 9 * i:8 + 9 * i] = 255
        m[i, 58:65, 6 + 8 * i:13 + 8 * i] = 255
        m[i, 70:71 + i, 4:60] = 255
    return recut(torch.from_numpy(m).cuda())

masks = blobs()
# the fused kernels (no workspace); the large-radius path, whose tmp plane restarts at each chunk, closing and opening
for iterations in (2, 9, -9):
    each_entry("morph %d" % iterations, L.prl_hip_morph_batch_device, lambda n: (iterations, n), masks, 1)

from prlib_amd.deskew import rotate_out_size
angles = np.array([0.0, 90.0, 7.5, -13.0, 181.0])

def rotate(pages, ang):
    n, h, w = pages.shape[:3]
    c = pages.shape[3] if pages.dim() == 4 else 1
    sizes = [rotate_out_size(w, h, a) for a in ang]
    buf = torch.zeros((n, max(s[1] for s in sizes), max(s[0] for s in sizes), c), dtype=torch.uint8, device="cuda")
    _capi.check(L.prl_hip_rotate_batch_device(n, c, ang.ctypes.data, pages.data_ptr(), pages.stride(0), pages.stride(1), w, h,
                                              buf.data_ptr(), buf.stride(0), buf.stride(1), _capi.stream_on(pages)))
    return [buf[i, :oh, :ow] for i, (ow, oh) in enumerate(sizes)]

for c, pages in ((1, gray), (3, colour)):
    got = rotate(pages, angles)
    for i in range(N):
        one = rotate(pages[i:i + 1], angles[i:i + 1])[0]
        assert got[i].shape == one.shape and torch.equal(got[i], one), ("rotate", c, i, int((got[i] != one).sum()))
    assert len(set(tuple(g.shape[:2]) for g in got)) > 1   # the pages' results differ in size
    checked.append("rotate c=%d" % c)

torch.cuda.synchronize()
print("stage chunks ok: %d comparisons" % len(checked))
'''
    env = dict(os.environ, PRL_HIP_STAGE_CHUNK="2")
    r = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "stage chunks ok" in r.stdout, r.stdout + r.stderr[-3000:]
