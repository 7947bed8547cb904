"""GPU parity of prl::binarizeByLocalVariances / ...WithoutFilters against the CPU oracle.

WithoutFilters is float32 arithmetic on integer-valued sums with a fixed operation order: bit-exact.  The filtered
variant goes through float32 log / exp (cv::log / cv::exp in the reference, logf / expf in the oracle, the device's logf
/ expf here): last-bit differences move a pixel of the 8-bit maps across a rounding boundary now and then, so the
stated tolerance is <= 1e-3 of the pixels differing (measured: ~1e-5)."""
import numpy as np
import pytest

from prlib_amd import synth

pytestmark = pytest.mark.gpu
TOL = 1e-3


def _colour(h, w, seed, skew=0.0, shading=0.2):
    g = synth.text_page_numpy(h, w, seed, skew_deg=skew, shading=shading)
    rng = np.random.default_rng(seed)
    return np.clip(g[..., None].astype(np.int32) + rng.normal(0, 5, (h, w, 3)), 0, 255).round().astype(np.uint8)


@pytest.mark.parametrize("shape", [(200, 260), (97, 131), (33, 40), (8, 32), (1, 1), (257, 65), (530, 777), (18, 3000)])
def test_without_filters_is_bit_exact(prl, oracle, cuda_device, shape):
    import torch

    pages = np.stack([_colour(shape[0], shape[1], s) for s in (1, 2)])
    for coeff, mv in ((0.125, 10), (0.5, 25), (0.0, 0)):
        got = prl.binarizeByLocalVariancesWithoutFilters(torch.from_numpy(pages).to(cuda_device), coeff, mv).cpu().numpy()
        for i in range(2):
            want = oracle.binarize_lv_nofilters(pages[i], coeff, mv)
            assert np.array_equal(got[i], want), (shape, coeff, mv, int((got[i] != want).sum()))


@pytest.mark.parametrize("shape", [(200, 260), (97, 131), (64, 48), (300, 411), (140, 700)])
def test_with_filters_within_tolerance(prl, oracle, cuda_device, shape):
    import torch

    pages = np.stack([_colour(shape[0], shape[1], s, skew=1.0) for s in (3, 4)])
    for coeff, mv, gamma in ((0.125, 25, 2.0), (0.3, 10, 2.0), (0.125, 25, 1.5)):
        got = prl.binarizeByLocalVariances(torch.from_numpy(pages).to(cuda_device), coeff, mv, gamma).cpu().numpy()
        for i in range(2):
            want = oracle.binarize_lv(pages[i], coeff, mv, gamma)
            bad = int((got[i] != want).sum())
            assert bad <= max(2, TOL * want.size), (shape, coeff, mv, gamma, bad, want.size)
            assert set(np.unique(got[i])) <= {0, 255}


def test_lv_flat_noise_host_entry_and_errors(prl, oracle, cuda_device):
    import torch

    flat = np.full((50, 60, 3), 120, np.uint8)          # variance 0.01 everywhere: nothing exceeds 10 -> all black
    assert prl.binarizeByLocalVariances(torch.from_numpy(flat).to(cuda_device)).max().item() == 0
    assert prl.binarizeByLocalVariancesWithoutFilters(torch.from_numpy(flat).to(cuda_device)).max().item() == 0
    rng = np.random.default_rng(9)
    noise = rng.integers(0, 256, (80, 90, 3), dtype=np.uint8)
    assert np.array_equal(prl.binarizeByLocalVariancesWithoutFilters(torch.from_numpy(noise).to(cuda_device)).cpu().numpy(),
                          oracle.binarize_lv_nofilters(noise))
    page = _colour(120, 150, 5)
    assert np.array_equal(prl.binarizeByLocalVariancesWithoutFilters(page), oracle.binarize_lv_nofilters(page))   # host entry
    got = prl.binarizeByLocalVariances(page)
    assert int((got != oracle.binarize_lv(page)).sum()) <= max(2, TOL * got.size)
    with pytest.raises(TypeError):
        prl.binarizeByLocalVariances(torch.zeros((10, 10), dtype=torch.uint8, device=cuda_device))
    with pytest.raises(ValueError):
        prl.binarizeByLocalVariances(np.zeros((0, 0, 3), np.uint8))


# ---- the filtered variant stage by stage: prl_hip_internal_lv_maps of the test-hooks build ---------------------------------------------
# The filtered function is cut where its floating point ends (tests/lv_ref.py).  The hooks entry runs the product entry's own launch
# sequence and hands out what pass 2 left in scratch: the 8-bit maps G and N and the per-page constants.  Everything before them is
# float32 with a fixed order on integer-valued sums and is held exactly; everything after them is integer and is held exactly on
# the device's own maps; G and N themselves are held to the nearest integer of their float64 values.
import lv_ref as lr  # noqa: E402

# h x w: around the 64 x 16 variance tile, the 64 x 32 final tile, the runs of eight rows, and the 131 / 132 columns and 34 rows
# from which a tile first takes the dword staging path
MAPS_SHAPES = [(1, 1), (1, 40), (40, 1), (8, 32), (15, 15), (16, 64), (17, 65), (31, 63), (32, 64), (33, 129), (47, 131), (70, 200), (97, 131)]
MAPS_PARAMS = [(0.125, 25, 2.0), (0.3, 10, 1.5), (0.5, 0, 3.0), (0.125, 126, 1.0)]   # (coeff, minResultVariance, gamma)
MAPS_EPS = 0.01          # on top of the 0.5 of rounding to the nearest integer; derived in the transcendental test's docstring
MAPS_MIN_RANGE = 15.0    # of the log map: what the derivation of MAPS_EPS assumes


def _maps_page(h, w, seed):
    """_colour's page.  The text generator keeps its ink off a margin, which is all of a page one pixel thin: such a page is noisy
    paper with a log-map range near 10, so it gets a flat run of ink drawn in (variance 0.01 inside, an edge of 195 levels)."""
    p = lr.colour(h, w, seed, skew=1.0)
    if min(h, w) == 1 and h * w > 1:
        line = p.reshape(-1, 3)
        line[len(line) // 4:len(line) // 4 + 8] = 30
    return p


def _noise_page(h, w, seed):
    """uniform noise whose amplitude grows from 1/256 of full scale at the left edge to full scale at the right one (uniform noise
    of one amplitude has a log-map range near 8)"""
    rng = np.random.default_rng(seed)
    u = rng.integers(0, 256, (h, w, 3)).astype(np.float64) - 127.5
    gain = np.exp(np.linspace(np.log(1 / 256), 0.0, w))[None, :, None]
    return np.clip(np.rint(127.5 + u * gain), 0, 255).astype(np.uint8)


def maps_batches():
    """[(name, pages n x h x w x 3)]: three pages per shape, the batch of three very different pages, three flat pages"""
    out = [(f"{h}x{w}", np.stack([_maps_page(h, w, s) for s in (11, 12, 13)])) for h, w in MAPS_SHAPES]
    text = lr.colour(70, 200, 21, skew=1.0, shading=0.0)
    quarter = np.rint(128.0 + (text.astype(np.float64) - 128.0) / 4).astype(np.uint8)
    out.append(("mixed", np.stack([text, quarter, _noise_page(70, 200, 22)])))
    out.append(("flat", np.stack([np.full((17, 65, 3), v, np.uint8) for v in (0, 120, 255)])))
    return out


def maps_row(name, k, page, params, mask, G, N, consts):
    """What the tests assert on, for one page of one call of the hooks entry (runs in the child)."""
    coeff, mv, gamma = params
    var = lr.variance_map(page)
    thr = lr.thresholds(var, coeff)
    r1, r2 = lr.r1_r2(var, thr)
    keep = r1 & r2
    g64, n64, lmin, lmax, lmean = lr.maps64(var, gamma)
    row = dict(case=name, page=k, h=page.shape[0], w=page.shape[1], coeff=coeff, mv=mv, gamma=gamma, range=lmax - lmin,
               keep=int(keep.sum()), ones=int((mask == 255).sum()), values=sorted(int(v) for v in np.unique(mask)),
               mask_bad=int((mask != lr.final_from_maps(G, N, mv)).sum()),
               n255_bad=int(((N == 255) != ~keep).sum()),
               thr_dev=[int(v) for v in consts[:3].view(np.uint32)], thr_ref=[int(v) for v in thr.view(np.uint32)],
               g_nonzero=int((G != 0).sum()), n_not255=int((N != 255).sum()), pad=[float(consts[6]), float(consts[7])])
    if lmax > lmin:
        ga, gb, lm = (float(np.float64(v)) for v in consts[3:6])
        row.update(g_err=float(np.abs(G.astype(np.float64) - g64).max()),
                   n_err=float(np.abs(N.astype(np.float64) - n64)[keep].max()) if keep.any() else 0.0,
                   lmean_err=abs(lm - lmean), lmin_err=abs(-gb / ga - lmin), lmax_err=abs((1.0 - gb) / ga - lmax),
                   ga_rel=abs(ga * (lmax - lmin) - 1.0))
    return row


_MAPS_CHILD = r'''
import ctypes as C, json, sys
import numpy as np, torch
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from prlib_amd import _capi
_capi.use_library(_capi.HOOKS_LIB_PATH)
import test_lv_gpu as T
L = _capi.lib()
vp, sz, i, d = C.c_void_p, C.c_size_t, C.c_int, C.c_double
L.prl_hip_internal_lv_maps.argtypes = [i, d, i, d, vp, sz, sz, i, i, vp, sz, sz, vp, vp, vp, vp]
dev = torch.device("cuda:0")
_capi.check(L.prl_hip_set_device(0))
stream = torch.cuda.current_stream(dev).cuda_stream
rows = []
for name, pages in T.maps_batches():
    n, h, w = pages.shape[:3]
    src = torch.from_numpy(pages).to(dev)
    for params in T.MAPS_PARAMS:
        coeff, mv, gamma = params
        dst = torch.full((n, h, w), 9, dtype=torch.uint8, device=dev)
        G = torch.full((n, h, w), 3, dtype=torch.uint8, device=dev)
        N = torch.full((n, h, w), 5, dtype=torch.uint8, device=dev)
        consts = torch.full((n, 8), -1.0, dtype=torch.float32, device=dev)
        _capi.check(L.prl_hip_internal_lv_maps(n, coeff, mv, gamma, src.data_ptr(), src.stride(0), src.stride(1), w, h, dst.data_ptr(),
                                               dst.stride(0), dst.stride(1), G.data_ptr(), N.data_ptr(), consts.data_ptr(), stream))
        torch.cuda.synchronize()
        dst, G, N, consts = (t.cpu().numpy() for t in (dst, G, N, consts))
        for k in range(n):
            rows.append(T.maps_row(name, k, pages[k], params, dst[k], G[k], N[k], consts[k]))
# more than one chunk of pages, or a missing output, is an argument error of the entry
one = torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device=dev)
out = torch.zeros((1, 4, 4), dtype=torch.uint8, device=dev)
f8 = torch.zeros((1, 8), dtype=torch.float32, device=dev)
errs = [L.prl_hip_internal_lv_maps(16385, 0.125, 25, 2.0, one.data_ptr(), 0, 12, 4, 4, out.data_ptr(), 0, 4, out.data_ptr(), out.data_ptr(),
                                   f8.data_ptr(), stream),
        L.prl_hip_internal_lv_maps(1, 0.125, 25, 2.0, one.data_ptr(), 48, 12, 4, 4, out.data_ptr(), 16, 4, None, out.data_ptr(),
                                   f8.data_ptr(), stream)]
torch.cuda.synchronize()
print("ROWS " + json.dumps(dict(rows=rows, errs=errs)))
'''
_maps_result = []


def _maps_child():
    """The rows of the one child of _MAPS_CHILD (run once per session).  A child that died (signal, abort, GPU fault, time limit) fails
    its test and every later one without another process being started."""
    import json
    import os
    import subprocess
    import sys
    import time

    if _maps_result:
        assert not isinstance(_maps_result[0], str), f"the child failed before and is not started again: {_maps_result[0]}"
        return _maps_result[0]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = _MAPS_CHILD % dict(root=root, tests=os.path.join(root, "tests"))
    _maps_result.append("did not finish")
    t0 = time.time()
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    print(f"lv maps child: {time.time() - t0:.1f} s")
    if r.returncode != 0 or "illegal memory access" in r.stderr:
        _maps_result[0] = f"exit {r.returncode}: {r.stderr[-2000:]}"
    assert r.returncode == 0 and "illegal memory access" not in r.stderr, (r.returncode, r.stdout[-2000:] + r.stderr[-2000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("ROWS ")]
    assert lines, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(lines[0][5:])
    assert len(res["rows"]) == (len(MAPS_SHAPES) + 2) * len(MAPS_PARAMS) * 3
    _maps_result[0] = res
    return res


def _live(rows):
    """the pages of two pixels or more that are not flat"""
    return [x for x in rows if x["case"] not in ("flat", "1x1")]


def test_maps_integer_side_is_exact(prl, cuda_device):
    """k_lv_final (the 15 x 15 sliding box and its replicate border, the runs of eight, the rounding of the mean, the subtraction of
    N) on the device's own maps: the mask the entry wrote equals lv_ref.final_from_maps(G_dev, N_dev, mv) on every byte."""
    rows = _live(_maps_child()["rows"])
    assert len(rows) == (len(MAPS_SHAPES) - 1 + 1) * len(MAPS_PARAMS) * 3
    for x in rows:
        assert x["mask_bad"] == 0 and set(x["values"]) <= {0, 255}, x
    for case in ("8x32", "70x200", "97x131", "mixed"):      # (not vacuous: both values occur)
        for x in rows:
            if x["case"] == case:
                assert 0 < x["ones"] < x["h"] * x["w"], x


def test_maps_float32_side_is_exact(prl, cuda_device):
    """The variance tile on both staging paths, the ring of the contrast filter, the page extrema and the per-page thresholds:
    (N_dev == 255) equals ~(result1 & result2) of lv_ref on every pixel, and the three thresholds equal lv_ref.thresholds bit for
    bit - in the batch of three very different pages too, where a neighbour's constants would show."""
    rows = _live(_maps_child()["rows"])
    for x in rows:
        assert x["n255_bad"] == 0, x
        assert x["thr_dev"] == x["thr_ref"], x
        assert x["pad"] == [0.0, 0.0], x
    mixed = [x for x in rows if x["case"] == "mixed"]
    assert len({tuple(x["thr_ref"]) for x in mixed}) == 3 * len({p[0] for p in MAPS_PARAMS})
    for x in rows:
        if x["h"] * x["w"] >= 200:
            assert 0 < x["keep"] < x["h"] * x["w"], x


def test_maps_transcendental_maps_to_the_nearest_integer(prl, cuda_device):
    """|G_dev - g64| <= 0.5 + eps on every pixel and |N_dev - n64| <= 0.5 + eps on every pixel with result1 & result2, g64 and n64 the
    float64 maps of lv_ref.maps64, eps = 0.01.  Derived, not measured: logf within 2 ulp on |log v| <= 9.7 plus two float32 additions
    on |l| <= 29 give dl < 1e-5; with a log-map range of at least 15 (asserted per page on the float64 values) and t <= 1,
    dt < 3e-6; 255 * gamma * dt < 3e-3 for gamma <= 3; 127 * 0.61 * 2 dl < 2e-3.  The CPU's float32 path of the same pages stays
    below 2.5e-4 on both maps beyond the 0.5 of rounding.  The device's largest deviations are printed; on an MI355X they were
    0.5 + 3.2e-5 on G and 0.5 + 1.3e-5 on N, at a smallest log-map range of 18.19 (profiles/r02/lv_maps_deviation.txt)."""
    rows = _live(_maps_child()["rows"])
    g = max(x["g_err"] for x in rows)
    n = max(x["n_err"] for x in rows)
    print(f"largest |G_dev - g64| = 0.5 + {g - 0.5:.3e}, largest |N_dev - n64| = 0.5 + {n - 0.5:.3e}, "
          f"smallest log-map range {min(x['range'] for x in rows):.2f}")
    for x in rows:
        assert x["range"] >= MAPS_MIN_RANGE, x
        assert x["g_err"] <= 0.5 + MAPS_EPS, x
        assert x["n_err"] <= 0.5 + MAPS_EPS, x


def test_maps_constants(prl, cuda_device):
    """lmean, and lmin / lmax recovered as -gb / ga and (1 - gb) / ga, within 2e-5 of the float64 values (the dl bound above with a
    factor of two); ga within 1e-5 relative of 1 / range."""
    rows = _live(_maps_child()["rows"])
    print("largest deviations: lmean %.2e, lmin %.2e, lmax %.2e, ga relative %.2e" % tuple(
        max(x[k] for x in rows) for k in ("lmean_err", "lmin_err", "lmax_err", "ga_rel")))
    for x in rows:
        assert x["lmean_err"] <= 2e-5 and x["lmin_err"] <= 2e-5 and x["lmax_err"] <= 2e-5, x
        assert x["ga_rel"] <= 1e-5, x


def test_maps_of_flat_pages_and_argument_errors(prl, cuda_device):
    """A flat page and the 1 x 1 page have a constant log map (0 / 0 in the scale): G == 0 and N == 255 everywhere, an all-zero
    mask.  The entry refuses more than one chunk of pages and a missing output."""
    res = _maps_child()
    rows = [x for x in res["rows"] if x["case"] in ("flat", "1x1")]
    assert len(rows) == 2 * len(MAPS_PARAMS) * 3
    for x in rows:
        assert x["range"] == 0.0 and x["g_nonzero"] == 0 and x["n_not255"] == 0 and x["ones"] == 0 and x["values"] == [0], x
        assert x["mask_bad"] == 0 and x["thr_dev"] == x["thr_ref"] == [0, 0, 0], x
    assert res["errs"] == [5, 5]     # PRL_ERR_BAD_ARG


# ---- the product library: views, several tiles per workgroup, page chunks, the height limit ------------------------------------------

@pytest.mark.parametrize("off", [1, 2, 3])
def test_views_of_both_variants(prl, oracle, cuda_device, off):
    """Pages that are views of a larger tensor (src_step > 3 * width, a page base 3 * off bytes past a dword boundary under the 4-byte
    staging loads, random bytes all round) into a view of a tensor filled with 7 (dst_step > width): the same bytes as the contiguous
    page gives, and nothing written outside the view.  70 x 200 has variance tiles on both staging paths."""
    import torch

    h, w, n = 70, 200, 2
    rng = np.random.default_rng(30 + off)
    big = rng.integers(0, 256, (n, h + 3, w + 8, 3), dtype=np.uint8)
    pages = np.stack([lr.colour(h, w, 31 + i, skew=1.0) for i in range(n)])
    big[:, 1:h + 1, off:off + w, :] = pages
    tbig = torch.from_numpy(big).to(cuda_device)
    view = tbig[:, 1:h + 1, off:off + w, :]
    assert (view.data_ptr() - tbig.data_ptr()) % 4 == (3 * off) % 4 and tbig.data_ptr() % 4 == 0 and view.stride(1) == 3 * (w + 8)
    contiguous = torch.from_numpy(pages).to(cuda_device)
    for with_filters in (False, True):
        obig = torch.full((n, h + 2, w + 5), 7, dtype=torch.uint8, device=cuda_device)
        out = obig[:, 1:h + 1, 2:2 + w]
        if with_filters:
            got = prl.binarizeByLocalVariances(view, 0.125, 25, 2.0, out=out)
            want = prl.binarizeByLocalVariances(contiguous, 0.125, 25, 2.0).cpu().numpy()
        else:
            got = prl.binarizeByLocalVariancesWithoutFilters(view, 0.125, 10, out=out)
            want = np.stack([oracle.binarize_lv_nofilters(p, 0.125, 10) for p in pages])
        assert got.data_ptr() == out.data_ptr()
        res = obig.cpu().numpy()
        assert np.array_equal(res[:, 1:h + 1, 2:2 + w], want), (off, with_filters, int((res[:, 1:h + 1, 2:2 + w] != want).sum()))
        assert 0 < int((want == 255).sum()) < want.size
        res[:, 1:h + 1, 2:2 + w] = 7
        assert (res == 7).all(), (off, with_filters, int((res != 7).sum()))
    assert np.array_equal(tbig.cpu().numpy(), big)


TILE_H, TILE_W = 70, 130     # 3 x 5 = 15 variance tiles of 64 x 16


def _tile_pages(n, seed=40):
    """Low-contrast texture (uniform noise of +-10 levels: variance near 37, contrast sums near 440) plus one 3 x 3 checker of 0 / 255
    (variance 16056: the page's maximum, which sets the thresholds to about 1000).  The spot's centre lies in tile (page index
    mod 15); in the two-column tiles of the right edge it is column 128."""
    rng = np.random.default_rng(seed)
    pages = (128 + rng.integers(-10, 11, (n, TILE_H, TILE_W, 3))).astype(np.uint8)
    plain = pages.copy()
    yy, xx = np.mgrid[0:3, 0:3]
    spot = np.where((yy + xx) % 2 == 0, 255, 0).astype(np.uint8)[:, :, None]
    for i in range(n):
        t = i % 15
        cx, cy = min((t % 3) * 64 + 30, TILE_W - 2), min((t // 3) * 16 + 6, TILE_H - 2)
        pages[i, cy - 1:cy + 2, cx - 1:cx + 2, :] = spot
    return pages, plain


def test_several_tiles_per_workgroup(prl, oracle, cuda_device):
    """1100 pages of 70 x 130: 15 variance tiles per page against max(8, 8192 / 1100) = 8 workgroups, so k_lv_stats walks its
    grid-stride loop.  First, on the CPU: removing the spot changes the oracle's mask by at least 50 pixels, and so does taking the
    thresholds from every pixel but those of the spot's tile - a tile the loop skipped cannot go unseen."""
    import torch

    n = 1100
    pages, plain = _tile_pages(n)
    for i in range(15):
        want = oracle.binarize_lv_nofilters(pages[i], 0.125, 10)
        assert int((want != oracle.binarize_lv_nofilters(plain[i], 0.125, 10)).sum()) >= 50, i
        var = lr.variance_map(pages[i])
        assert np.array_equal(lr.nofilters_from(var, lr.thresholds(var, 0.125), 10), want)
        outside = np.ones((TILE_H, TILE_W), bool)
        outside[(i // 3) * 16:(i // 3) * 16 + 16, (i % 3) * 64:(i % 3) * 64 + 64] = False
        skipped = lr.nofilters_from(var, lr.thresholds(var[outside], 0.125), 10)
        assert int((skipped != want).sum()) >= 50, (i, int((skipped != want).sum()))
    got = prl.binarizeByLocalVariancesWithoutFilters(torch.from_numpy(pages).to(cuda_device), 0.125, 10).cpu().numpy()
    bad = [i for i in range(n) if not np.array_equal(got[i], oracle.binarize_lv_nofilters(pages[i], 0.125, 10))]
    assert not bad, (len(bad), bad[:20])


CHUNK_PAGES = (0, 1, 16383, 16384, 16399)


def _chunk_pages(n=16400, seed=50):
    """5 x 6 pages of texture whose amplitude differs from page to page.  The first page of the second chunk (16384) is texture of
    +-10 levels with one pixel of 255 in its corner: its own thresholds (near 1000 at coeff = 0.5) leave the texture black, those of
    the last pages of either chunk (texture of +-6 levels alone) would turn most of it white."""
    rng = np.random.default_rng(seed)
    amp = rng.integers(4, 40, n)
    amp[[16383, 16384, 16399]] = 6, 10, 6
    pages = np.clip(128 + rng.integers(-1000, 1001, (n, 5, 6, 3)) * amp[:, None, None, None] // 1000, 0, 255).astype(np.uint8)
    pages[16384, 0, 0, :] = 255
    return pages


CHUNK_COEFF = 0.5


def test_page_chunks(prl, oracle, cuda_device):
    """16400 pages of 5 x 6 go in two chunks (16384 + 16), the second through the first one's scratch.  WithoutFilters equals the
    oracle, the filtered variant the same page run alone, on the pages at both ends of both chunks.  On the CPU first: page 16384
    under the thresholds of page 16383 or 16399 is another mask."""
    import torch

    pages = _chunk_pages()
    var = lr.variance_map(pages[16384])
    own = lr.nofilters_from(var, lr.thresholds(var, CHUNK_COEFF), 10)
    assert 0 < int((own == 255).sum()) < own.size
    for other in (16383, 16399):
        leaked = lr.nofilters_from(var, lr.thresholds(lr.variance_map(pages[other]), CHUNK_COEFF), 10)
        assert int((leaked != own).sum()) >= 10, other
    t = torch.from_numpy(pages).to(cuda_device)
    got = prl.binarizeByLocalVariancesWithoutFilters(t, CHUNK_COEFF, 10).cpu().numpy()
    for i in CHUNK_PAGES:
        want = oracle.binarize_lv_nofilters(pages[i], CHUNK_COEFF, 10)
        assert np.array_equal(got[i], want), (i, got[i], want)
    got = prl.binarizeByLocalVariances(t, CHUNK_COEFF, 0, 2.0).cpu().numpy()
    ones = 0
    for i in CHUNK_PAGES:
        alone = prl.binarizeByLocalVariances(t[i:i + 1].clone(), CHUNK_COEFF, 0, 2.0).cpu().numpy()[0]
        assert np.array_equal(got[i], alone), (i, got[i], alone)
        ones += int((alone == 255).sum())
    assert ones > 0


def test_height_limit(prl, oracle, cuda_device):
    """(height + 15) / 16 > 65535 is refused: 1048560 x 1 is the tallest page (65535 tile rows), 1048561 x 1 is PRL_ERR_BAD_ARG."""
    import torch

    from prlib_amd import _capi

    h = 1048560
    rng = np.random.default_rng(60)
    col = (128 + rng.integers(-10, 11, (h + 1, 1, 3))).astype(np.uint8)
    for y in rng.integers(0, h, 2000):      # strokes of ink down the column, a checker of extremes near both ends
        col[y:y + 5] = 30
    col[3:6, 0, :] = np.array([255, 0, 255], np.uint8)[:, None]
    col[h - 6:h - 3, 0, :] = np.array([0, 255, 0], np.uint8)[:, None]
    page = np.ascontiguousarray(col[:h])
    got = prl.binarizeByLocalVariancesWithoutFilters(torch.from_numpy(page).to(cuda_device), 0.0625, 10).cpu().numpy()
    want = oracle.binarize_lv_nofilters(page, 0.0625, 10)
    assert np.array_equal(got, want), int((got != want).sum())
    assert 1000 < int((want == 255).sum()) < h - 1000 and want[h - 20:].any()
    with pytest.raises(_capi.PrlError) as e:
        prl.binarizeByLocalVariancesWithoutFilters(torch.from_numpy(col).to(cuda_device), 0.0625, 10)
    assert e.value.status == _capi.PRL_ERR_BAD_ARG
