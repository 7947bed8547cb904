"""prl::binarizeFBCITB and its own device parts (fbcitb.hip) against tests/fbcitb_ref.py: the variance mask, the ordered paint, and
the whole call in its three modes through Python and the host entry.  Every byte and every count is compared for equality."""
import os
import subprocess

import numpy as np
import pytest

import fbcitb_ref as fr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev_of(page, device):
    import torch

    return torch.from_numpy(np.ascontiguousarray(page)).to(device)


# ---- the variance mask -----------------------------------------------------------------------------------------------------------

def disagreeing_page():
    """41 x 67 x 3: smooth noise whose channels have their busy regions in different places, so the three channel masks differ"""
    page = np.stack([fr.smooth_noise(41, 67, 30 + c, spread=4 + 10 * c) for c in range(3)], axis=2)
    page[:, :22, 0] = 90
    page[:14, :, 1] = 120
    return np.ascontiguousarray(page)


@pytest.mark.parametrize("threshold", (0.0, 0.005, 200.0, 200.5, 16000.0))
def test_variance_mask_thresholds(prl, cuda_device, threshold):
    """0 and 0.005 lie below the map's 0.01 floor (every pixel passes); 16 000 is above every value but the largest windows'"""
    colour = disagreeing_page()
    gray = fr.noise(19, 300, 1, 3)      # more than one block of 256 columns; the page edge replicates
    edge = np.zeros((5, 7), np.uint8)
    edge[0, :] = 255                    # a window of the replicated edge: rows -1 and 0 are equal
    for page in (colour, gray, edge, np.array([[7]], np.uint8)):
        got = prl.varianceMask(dev_of(page, cuda_device), threshold).cpu().numpy()
        want = fr.variance_mask(page, threshold)
        assert np.array_equal(got, want), (page.shape, threshold, int((got != want).sum()))
    if threshold == 200.0:
        import lv_ref as lv

        each = lv.variance_map(colour) > np.float32(200.0)
        assert len({each[..., c].tobytes() for c in range(3)}) == 3, "the three channels disagree"
        m = fr.variance_mask(colour, threshold)
        assert (m == 255).any() and (m == 0).any()
    if threshold < 0.01:
        assert (fr.variance_mask(colour, threshold) == 255).all()


def test_variance_mask_nan_and_a_batch(prl, cuda_device):
    pages = np.stack([fr.noise(20, 33, 3, s) for s in range(3)])
    got = prl.varianceMask(dev_of(pages, cuda_device), 1500.0).cpu().numpy()
    for i in range(3):
        assert np.array_equal(got[i], fr.variance_mask(pages[i], 1500.0))
    assert (prl.varianceMask(dev_of(pages[0], cuda_device), float("nan")).cpu().numpy() == 0).all()
    assert (prl.varianceMask(dev_of(pages[0], cuda_device), 1e30).cpu().numpy() == 0).all()


# ---- the ordered paint -----------------------------------------------------------------------------------------------------------

def test_paint_small_rectangles_borders_and_order(prl, cuda_device):
    gray = fr.noise(40, 70, 1, 5)
    H, W = gray.shape
    rects = [(0, 0, W, H, 128, 0),            # the whole page
             (0, 0, 1, 1, 0, 1), (W - 1, 0, 1, 1, 0, 0), (0, H - 1, 1, 1, 255, 1), (W - 1, H - 1, 1, 1, 256, 0),   # one pixel, the four corners
             (0, 5, 3, 20, 100, 1), (W - 4, 5, 4, 20, 100, 0), (10, 0, 30, 2, 77, 1), (10, H - 3, 30, 3, 77, 0),   # the four borders
             (20, 10, 25, 15, 140, 0), (30, 15, 25, 15, 140, 1),                                               # overlapping, opposite polarities
             (-1, 0, 5, 5, 0, 0), (W - 2, 0, 3, 3, 0, 0), (5, 5, 0, 4, 0, 0)]                                      # not on the page: ignored
    want = fr.paint(gray, rects)
    got = prl.rectPaint(dev_of(gray, cuda_device), rects).cpu().numpy()
    assert np.array_equal(got, want)
    swapped = list(rects)
    swapped[9], swapped[10] = swapped[10], swapped[9]
    want2 = fr.paint(gray, swapped)
    assert not np.array_equal(want, want2), "the order matters where the two overlap"
    assert np.array_equal(prl.rectPaint(dev_of(gray, cuda_device), swapped).cpu().numpy(), want2)
    assert (prl.rectPaint(dev_of(gray, cuda_device), []).cpu().numpy() == 255).all()


def test_paint_3000_overlapping_rectangles_and_an_empty_page(prl, cuda_device):
    """3000 rectangles over one another on the first page (small and large ones: both kernels), none on the second, 50 on the third"""
    rng = np.random.default_rng(9)
    H, W = 120, 200
    gray = np.stack([fr.noise(H, W, 1, s) for s in (1, 2, 3)])

    def some(n):
        out = []
        for _ in range(n):
            w, h = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
            if rng.random() < 0.7:
                w, h = min(w, 40), min(h, 40)
            out.append((int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h, int(rng.integers(0, 257)), int(rng.integers(0, 2))))
        return out

    lists = [some(3000), [], some(50)]
    assert sum(1 for r in lists[0] if r[2] * r[3] > 4096) > 100 and sum(1 for r in lists[0] if r[2] * r[3] <= 4096) > 1000
    got = prl.rectPaint(dev_of(gray, cuda_device), lists).cpu().numpy()
    for i in range(3):
        assert np.array_equal(got[i], fr.paint(gray[i], lists[i])), i
    assert (got[1] == 255).all()


# ---- the whole call --------------------------------------------------------------------------------------------------------------

def pages():
    from prlib_amd import synth

    text = synth.text_page_numpy(200, 300, 20)
    gray = np.load(os.path.join(ROOT, "tests", "golden", "scans", "0004.npz"))["gray"][400:640, 300:556]
    bgr = np.load(os.path.join(ROOT, "tests", "golden", "autocrop", "photo_05_600x440.npz"))["bgr"][100:356, 200:456]
    return dict(text=text, gray=np.ascontiguousarray(gray), bgr=np.ascontiguousarray(bgr))


# (page, useCanny, useVariancesMap, the least number of kept contours the page must give).  A numpy prototype of the reference
# that counted contours passing the rectangle filters WITHOUT the hierarchy pruning gave, for both stages / the variance mask with
# Canny / CannyEdgeDetection alone: 16 / 183 / 106 on the gray crop, 0 / 65 / 54 on the text page, 0 / 1 / 1 on the colour crop.
# The pruning can only drop contours, so those are upper bounds; the least counts asked here are a half of them or less (a fifth where
# children dominate), and 0 where the prototype found none: the header default on clean text paints nothing, which is the reference.
MODES = [("gray", True, True, 8), ("gray", False, True, 50), ("gray", True, False, 20), ("gray", False, False, 50),
         ("text", False, True, 20), ("text", True, False, 10), ("text", False, False, 20), ("text", True, True, 0),
         ("bgr", False, True, 1), ("bgr", True, False, 1), ("bgr", True, True, 0)]


@pytest.mark.parametrize("name, canny, variances, least", MODES, ids=lambda v: str(v))
def test_whole_call_modes(prl, cuda_device, name, canny, variances, least):
    page = pages()[name]
    want, counts = fr.binarize_fbcitb(page, canny, variances)
    got, got_counts = prl.binarizeFBCITB(dev_of(page, cuda_device), canny, variances, with_counts=True)
    assert tuple(got_counts.tolist()) == counts, (got_counts, counts)
    assert counts[2] >= least, counts
    got = got.cpu().numpy()
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("off", ("useCLAHE", "useBilateral", "useMorphology", "useCannyOnVariances"))
def test_whole_call_each_stage_off_once(prl, cuda_device, off):
    ref_name = dict(useCLAHE="use_clahe", useBilateral="use_bilateral", useMorphology="use_morphology", useCannyOnVariances="canny_on_variances")[off]
    for name, canny, variances in (("gray", True, True), ("text", False, True), ("bgr", True, False)):
        page = pages()[name]
        want, counts = fr.binarize_fbcitb(page, canny, variances, **{ref_name: False})
        got, got_counts = prl.binarizeFBCITB(dev_of(page, cuda_device), canny, variances, with_counts=True, **{off: False})
        assert tuple(got_counts.tolist()) == counts and np.array_equal(got.cpu().numpy(), want), (name, off, counts, got_counts)


def test_a_batch_a_flat_page_and_the_host_entry(prl, cuda_device):
    from prlib_amd import synth

    batch = np.stack([synth.text_page_numpy(120, 160, 30), np.full((120, 160), 200, np.uint8), synth.text_page_numpy(120, 160, 31)])
    got, counts = prl.binarizeFBCITB(dev_of(batch, cuda_device), False, True, with_counts=True)
    got = got.cpu().numpy()
    for i in range(3):
        want, c = fr.binarize_fbcitb(batch[i], False, True)
        assert tuple(counts[i].tolist()) == c and np.array_equal(got[i], want), i
    assert (got[1] == 255).all() and tuple(counts[1].tolist()) == (0, 0, 0), "a flat page has no contours and is all white"
    assert counts[0][2] >= 5 and counts[2][2] >= 5
    page = pages()["gray"]
    want, c = fr.binarize_fbcitb(page, False, True)
    got, counts = prl.binarizeFBCITB(page, False, True, with_counts=True)   # numpy in: the host entry
    assert np.array_equal(got, want) and tuple(counts.tolist()) == c
    colour = pages()["bgr"]
    assert np.array_equal(prl.binarizeFBCITB(colour, True, False), fr.binarize_fbcitb(colour, True, False)[0])


def test_dropin_caller_mutates_a_gray_mat_and_agrees_with_the_restatement(prl, cuda_device, tmp_path):
    """prl::binarizeFBCITB through the C++ drop-in header: a gray input comes back as its GRAY2BGR conversion (the program checks the
    caller's Mat), a colour input untouched; the masks are the restatement's; prl::bilateralFilter beside it"""
    from test_fbcitb_cpu import build_dropin

    exe = build_dropin(str(tmp_path))
    for name, canny, variances in (("gray", False, True), ("bgr", True, False)):
        page = pages()[name]
        cn = 1 if page.ndim == 2 else 3
        src, dst = str(tmp_path / (name + ".in")), str(tmp_path / (name + ".out"))
        page.tofile(src)
        r = subprocess.run([exe, "run", str(page.shape[0]), str(page.shape[1]), str(cn), src, dst, str(int(canny)), str(int(variances))],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "fbcitb dropin run: OK" in r.stdout, r.stdout + r.stderr
        got = np.fromfile(dst, np.uint8).reshape(page.shape[:2])
        assert np.array_equal(got, fr.binarize_fbcitb(page, canny, variances)[0]), name
    page = pages()["bgr"][:60, :70]
    src, dst = str(tmp_path / "f.in"), str(tmp_path / "f.out")
    np.ascontiguousarray(page).tofile(src)
    r = subprocess.run([exe, "filter", "60", "70", "3", src, dst, "7", "25.0", "3.0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "fbcitb dropin run: OK" in r.stdout, r.stdout + r.stderr
    assert np.array_equal(np.fromfile(dst, np.uint8).reshape(60, 70, 3), fr.bilateral(np.ascontiguousarray(page), 7, 25.0, 3.0))
