"""prl::removeLines (lines.hip) on the MI355X: every output byte against the restatement of tests/lines_ref.py - the sizes that
put the element lengths where the bit kernels can break, every input family, per-page thresholds in a batch, colour, strided
layouts, in place, a side stream, crops of the reference's scans, the byte path of the hooks build, the C++ drop-in and the
numpy host entry."""
import os
import subprocess
import sys

import numpy as np
import pytest

import lines_ref as lr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mismatch(got, want):
    bad = np.argwhere(got != want)
    return int(bad.shape[0]), bad[:5].tolist()


def _dev(prl, pages, **kw):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(pages)).cuda()
    r = prl.removeLines(t, **kw)
    torch.cuda.synchronize()
    return r.cpu().numpy()


@pytest.mark.parametrize("size", lr.SIZES, ids=[f"{w}x{h}" for w, h in lr.SIZES])
def test_sizes_and_families(prl, cuda_device, oracle, size):
    """smallest legal and L = 1, 2, 3; L = 63 / 64 / 65 each way; L = 129; L = 260 (beyond the byte path) each way; a ragged last
    word with both passes at work - all families of a size in one batch"""
    w, h = size
    fam = lr.families(w, h, seed=3)
    pages = np.stack([p for _, p in fam])
    got = _dev(prl, pages)
    assert got.shape == pages.shape and got.dtype == np.uint8
    for i, (name, page) in enumerate(fam):
        n_bad, where = _mismatch(got[i], lr.remove_lines(page))
        print(f"{w}x{h} {name}: {n_bad} mismatching bytes")
        assert n_bad == 0, (size, name, where)


def _contrast_batch(w, h):
    base = lr.table_page(w, h, 11).astype(np.float64)
    pages = [base, 255 - (255 - base) * 0.5, base * 0.55 + 20, 128 + (base - 128) * 0.3, np.clip(base * 1.2 - 60, 0, 255)]
    return np.stack([np.clip(p, 0, 255).astype(np.uint8) for p in pages])


def test_batch_of_pages_with_their_own_thresholds(prl, cuda_device, oracle):
    pages = _contrast_batch(1031, 517)
    thr = [lr.mask_of(p)[1] for p in pages]
    assert len(set(thr)) >= 4, thr
    got = _dev(prl, pages)
    for i, p in enumerate(pages):
        n_bad, where = _mismatch(got[i], lr.remove_lines(p))
        print(f"page {i} (t = {thr[i]}): {n_bad} mismatching bytes")
        assert n_bad == 0, (i, where)
        assert np.array_equal(_dev(prl, p), got[i])   # a batch equals one call per page


def test_threshold_scan_runs_over_the_inverted_page(prl, cuda_device, oracle):
    """pages with a tie in Otsu's between-class variance (tests/test_lines_cpu.py holds that a scan from the other end classifies
    their half-way pixels the other way)"""
    pages = np.stack([lr.tie_page(4), lr.tie_page(8), 255 - lr.tie_page(4), 255 - lr.tie_page(8)])
    got = _dev(prl, pages)
    for i, p in enumerate(pages):
        assert np.array_equal(got[i], lr.remove_lines(p)), i
    assert (got[0][:, 80:][pages[0][:, 80:] == 125] == 0).all() and (got[1] == 255).all()


def _colour(w, h, seed):
    rng = np.random.default_rng(seed)
    g = lr.table_page(w, h, seed).astype(np.int16)
    bgr = np.stack([g + rng.integers(-25, 26, size=g.shape) for _ in range(3)], axis=2)
    return np.clip(bgr, 0, 255).astype(np.uint8)


def test_three_channels(prl, cuda_device, oracle):
    for w, h in ((1031, 517), (150, 150), (257, 131)):
        pages = np.stack([_colour(w, h, s) for s in (1, 2, 3)])
        got = _dev(prl, pages)
        assert got.shape == (3, h, w)
        for i in range(3):
            n_bad, where = _mismatch(got[i], lr.remove_lines(pages[i]))
            print(f"colour {w}x{h} page {i}: {n_bad} mismatching bytes")
            assert n_bad == 0, (w, h, i, where)
        one = _dev(prl, pages[1])   # H x W x 3
        assert one.shape == (h, w) and np.array_equal(one, got[1])


@pytest.mark.parametrize("c", [1, 3])
def test_strided_rows_and_pages(prl, cuda_device, oracle, c):
    import torch

    w, h = 203, 117
    pages = np.stack([_colour(w, h, s) for s in (4, 5, 6)]) if c == 3 else _contrast_batch(w, h)[:3]
    n = pages.shape[0]
    want = np.stack([lr.remove_lines(p) for p in pages])
    # source rows of w c + 5 bytes, pages 9 rows apart; destination rows of w + 3 bytes, 4 spare rows: nothing a multiple of 4
    sb = torch.full((n, h + 9, w * c + 5), 7, dtype=torch.uint8, device="cuda")
    sv = sb[:, :h, :w * c]
    sv = sv.unflatten(2, (w, c)) if c == 3 else sv
    sv.copy_(torch.from_numpy(pages))
    db = torch.full((n, h + 4, w + 3), 201, dtype=torch.uint8, device="cuda")
    dv = db[:, :h, :w]
    prl.removeLines(sv, out=dv)
    torch.cuda.synchronize()
    n_bad, where = _mismatch(dv.cpu().numpy(), want)
    assert n_bad == 0, where
    d = db.cpu().numpy()
    assert (d[:, h:] == 201).all() and (d[:, :, w:] == 201).all(), "padding bytes of the destination written"
    s = sb.cpu().numpy()
    assert np.array_equal(s[:, :h, :w * c].reshape(pages.shape), pages) and (s[:, h:] == 7).all() and (s[:, :, w * c:] == 7).all()


def test_in_place(prl, cuda_device, oracle):
    import torch

    w, h = 203, 117
    pages = _contrast_batch(w, h)
    want = np.stack([lr.remove_lines(p) for p in pages])
    ip = torch.from_numpy(pages).cuda()
    prl.removeLines(ip, out=ip)
    torch.cuda.synchronize()
    assert np.array_equal(ip.cpu().numpy(), want)
    sb = torch.full((5, h + 2, w + 5), 9, dtype=torch.uint8, device="cuda")
    sv = sb[:, :h, :w]
    sv.copy_(torch.from_numpy(pages))
    prl.removeLines(sv, out=sv)
    torch.cuda.synchronize()
    assert np.array_equal(sv.cpu().numpy(), want)
    s = sb.cpu().numpy()
    assert (s[:, h:] == 9).all() and (s[:, :, w:] == 9).all()


def test_side_stream(prl, cuda_device, oracle):
    import torch

    pages = _contrast_batch(300, 260)
    t = torch.from_numpy(pages).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out = prl.removeLines(t)
        out2 = prl.removeLines(out)
    s.synchronize()
    want = np.stack([lr.remove_lines(p) for p in pages])
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(out2.cpu().numpy(), np.stack([lr.remove_lines(p) for p in want]))


CROPS = ["0018_x1000_y400_1536x1024", "0037_x700_y900_1024x1536", "0064_x1800_y700_1536x1024"]


@pytest.mark.parametrize("name", CROPS)
def test_reference_scan_crops(prl, cuda_device, oracle, name):
    img = np.load(os.path.join(ROOT, "tests", "golden", "scans", name + ".npz"))["gray"]
    assert img.shape[0] <= 1536 and img.shape[1] <= 1536 and img.size <= 1536 * 1024
    want = lr.remove_lines(img)
    n_bad, where = _mismatch(_dev(prl, img), want)
    print(f"{name}: {n_bad} mismatching bytes of {want.size}; {int((want == 0).sum())} ink pixels kept")
    assert n_bad == 0, where


def test_byte_path_of_the_hooks_build_equals_the_bit_path(prl, cuda_device, oracle, tmp_path):
    """PRL_HIP_LINES_BYTES=1 (hooks build): the two openings through k_gm_span on byte masks, in a child process"""
    code = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from prlib_amd import _capi
_capi.use_library(_capi.HOOKS_LIB_PATH)
import torch, prlib_amd
z = np.load(sys.argv[2])
out = {}
for key in z.files:
    out[key] = prlib_amd.removeLines(torch.from_numpy(z[key]).cuda()).cpu().numpy()
np.savez(sys.argv[3], **out)
print("bytes ok")
'''
    sizes = [(50, 50), (99, 120), (150, 150), (3200, 65), (65, 3200), (6450, 130), (1031, 517)]
    pages = {f"g{w}x{h}": np.stack([p for _, p in lr.families(w, h, seed=5)]) for w, h in sizes}
    pages["c257x131"] = np.stack([_colour(257, 131, s) for s in (7, 8)])
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, **pages)
    env = dict(os.environ, PRL_HIP_LINES_BYTES="1")
    r = subprocess.run([sys.executable, "-c", code, ROOT, src, dst], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "bytes ok" in r.stdout, r.stdout + r.stderr[-3000:]
    byt = np.load(dst)
    for key, p in pages.items():
        bits = _dev(prl, p)
        n_bad, where = _mismatch(byt[key], bits)
        print(f"{key}: byte path vs bit path {n_bad} mismatching bytes")
        assert n_bad == 0, (key, where)
        assert np.array_equal(bits[-1], lr.remove_lines(p[-1])), key


def test_cpp_dropin_on_device(prl, cuda_device, oracle, tmp_path):
    from test_lines_cpu import build_dropin

    exe = build_dropin(str(tmp_path))
    for name, img, roi in (("gray", lr.table_page(333, 211, 4), False), ("gray_roi", lr.table_page(333, 211, 5), True),
                           ("bgr_roi", _colour(260, 190, 6), True)):
        src = tmp_path / f"{name}.raw"
        dst = tmp_path / f"{name}.out"
        src.write_bytes(np.ascontiguousarray(img).tobytes())
        h, w = img.shape[:2]
        c = img.shape[2] if img.ndim == 3 else 1
        r = subprocess.run([exe, "run", str(h), str(w), str(c), str(src), str(dst)] + (["roi"] if roi else []), capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0 and "lines dropin run: OK" in r.stdout, r.stdout + r.stderr
        view = np.ascontiguousarray(img[2:h - 3, 3:w - 4] if roi else img)
        got = np.frombuffer(dst.read_bytes(), np.uint8).reshape(view.shape[:2])
        assert np.array_equal(got, lr.remove_lines(view)), name


def test_host_entry_numpy(prl, cuda_device, oracle):
    from prlib_amd import _capi

    for img in (lr.table_page(203, 117, 1), lr.table_page(203, 117, 2)[:, :, None], _colour(203, 117, 3), lr.table_page(50, 50, 4)):
        got = prl.removeLines(img)
        assert got.shape == img.shape[:2] and np.array_equal(got, lr.remove_lines(img))
    view = _colour(240, 160, 9)[5:140, 7:231]   # strided rows
    assert np.array_equal(prl.removeLines(view), lr.remove_lines(np.ascontiguousarray(view)))
    out = np.full((117, 203), 3, np.uint8)
    assert prl.removeLines(lr.table_page(203, 117, 1), out=out) is out and np.array_equal(out, lr.remove_lines(lr.table_page(203, 117, 1)))
    marker = np.full((40, 203), 3, np.uint8)
    with pytest.raises(_capi.PrlError) as e:   # below 50 rows: refused with the output untouched
        prl.removeLines(lr.table_page(203, 117, 1)[:40], out=marker)
    assert e.value.status == _capi.PRL_ERR_BAD_ARG and (marker == 3).all()
