"""tone.hip on the MI355X, every byte against tests/tone_ref.py: the histogram kernel against np.bincount on the pages its
wavefront-uniform shortcut could get wrong, the table kernel, the four reference functions on batches of strided pages, the
tables derived on the device against the host builders', two of the reference's colour scans, the numpy host entries and the
C++ drop-in.  (Written without access to a device: this file has not yet run on an MI355X; its own logic was run on the CPU with
the models of tone_ref.py standing in for the library.)"""
import os
import subprocess

import numpy as np
import pytest

import tone_ref as tr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTION_SIZES = [(1031, 517), (99, 120)]


def _mismatch(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape)
    bad = np.argwhere(got != want)
    return int(bad.shape[0]), bad[:5].tolist()


def _cuda(a):
    import torch

    return torch.from_numpy(np.array(a, order="C")).cuda()   # (a copy: broadcast views are read-only)


def _strided(pages, fill=7):
    """N x H x W x C on the device with rows of W C + 1 bytes (off dword alignment) and two spare rows between pages"""
    import torch

    n, h, w, c = pages.shape
    buf = torch.full((n, h + 2, w * c + 1), fill, dtype=torch.uint8, device="cuda")
    view = buf[:, :h, :w * c].unflatten(2, (w, c))
    view.copy_(torch.from_numpy(np.ascontiguousarray(pages)))
    return buf, view


def _padding_intact(buf, h, row, fill):
    b = buf.cpu().numpy()
    return (b[:, h:] == fill).all() and (b[:, :, row:] == fill).all()


# ---- histogram -------------------------------------------------------------------------------------------------------------------

def _want_hist(pages):
    return np.stack([tr.histograms(p) for p in pages])


@pytest.mark.parametrize("size", tr.HIST_SIZES, ids=[f"{w}x{h}" for w, h in tr.HIST_SIZES])
def test_histogram_against_bincount(prl, cuda_device, size):
    """all families of a size in one call per channel count; 2 channels on one size"""
    import torch

    w, h = size
    for c in (1, 3, 4) + ((2,) if size == (257, 3) else ()):
        fam = tr.hist_families(w, h, c, seed=3)
        pages = np.stack([p for _, p in fam])
        out = torch.full((len(fam), c, 256), -12345, dtype=torch.int32, device="cuda")   # garbage: the call overwrites it
        got = prl.histogram(_cuda(pages), out=out)
        torch.cuda.synchronize()
        got = got.cpu().numpy().astype(np.int64)
        want = _want_hist(pages)
        for i, (name, _) in enumerate(fam):
            n_bad = int((got[i] != want[i]).sum())
            print(f"{w}x{h} C={c} {name}: {n_bad} wrong bins")
            assert n_bad == 0, (size, c, name, np.argwhere(got[i] != want[i])[:5].tolist())
        assert (got.sum(axis=2) == w * h).all()


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_histogram_strided_and_shapes(prl, cuda_device, c):
    import torch

    w, h = 203, 117
    pages = np.stack([tr.noise_page(w, h, c, 1), tr.checker_page(w, h, c), tr.ramp_page(w, h, c)])   # three different pages
    want = _want_hist(pages)
    buf, view = _strided(pages)
    got = prl.histogram(view)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)
    assert _padding_intact(buf, h, w * c, 7)
    one = prl.histogram(_cuda(pages[1]) if c > 1 else _cuda(pages[1][:, :, 0]))   # H x W x C / H x W
    assert tuple(one.shape) == (c, 256) and np.array_equal(one.cpu().numpy(), want[1])
    if c == 1:
        assert np.array_equal(prl.histogram(_cuda(pages[:, :, :, 0])).cpu().numpy(), want)   # N x H x W


# ---- table look-up -----------------------------------------------------------------------------------------------------------------

def _tables(n, c, seed):
    rng = np.random.default_rng(seed)
    return np.stack([np.stack([rng.permutation(256) for _ in range(c)]) for _ in range(n)]).astype(np.uint8)


@pytest.mark.parametrize("size", tr.HIST_SIZES, ids=[f"{w}x{h}" for w, h in tr.HIST_SIZES])
def test_lut_sizes(prl, cuda_device, size):
    import torch

    w, h = size
    for c in (1, 3, 4) + ((2,) if size == (257, 3) else ()):
        pages = np.stack([tr.noise_page(w, h, c, 5), tr.ramp_page(w, h, c), tr.checker_page(w, h, c)])
        t = _cuda(pages)
        ident = np.broadcast_to(np.arange(256, dtype=np.uint8), (c, 256))
        rev = np.ascontiguousarray(ident[:, ::-1])
        perm = _tables(3, c, 11)
        assert np.array_equal(prl.lut(t, _cuda(ident)).cpu().numpy(), pages)
        assert np.array_equal(prl.lut(t, _cuda(rev)).cpu().numpy(), 255 - pages)
        shared = prl.lut(t, _cuda(perm[0])).cpu().numpy()
        per_page = prl.lut(t, _cuda(perm)).cpu().numpy()
        torch.cuda.synchronize()
        for i in range(3):
            assert _mismatch(shared[i], tr.apply_luts(pages[i], perm[0]))[0] == 0, (size, c, i)
            assert _mismatch(per_page[i], tr.apply_luts(pages[i], perm[i]))[0] == 0, (size, c, i)


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_lut_strided_in_place_and_side_stream(prl, cuda_device, c):
    import torch

    w, h = 203, 117
    pages = np.stack([tr.noise_page(w, h, c, s) for s in (1, 2, 3)])
    perm = _tables(3, c, 7)
    want = np.stack([tr.apply_luts(pages[i], perm[i]) for i in range(3)])
    sbuf, sview = _strided(pages, 7)
    dbuf, dview = _strided(np.zeros_like(pages), 201)
    dbuf.fill_(201)
    prl.lut(sview, _cuda(perm), out=dview)
    torch.cuda.synchronize()
    assert _mismatch(dview.cpu().numpy(), want)[0] == 0
    assert _padding_intact(dbuf, h, w * c, 201) and _padding_intact(sbuf, h, w * c, 7)
    assert np.array_equal(sview.cpu().numpy(), pages)
    prl.lut(sview, _cuda(perm), out=sview)   # in place, strided
    torch.cuda.synchronize()
    assert _mismatch(sview.cpu().numpy(), want)[0] == 0 and _padding_intact(sbuf, h, w * c, 7)
    t = _cuda(pages)
    tab = _cuda(perm)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a = prl.lut(t, tab)
        b = prl.lut(a, tab)
    s.synchronize()
    assert np.array_equal(a.cpu().numpy(), want)
    assert np.array_equal(b.cpu().numpy(), np.stack([tr.apply_luts(want[i], perm[i]) for i in range(3)]))


# ---- the four functions ----------------------------------------------------------------------------------------------------------

def _run_strided(fn, pages, oc):
    """fn(view, out=view) on strided source and destination batches; returns the result and checks both paddings"""
    import torch

    n, h, w, c = pages.shape
    sbuf, sview = _strided(pages, 7)
    dbuf, dview = _strided(np.zeros((n, h, w, oc), np.uint8), 201)
    dbuf.fill_(201)
    fn(sview, dview)
    torch.cuda.synchronize()
    assert _padding_intact(dbuf, h, w * oc, 201) and _padding_intact(sbuf, h, w * c, 7), "padding bytes written"
    assert np.array_equal(sview.cpu().numpy(), pages), "the source was written"
    return dview.cpu().numpy()


def _colour_batch(w, h, seed):
    fam = dict(tr.colour_families(w, h, seed))
    return np.stack([fam["noise"], fam["paper"], fam["gray3"]])


@pytest.mark.parametrize("size", FUNCTION_SIZES, ids=[f"{w}x{h}" for w, h in FUNCTION_SIZES])
@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_gamma_correction(prl, cuda_device, size, c):
    w, h = size
    pages = np.stack([tr.noise_page(w, h, c, 1), tr.ramp_page(w, h, c), tr.checker_page(w, h, c)])
    oc = 3 if c == 4 else c
    for k, gamma in ((1.0, 2.2), (0.5, 0.4), (1.7, 1.0), (1.0 + 5e-8, 2.2)):
        got = _run_strided(lambda s, d: prl.gammaCorrection(s, k, gamma, out=d), pages, oc)
        for i in range(3):
            n_bad, where = _mismatch(got[i], tr.gamma_model(pages[i], k, gamma))
            print(f"gamma {w}x{h} C={c} k={k} gamma={gamma} page {i}: {n_bad} mismatching bytes")
            assert n_bad == 0, (size, c, k, gamma, i, where)
    if c == 4:   # alpha dropped, no gamma: only the k step
        assert np.array_equal(got, tr.k_step_lut(1.0 + 5e-8)[pages[:, :, :, :3]])
    if c in (1, 3):   # in place, and the shapes without a page / channel axis
        t = _cuda(pages)
        prl.gammaCorrection(t, 0.5, 2.2, out=t)
        assert np.array_equal(t.cpu().numpy(), np.stack([tr.gamma_model(p, 0.5, 2.2) for p in pages]))
        one = pages[0] if c == 3 else pages[0][:, :, 0]
        assert np.array_equal(prl.gammaCorrection(_cuda(one), 1.7, 0.4).cpu().numpy(), tr.gamma_model(one, 1.7, 0.4))


@pytest.mark.parametrize("size", FUNCTION_SIZES, ids=[f"{w}x{h}" for w, h in FUNCTION_SIZES])
def test_simple_white_balance(prl, cuda_device, size):
    w, h = size
    pages = _colour_batch(w, h, 1)
    for k in tr.SWB_KS:
        got = _run_strided(lambda s, d: prl.simpleWhiteBalance(s, k, out=d), pages, 3)
        for i in range(3):
            n_bad, where = _mismatch(got[i], tr.swb_model(pages[i], k))
            print(f"simple white balance {w}x{h} k={k} page {i}: {n_bad} mismatching bytes")
            assert n_bad == 0, (size, k, i, where)
    assert np.array_equal(got[0], tr.swb_literal(pages[0], tr.SWB_KS[-1]))
    fam = dict(tr.colour_families(w, h, 2))
    degenerate = np.stack([fam[n] for n in ("zero_channel", "flat255", "flat100", "two_valued", "flat_each", "ramp")])
    for k in (0.01, 0.5, 25.0):
        got = prl.simpleWhiteBalance(_cuda(degenerate), k).cpu().numpy()
        for i, p in enumerate(degenerate):
            assert _mismatch(got[i], tr.swb_model(p, k))[0] == 0, (size, k, i)
    t = _cuda(pages)
    prl.simpleWhiteBalance(t, 0.01, out=t)   # in place
    assert np.array_equal(t.cpu().numpy(), np.stack([tr.swb_model(p, 0.01) for p in pages]))


@pytest.mark.parametrize("size", FUNCTION_SIZES, ids=[f"{w}x{h}" for w, h in FUNCTION_SIZES])
def test_gray_world(prl, cuda_device, size):
    w, h = size
    pages = _colour_batch(w, h, 1)
    for p, wm in ((1.0, False), (1.0, True), (2.5, True), (2.0, False)):
        got = _run_strided(lambda s, d: prl.grayWorldWhiteBalance(s, p, wm, out=d), pages, 3)
        for i in range(3):
            n_bad, where = _mismatch(got[i], tr.gw_model(pages[i], p, wm))
            print(f"gray world {w}x{h} p={p} withMax={wm} page {i}: {n_bad} mismatching bytes")
            assert n_bad == 0, (size, p, wm, i, where)
    assert np.array_equal(got[1], tr.gw_literal(pages[1], 2.0, False))
    fam = dict(tr.colour_families(w, h, 2))
    degenerate = np.stack([fam[n] for n in ("zero_channel", "flat255", "flat100", "two_valued", "flat_each", "ramp")]
                          + [tr.flat_page(w, h, (0, 0, 0))])
    for p, wm in ((1.0, False), (1.0, True), (0.5, False)):
        got = prl.grayWorldWhiteBalance(_cuda(degenerate), p, wm).cpu().numpy()
        for i, page in enumerate(degenerate):
            assert _mismatch(got[i], tr.gw_model(page, p, wm))[0] == 0, (size, p, wm, i)
    assert (got[-1] == 255).all() and (got[0][:, :, 1] == 255).all()   # NaN -> 255


def test_gray_world_p1_enqueues_without_a_host_round_trip(prl, cuda_device):
    """behind a kernel that keeps the stream busy for some milliseconds, the p = 1 call (and simpleWhiteBalance) return with the
    stream's work still pending: histograms and tables never leave the device"""
    import torch

    pages = _cuda(_colour_batch(99, 120, 3))
    out, out2 = torch.empty_like(pages), torch.empty_like(pages)
    prl.grayWorldWhiteBalance(pages, 1.0, False, out=out)   # (the workspace is allocated here, not behind the busy kernel)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.cuda._sleep(20_000_000)
        prl.grayWorldWhiteBalance(pages, 1.0, True, out=out)
        pending = not s.query()
        prl.simpleWhiteBalance(pages, 0.01, out=out2)
        pending_swb = not s.query()
    s.synchronize()
    assert pending and pending_swb, "a device-resident path waited for the stream"
    host = pages.cpu().numpy()
    assert np.array_equal(out.cpu().numpy(), np.stack([tr.gw_model(p, 1.0, True) for p in host]))
    assert np.array_equal(out2.cpu().numpy(), np.stack([tr.swb_model(p, 0.01) for p in host]))


@pytest.mark.parametrize("size", FUNCTION_SIZES + [(9, 14)], ids=["1031x517", "99x120", "9x14_below_one_tile"])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_clean_background(prl, cuda_device, oracle, size, c):
    w, h = size
    paper = tr.paper_page(w, h, 5)
    base = [paper, tr.paper_page(w, h, 6, tint=(180, 190, 170)), tr.noise_page(w, h, 3, 7)]
    if c == 1:
        pages = np.stack([p[:, :, 1:2] for p in base])
    elif c == 3:
        pages = np.stack(base)
    else:
        pages = np.stack([np.concatenate([p, tr.noise_page(w, h, 1, 9)], axis=2) for p in base])
    oc = 1 if c == 1 else 3
    got = _run_strided(lambda s, d: prl.cleanBackgroundToWhite(s, out=d), pages, oc)
    norm = prl.backgroundNormalization(_cuda(pages)).cpu().numpy()
    for i in range(3):
        bg = oracle.bgnorm(pages[i]).reshape(h, w, oc)
        assert np.array_equal(norm[i], bg), "prl_hip_bgnorm_batch_device changed"
        n_bad, where = _mismatch(got[i], tr.CLEAN_LUT[bg])
        print(f"clean background {w}x{h} C={c} page {i}: {n_bad} mismatching bytes")
        assert n_bad == 0, (size, c, i, where)
    if size == (9, 14):   # below one 10 x 15 tile the normalisation copies the page: the curve is applied to the copy
        assert np.array_equal(got, tr.CLEAN_LUT[pages[:, :, :, :oc]])
    if c in (1, 3):
        t = _cuda(pages)
        prl.cleanBackgroundToWhite(t, out=t)   # in place
        assert np.array_equal(t.cpu().numpy(), got)
        one = pages[0] if c == 3 else pages[0][:, :, 0]
        assert np.array_equal(prl.cleanBackgroundToWhite(_cuda(one)).cpu().numpy(), got[0] if c == 3 else got[0][:, :, 0])


# ---- the tables derived on the device ----------------------------------------------------------------------------------------

def test_device_tables_equal_the_host_builders(prl, cuda_device):
    """every family with a strip holding all 256 values in every channel: the output there is the page's whole table set, compared
    with prl_hip_*_luts on the histograms the device counted"""
    from prlib_amd import _capi

    L = _capi.lib()
    w, h = 99, 120
    fam = tr.colour_families(w, h, 8)
    pages = np.stack([p for _, p in fam])
    ramp = np.arange(256, dtype=np.uint8)
    for i in range(len(fam)):
        pages[i].reshape(-1, 3)[1000:1256] = ramp[:, None]
    t = _cuda(pages)
    hist = prl.histogram(t).cpu().numpy().astype(np.uint32)
    assert np.array_equal(hist, np.stack([tr.histograms(p) for p in pages]))

    def host_luts(fn, i, *args):
        out = np.zeros((3, 256), np.uint8)
        hh = np.ascontiguousarray(hist[i])
        assert fn(*args, hh.ctypes.data, out.ctypes.data) == 0
        return out

    def device_luts(res, i):
        return np.ascontiguousarray(res[i].reshape(-1, 3)[1000:1256].T)

    for k in tr.SWB_KS + [25.0]:
        res = prl.simpleWhiteBalance(t, k).cpu().numpy()
        for i, (name, _) in enumerate(fam):
            assert np.array_equal(device_luts(res, i), host_luts(L.prl_hip_simple_white_balance_luts, i, k)), (name, k)
    for wm in (0, 1):
        res = prl.grayWorldWhiteBalance(t, 1.0, bool(wm)).cpu().numpy()
        for i, (name, _) in enumerate(fam):
            assert np.array_equal(device_luts(res, i), host_luts(L.prl_hip_gray_world_luts, i, 1.0, wm)), (name, wm)


# ---- the reference's scans, the host entries, C++ ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["chain_0195", "chain_0004_x90_y150_900x1300"])
def test_reference_colour_scans(prl, cuda_device, oracle, name):
    """the reference's programs cannot run here: the expected bytes are the restatement's, none are recorded"""
    img = np.load(os.path.join(ROOT, "tests", "golden", "stages", name + ".npz"))["bgr"]
    t = _cuda(img)
    checks = [("gamma", prl.gammaCorrection(t, 0.9, 2.2), tr.gamma_model(img, 0.9, 2.2)),
              ("simple white", prl.simpleWhiteBalance(t, 0.01), tr.swb_literal(img, 0.01)),
              ("gray world p=1", prl.grayWorldWhiteBalance(t, 1.0, False), tr.gw_literal(img, 1.0, False)),
              ("gray world p=6 max", prl.grayWorldWhiteBalance(t, 6.0, True), tr.gw_model(img, 6.0, True)),
              ("clean background", prl.cleanBackgroundToWhite(t), tr.clean_background(oracle, img))]
    for what, got, want in checks:
        n_bad, where = _mismatch(got.cpu().numpy(), want)
        print(f"{name} {what}: {n_bad} mismatching bytes of {want.size}")
        assert n_bad == 0, (what, where)


def test_host_entries_numpy(prl, cuda_device, oracle):
    from prlib_amd import _capi

    w, h = 203, 117
    bgr = tr.paper_page(w, h, 3)
    gray = bgr[:, :, 1].copy()
    bgra = np.concatenate([bgr, tr.noise_page(w, h, 1, 4)], axis=2)
    for img in (gray, gray[:, :, None], tr.noise_page(w, h, 2, 5), bgr, bgra):
        got = prl.gammaCorrection(img, 0.5, 2.2)
        assert _mismatch(got, tr.gamma_model(img, 0.5, 2.2))[0] == 0
    assert prl.gammaCorrection(bgra, 1.0, 2.2).shape == (h, w, 3)
    assert np.array_equal(prl.simpleWhiteBalance(bgr, 0.01), tr.swb_model(bgr, 0.01))
    assert np.array_equal(prl.grayWorldWhiteBalance(bgr, 1.0, False), tr.gw_model(bgr, 1.0, False))
    assert np.array_equal(prl.grayWorldWhiteBalance(bgr, 2.5, True), tr.gw_model(bgr, 2.5, True))
    for img in (gray, bgr, bgra):
        assert np.array_equal(prl.cleanBackgroundToWhite(img), tr.clean_background(oracle, img))
    view = tr.paper_page(240, 160, 9)[5:140, 7:231]   # strided rows
    assert np.array_equal(prl.simpleWhiteBalance(view, 0.25), tr.swb_model(np.ascontiguousarray(view), 0.25))
    out = np.full((h, w, 3), 3, np.uint8)
    assert prl.grayWorldWhiteBalance(bgr, 3.0, False, out=out) is out and np.array_equal(out, tr.gw_model(bgr, 3.0, False))
    with pytest.raises(_capi.PrlError) as e:
        prl.simpleWhiteBalance(gray, 0.01)
    assert e.value.status == _capi.PRL_ERR_BAD_CHANNELS


def test_cpp_dropin_on_device(prl, cuda_device, oracle, tmp_path):
    from test_tone_cpu import build_dropin

    exe = build_dropin(str(tmp_path))
    bgr = tr.paper_page(260, 190, 6)
    bgra = np.concatenate([bgr, tr.noise_page(260, 190, 1, 2)], axis=2)
    gray = np.ascontiguousarray(bgr[:, :, 1])
    cases = [("gamma", 0.5, 2.2, gray, False, lambda v: tr.gamma_model(v, 0.5, 2.2)),
             ("gamma", 1.7, 0.4, bgr, True, lambda v: tr.gamma_model(v, 1.7, 0.4)),
             ("gamma", 0.5, 2.2, bgra, True, lambda v: tr.gamma_model(v, 0.5, 2.2)),   # 4 channels: 3 come back, no gamma
             ("swb", 0.01, 0, bgr, True, lambda v: tr.swb_model(v, 0.01)),
             ("gw", 1.0, 0, bgr, False, lambda v: tr.gw_model(v, 1.0, False)),
             ("gw", 2.5, 1, bgr, True, lambda v: tr.gw_model(v, 2.5, True)),
             ("clean", 0, 0, gray, True, lambda v: tr.clean_background(oracle, v)),
             ("clean", 0, 0, bgra, False, lambda v: tr.clean_background(oracle, v))]
    for n, (fn, a, b, img, roi, want_of) in enumerate(cases):
        src, dst = tmp_path / f"{n}.raw", tmp_path / f"{n}.out"
        src.write_bytes(np.ascontiguousarray(img).tobytes())
        h, w = img.shape[:2]
        c = img.shape[2] if img.ndim == 3 else 1
        r = subprocess.run([exe, "run", fn, str(a), str(b), str(h), str(w), str(c), str(src), str(dst)] + (["roi"] if roi else []),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "tone dropin run: OK" in r.stdout, (fn, r.stdout + r.stderr)
        view = np.ascontiguousarray(img[2:h - 3, 3:w - 4] if roi else img)
        want = want_of(view)
        got = np.frombuffer(dst.read_bytes(), np.uint8).reshape(want.shape)
        assert np.array_equal(got, want), (fn, c, roi)
        if fn == "gamma" and c == 4:
            assert "channels=3" in r.stdout and np.array_equal(got, tr.k_step_lut(0.5)[view[:, :, :3]])
