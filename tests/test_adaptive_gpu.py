"""The adaptive-threshold binarizers on the MI355X: every kernel path (tile widths 256 / 128 / 64 / 32, both methods, both
threshold types, the byte and the bit-plane output), layouts, the reference's scans, user-sized batches, the C++ drop-in, a
seeded random run and a call beside prl.binarize on another stream - every byte against the restatement of
tests/adaptive_ref.py, 0 differences allowed."""
import glob
import os
import subprocess
import threading

import numpy as np
import pytest

import adaptive_ref as ar
import median_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 61 | 63, 123 | 125, 245 | 247: the sizes on either side of each tile-width switch of k_adaptive
BLOCKS = (3, 5, 7, 9, 19, 21, 61, 63, 101, 123, 125, 245, 247, 255)
DELTAS = (-3.5, -0.5, 0, 0.5, 9, 300)
MAX_VALUES = (-1, 0, 127.5, 255, 300)


def _inputs(h, w, seed):
    """the page kinds of test_median_gpu._inputs (uniform random; synth pages with 5 % and 20 % impulses; all 0; all 255;
    one-pixel checkerboard) plus the stripes page"""
    from test_median_gpu import _inputs as median_inputs

    return np.concatenate([median_inputs(h, w, 1, seed)[..., 0], ar.stripes_page(h, w)[None]])


def _dev(prl, pages, *args, **kw):
    import torch

    r = prl.adaptiveThreshold(torch.from_numpy(pages).cuda(), *args, **kw)
    torch.cuda.synchronize()
    return r.cpu().numpy()


@pytest.mark.parametrize("method", [ar.MEAN_C, ar.GAUSSIAN_C], ids=["mean", "gaussian"])
@pytest.mark.parametrize("shape", [(37, 53), (131, 301)], ids=["37x53", "131x301"])
def test_parity_grid(prl, cuda_device, method, shape):
    import torch

    pages = _inputs(shape[0], shape[1], 5 + method)
    t = torch.from_numpy(pages).cuda()
    side = torch.cuda.Stream()
    calls = 0
    for bs in BLOCKS:
        means = [ar.local_mean(p, method, bs) for p in pages]
        for type_ in (ar.BINARY, ar.BINARY_INV):
            for delta in DELTAS:
                for mv in MAX_VALUES:
                    for inv in (False, True):
                        calls += 1
                        if calls % 7 == 0:   # a non-default stream now and then
                            with torch.cuda.stream(side):
                                got = prl.adaptiveThreshold(t, mv, method, type_, bs, delta, autoInvert=inv)
                            side.synchronize()
                        else:
                            got = prl.adaptiveThreshold(t, mv, method, type_, bs, delta, autoInvert=inv)
                        got = got.cpu().numpy()
                        want = np.stack([ar.threshold_from_mean(p, m, mv, type_, delta, inv) for p, m in zip(pages, means)])
                        bad = np.argwhere(got != want)
                        assert bad.size == 0, (bs, type_, delta, mv, inv, len(bad), bad[:5].tolist())


def test_known_answers_on_device(prl, cuda_device):
    from test_adaptive_cpu import KNOWN, crc, known_pages

    for name, g in known_pages().items():
        # with maxValue 255, delta 0 and BINARY, the mask is p >= M + 1 ... the mean plane itself is not an output; the
        # restatement pins it (test_adaptive_cpu) and the device must give the restatement's masks at those block sizes
        for bs in (3, 7, 19, 101):
            for method in (ar.MEAN_C, ar.GAUSSIAN_C):
                got = _dev(prl, g, 255.0, method, ar.BINARY, bs, 0.0)
                assert np.array_equal(got, ar.adaptive_threshold(g, 255.0, method, ar.BINARY, bs, 0.0)), (name, bs, method)
        m = _dev_native(prl, g)
        assert crc(m) == KNOWN[name]["mask"] and round(float((m == 255).mean()), 4) == KNOWN[name]["white"], name


def _dev_native(prl, img, **kw):
    import torch

    r = prl.binarizeNativeAdaptive(torch.from_numpy(img).cuda(), **kw)
    torch.cuda.synchronize()
    return r.cpu().numpy()


def test_flip_outcomes_in_one_batch(prl, cuda_device):
    """flipping and non-flipping pages side by side, and the boundary at a mean of exactly 128"""
    from prlib_amd import synth

    h, w = 120, 144
    flat = np.full((h, w), 77, np.uint8)
    half = np.zeros((h, w), np.uint8)
    half[:, : w // 2] = 255                                  # mask of maxValue 255: half on -> mean 127.5 -> flips
    pages = np.stack([ar.stripes_page(h, w), synth.page_numpy(h, w, index=3), flat, half,
                      np.random.default_rng(3).integers(0, 256, (h, w), dtype=np.uint8)])
    for mv in (255.0, 128.0, 127.0, 127.5, 128.5, 1.0, 0.0):
        for delta in (9.0, 0.0, -1.0):
            for method in (ar.GAUSSIAN_C, ar.MEAN_C):
                got = _dev(prl, pages, mv, method, ar.BINARY_INV, 19, delta, autoInvert=True)
                want = np.stack([ar.adaptive_threshold(p, mv, method, ar.BINARY_INV, 19, delta, auto_invert=True) for p in pages])
                assert np.array_equal(got, want), (mv, delta, method)
    # the outcomes really are mixed at the defaults
    plain = [ar.adaptive_threshold(p, 255.0, ar.GAUSSIAN_C, ar.BINARY_INV, 19, 9.0) for p in pages]
    assert [ar.flips(m) for m in plain[:3]] == [False, True, True]
    # flat page, delta 0: maxValue 128 -> all 128, mean exactly 128, no flip; 127 -> all 127 -> flips to 128
    for mv, value in ((128.0, 128), (127.0, 128), (127.5, 128), (128.5, 128), (126.0, 129)):
        got = _dev(prl, flat, mv, ar.GAUSSIAN_C, ar.BINARY_INV, 19, 0.0, autoInvert=True)
        assert (got == value).all(), (mv, int(got[0, 0]))


def test_layouts(prl, cuda_device):
    import torch

    h, w = 41, 75
    pages = _inputs(h, w, 17)
    n = pages.shape[0]
    # source rows of 97 bytes, pages 50 rows apart; destination rows of 100 bytes, pages of 45 rows
    sb = torch.full((n, 50, 97), 7, dtype=torch.uint8, device="cuda")
    sv = sb[:, :h, :w]
    sv.copy_(torch.from_numpy(pages))
    for bs, method, inv in ((19, ar.GAUSSIAN_C, True), (5, ar.MEAN_C, False), (63, ar.MEAN_C, True), (125, ar.GAUSSIAN_C, False)):
        db = torch.full((n, 45, 100), 201, dtype=torch.uint8, device="cuda")
        dv = db[:, :h, 3:3 + w]   # destination rows that are not 8-byte aligned: the expand kernel's byte path
        r = prl.adaptiveThreshold(sv, 255, method, ar.BINARY_INV, bs, 9, autoInvert=inv, out=dv)
        torch.cuda.synchronize()
        assert r is dv
        want = np.stack([ar.adaptive_threshold(p, 255, method, ar.BINARY_INV, bs, 9, auto_invert=inv) for p in pages])
        assert np.array_equal(dv.cpu().numpy(), want), (bs, method, inv)
        d = db.cpu().numpy()
        assert (d[:, h:] == 201).all() and (d[:, :, :3] == 201).all() and (d[:, :, 3 + w:] == 201).all(), "padding bytes of the destination written"
        s = sb.cpu().numpy()
        assert np.array_equal(s[:, :h, :w], pages) and (s[:, h:] == 7).all() and (s[:, :, w:] == 7).all()
        # a batch of different pages equals one call per page
        for i in range(n):
            assert np.array_equal(_dev(prl, pages[i], 255, method, ar.BINARY_INV, bs, 9, autoInvert=inv), want[i]), i
    # colour pages with strided rows through the composed entry
    rng = np.random.default_rng(2)
    col = rng.integers(0, 256, size=(3, h, w, 3), dtype=np.uint8)
    cb = torch.zeros((3, h + 2, w * 3 + 5), dtype=torch.uint8, device="cuda")
    cv = cb[:, :h, :w * 3].unflatten(2, (w, 3))
    cv.copy_(torch.from_numpy(col))
    got = prl.binarizeNativeAdaptive(cv).cpu().numpy()
    assert np.array_equal(got, np.stack([ar.binarize_native_adaptive(p) for p in col]))
    got = prl.binarizeAT(cv, 3, 255, 19, 9).cpu().numpy()
    assert np.array_equal(got, np.stack([ar.binarize_at(p, 3, 255, 19, 9) for p in col]))


def test_host_entry_numpy(prl, cuda_device):
    rng = np.random.default_rng(8)
    for shape in ((19, 23), (1, 1), (1, 40), (40, 1), (3, 200)):
        g = rng.integers(0, 256, size=shape, dtype=np.uint8)
        for bs, method in ((3, 0), (19, 1), (101, 1), (255, 0)):
            for inv in (False, True):
                got = prl.adaptiveThreshold(g, 255, method, ar.BINARY_INV, bs, 9, autoInvert=inv)
                assert np.array_equal(got, ar.adaptive_threshold(g, 255, method, ar.BINARY_INV, bs, 9, auto_invert=inv)), (shape, bs, method, inv)
        assert np.array_equal(prl.binarizeNativeAdaptive(g), ar.binarize_native_adaptive(g)), shape
    for c in (3, 4):
        img = rng.integers(0, 256, size=(33, 47, c), dtype=np.uint8)
        assert np.array_equal(prl.binarizeNativeAdaptive(img), ar.binarize_native_adaptive(img))
        assert np.array_equal(prl.binarizeNativeAdaptive(img, isAdaptiveThresholdCalculatedByGaussian=False, medianBlurKernelSize=7),
                              ar.binarize_native_adaptive(img, median=7, gaussian=False))
        assert np.array_equal(prl.binarizeAT(img, 5, 255, 19, 9), ar.binarize_at(img, 5, 255, 19, 9))
        assert np.array_equal(prl.binarizeAGT(img, 1, 200.4, 7, -3), ar.binarize_agt(img, 1, 200.4, 7, -3))
        assert np.array_equal(prl.binarizePureAdaptiveGaussian(img, 255, 21, 2), ar.binarize_pure_adaptive_gaussian(img, 255, 21, 2))
    view = rng.integers(0, 256, size=(30, 40, 3), dtype=np.uint8)[2:25, 3:31]   # strided rows
    assert np.array_equal(prl.binarizeAGT(view, 3, 255, 9, 4), ar.binarize_agt(view, 3, 255, 9, 4))


COLOUR = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "stages", "chain_*.npz")))
GRAY = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "scans", "*.npz")))


@pytest.mark.parametrize("path", COLOUR, ids=[os.path.basename(p)[6:-4] for p in COLOUR])
def test_reference_colour_scans(prl, cuda_device, path):
    import torch

    img = np.load(path)["bgr"]
    t = torch.from_numpy(img).cuda()
    med3 = median_ref.denoise_salt_pepper(img, 3, 1)
    want_native = ar.binarize_native_adaptive(img)
    assert np.array_equal(prl.binarizeNativeAdaptive(t).cpu().numpy(), want_native)
    assert np.array_equal(prl.binarizeNativeAdaptive(img), want_native)
    g3 = ar.bgr2gray(med3)
    assert np.array_equal(prl.binarizeAT(t, 3, 255, 19, 9).cpu().numpy(), ar.adaptive_threshold(g3, 255, ar.MEAN_C, ar.BINARY, 19, 9))
    assert np.array_equal(prl.binarizeAGT(t, 3, 255, 19, 9).cpu().numpy(), ar.adaptive_threshold(g3, 255, ar.GAUSSIAN_C, ar.BINARY, 19, 9))
    assert np.array_equal(prl.binarizePureAdaptiveGaussian(t, 255, 19, 9).cpu().numpy(), ar.binarize_pure_adaptive_gaussian(img, 255, 19, 9))


@pytest.mark.parametrize("path", GRAY, ids=[os.path.basename(p)[:-4] for p in GRAY])
def test_reference_gray_scans(prl, cuda_device, path):
    import torch

    g = np.load(path)["gray"]
    t = torch.from_numpy(g).cuda()
    b = median_ref.denoise_salt_pepper(g, 5, 1)
    assert np.array_equal(prl.binarizeNativeAdaptive(t).cpu().numpy(),
                          ar.adaptive_threshold(b, 255.0, ar.GAUSSIAN_C, ar.BINARY_INV, 19, 9.0, auto_invert=True))
    bs = ar.auto_block_size(*g.shape)
    if bs % 2 == 1:
        got = prl.binarizeNativeAdaptive(t, adaptiveThresholdingBlockSize=0).cpu().numpy()
        assert np.array_equal(got, ar.adaptive_threshold(b, 255.0, ar.GAUSSIAN_C, ar.BINARY_INV, bs, 9.0, auto_invert=True)), bs
    else:
        from prlib_amd import _capi

        with pytest.raises(_capi.PrlError) as e:
            prl.binarizeNativeAdaptive(t, adaptiveThresholdingBlockSize=0)
        assert e.value.status == _capi.PRL_ERR_BAD_WINDOW


def test_sizes_users_run(prl, cuda_device):
    import torch

    from prlib_amd import _capi, synth

    rng = np.random.default_rng(21)
    pages = np.stack([synth.page_numpy(3508, 2480, index=i) for i in range(8)])
    pages[5] = 255 - pages[5]   # a dark page: white ink on black
    t = torch.from_numpy(pages).cuda()
    got = prl.binarizeNativeAdaptive(t)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    for i in (0, 5):
        assert np.array_equal(got[i], ar.binarize_native_adaptive(pages[i])), i
    for i in range(8):
        assert np.array_equal(got[i], prl.binarizeNativeAdaptive(t[i]).cpu().numpy()), i
    assert ar.auto_block_size(3508, 2480) == 19
    assert np.array_equal(prl.binarizeNativeAdaptive(t, adaptiveThresholdingBlockSize=0).cpu().numpy(), got)
    del pages, got, t
    big = rng.integers(0, 256, size=(4096, 4096), dtype=np.uint8)
    big[1000:3000, 500:3500] = synth.page_numpy(2000, 3000, index=2)
    tb = torch.from_numpy(big).cuda()
    got = prl.binarizeNativeAdaptive(tb).cpu().numpy()
    assert np.array_equal(got, ar.binarize_native_adaptive(big))
    with pytest.raises(_capi.PrlError) as e:   # the automatic block size of a 4096 x 4096 page is 24
        prl.binarizeNativeAdaptive(tb, adaptiveThresholdingBlockSize=0)
    assert e.value.status == _capi.PRL_ERR_BAD_WINDOW


def test_cpp_dropin_on_device(prl, cuda_device, tmp_path):
    from test_adaptive_cpu import build_dropin

    exe = build_dropin(str(tmp_path))
    bgr = np.load(COLOUR[0])["bgr"][:400, :300]
    gray = np.ascontiguousarray(np.load(GRAY[0])["gray"][:600, :400])
    cases = [
        ("native", bgr, dict(median=5, mv=255.0, bs=19, shift=9.0, gaussian=1), ar.binarize_native_adaptive(bgr)),
        ("native", gray, dict(median=3, mv=200.5, bs=0, shift=-2.5, gaussian=0),
         ar.binarize_native_adaptive(gray, median=3, gaussian=False, max_value=200.5, bs=0, shift=-2.5)),
        ("at", bgr, dict(median=5, mv=255.0, bs=19, shift=9, gaussian=0), ar.binarize_at(bgr, 5, 255.0, 19, 9)),
        ("agt", bgr, dict(median=1, mv=255.0, bs=21, shift=-3, gaussian=1), ar.binarize_agt(bgr, 1, 255.0, 21, -3)),
        ("pag", bgr, dict(median=0, mv=180.0, bs=7, shift=4, gaussian=1), ar.binarize_pure_adaptive_gaussian(bgr, 180.0, 7, 4)),
    ]
    assert ar.auto_block_size(*gray.shape) % 2 == 1
    for i, (fn, img, p, want) in enumerate(cases):
        src, dst = tmp_path / f"{i}.raw", tmp_path / f"{i}.want"
        src.write_bytes(np.ascontiguousarray(img).tobytes())
        dst.write_bytes(np.ascontiguousarray(want).tobytes())
        h, w = img.shape[:2]
        c = img.shape[2] if img.ndim == 3 else 1
        r = subprocess.run([exe, "run", fn, str(h), str(w), str(c), str(src), str(dst), str(p["median"]), repr(p["mv"]), str(p["bs"]),
                            repr(p["shift"]), str(p["gaussian"])], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "adaptive dropin run: OK" in r.stdout, (fn, r.stdout + r.stderr)


def test_seeded_random_calls(prl, cuda_device):
    """300 calls drawn from one seed - function, parameters, size, batch and page kind - one after the other on one stream,
    so consecutive calls reuse one workspace at changing sizes; every mask against the restatement"""
    import torch

    from prlib_amd import synth

    rng = np.random.default_rng(20240607)
    stream = torch.cuda.Stream()
    for it in range(300):
        fn = int(rng.integers(0, 5))
        h, w = int(rng.integers(1, 150)), int(rng.integers(1, 330))
        n = int(rng.choice([1, 1, 2, 5]))
        bs = int(rng.choice([3, 5, 7, 9, 19, 21, 31, 61, 63, 101, 125, 255]))
        mv = float(rng.choice([255.0, 255.0, 128.0, 127.0, 0.0, 77.7]))
        delta = float(rng.choice([9.0, 0.0, -0.5, 0.5, -3.5, 300.0, -300.0]))
        med = int(rng.choice([1, 3, 5, 7, 9]))
        kind = int(rng.integers(0, 4))
        c = 1 if fn == 0 else int(rng.choice([3, 4])) if fn >= 2 else int(rng.choice([1, 3, 4]))
        if kind == 0:
            pages = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
        elif kind == 1:
            pages = np.stack([np.repeat(synth.page_numpy(h, w, index=int(rng.integers(0, 99)))[:, :, None], c, axis=2) for _ in range(n)])
            pages = pages ^ rng.integers(0, 4, size=pages.shape, dtype=np.uint8)
        elif kind == 2:
            pages = np.full((n, h, w, c), int(rng.integers(0, 256)), np.uint8)
        else:
            pages = np.repeat(np.stack([ar.stripes_page(h, w)] * n)[..., None], c, axis=3)
        if fn == 0:
            pages = pages[..., 0]   # gray pages N x H x W; the functions take N x H x W x C (3 dimensions would be one H x W x C page)
        with torch.cuda.stream(stream):
            t = torch.from_numpy(pages).cuda()
            if fn == 0:
                method, type_, inv = int(rng.integers(0, 2)), int(rng.integers(0, 2)), bool(rng.integers(0, 2))
                got = prl.adaptiveThreshold(t, mv, method, type_, bs, delta, autoInvert=inv)
                want = [ar.adaptive_threshold(p, mv, method, type_, bs, delta, auto_invert=inv) for p in pages]
            elif fn == 1:
                gaussian = bool(rng.integers(0, 2))
                k = max(med, 3)
                got = prl.binarizeNativeAdaptive(t, medianBlurKernelSize=k, isAdaptiveThresholdCalculatedByGaussian=gaussian,
                                                 adaptiveThresholdingMaxValue=mv, adaptiveThresholdingBlockSize=bs, adaptiveThresholdingShift=delta)
                want = [ar.binarize_native_adaptive(p, median=k, gaussian=gaussian, max_value=mv, bs=bs, shift=delta) for p in pages]
            elif fn == 2:
                got = prl.binarizeAT(t, med, mv, bs, int(delta))
                want = [ar.binarize_at(p, med, mv, bs, int(delta)) for p in pages]
            elif fn == 3:
                got = prl.binarizeAGT(t, med, mv, bs, int(delta))
                want = [ar.binarize_agt(p, med, mv, bs, int(delta)) for p in pages]
            else:
                got = prl.binarizePureAdaptiveGaussian(t, mv, bs, int(delta))
                want = [ar.binarize_pure_adaptive_gaussian(p, mv, bs, int(delta)) for p in pages]
        stream.synchronize()
        assert np.array_equal(got.cpu().numpy(), np.stack(want)), (it, fn, h, w, n, c, bs, mv, delta, med, kind)


def test_side_stream_beside_binarize(prl, oracle, cuda_device):
    """the new entries share the device workspace (scratch) with the other batch entries: a thread on its own stream runs
    them while another runs prl.binarize and prl.denoiseSaltPepper"""
    import torch

    from prlib_amd import synth

    rng = np.random.default_rng(77)
    a_pages = np.stack([synth.page_numpy(300, 420, index=i) for i in range(4)])
    col = rng.integers(0, 256, size=(3, 200, 260, 3), dtype=np.uint8)
    want_native = np.stack([ar.binarize_native_adaptive(p) for p in a_pages])
    want_at = np.stack([ar.binarize_at(p, 5, 255, 19, 9) for p in col])
    po = oracle.make_params(prl.SAUVOLA, 31, 0.2, 0)
    pp = prl.make_params(prl.SAUVOLA, 31, 0.2, 0)
    want_bin = np.stack([oracle.binarize(p, po) for p in a_pages])
    want_med = np.stack([median_ref.denoise_salt_pepper(p, 5, 2) for p in a_pages])
    bad = {"adaptive": 0, "other": 0}
    errors = []

    def adaptive_worker():
        try:
            s = torch.cuda.Stream(device=cuda_device)
            for _ in range(12):
                with torch.cuda.stream(s):
                    g1 = prl.binarizeNativeAdaptive(torch.from_numpy(a_pages).to(cuda_device))
                    g2 = prl.binarizeAT(torch.from_numpy(col).to(cuda_device), 5, 255, 19, 9)
                    s.synchronize()
                bad["adaptive"] += int((g1.cpu().numpy() != want_native).sum()) + int((g2.cpu().numpy() != want_at).sum())
        except BaseException as e:   # noqa: BLE001 - reported by the test
            errors.append(repr(e))

    def other_worker():
        try:
            s = torch.cuda.Stream(device=cuda_device)
            for _ in range(12):
                with torch.cuda.stream(s):
                    t = torch.from_numpy(a_pages).to(cuda_device)
                    g1 = prl.binarize(t, pp)
                    g2 = prl.denoiseSaltPepper(t, 5, 2)
                    s.synchronize()
                bad["other"] += int((g1.cpu().numpy() != want_bin).sum()) + int((g2.cpu().numpy() != want_med).sum())
        except BaseException as e:   # noqa: BLE001
            errors.append(repr(e))

    ts = [threading.Thread(target=adaptive_worker), threading.Thread(target=other_worker)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errors, errors
    assert bad == {"adaptive": 0, "other": 0}, bad
