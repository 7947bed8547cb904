"""GPU parity of the thinning step against the CPU oracle: boolean logic => bit-exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _mask(shape, seed, kind):
    from prlib_amd import synth

    rng = np.random.default_rng(seed)
    h, w = shape
    if kind == "doc":   # thinning treats white as foreground: invert a binarized page so strokes are white
        page = synth.page_numpy(h, w, index=seed)
        return np.where(page < 150, 255, 0).astype(np.uint8)
    if kind == "noise":
        return (rng.random((h, w)) < 0.55).astype(np.uint8) * 255
    if kind == "blobs":
        a = np.zeros((h, w), np.uint8)
        for _ in range(12):
            y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
            a[max(0, y - 9):y + 9, max(0, x - 14):x + 14] = 255
        return a
    if kind == "full":
        return np.full((h, w), 255, np.uint8)
    if kind == "odd_values":  # `&= 1`: only bit 0 counts
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    raise ValueError(kind)


@pytest.mark.parametrize("method", [0, 1], ids=["zhangsuen", "guohall"])
@pytest.mark.parametrize("shape", [(40, 60), (64, 64), (33, 97), (100, 31), (129, 257), (3, 50), (50, 2), (1, 1)])
def test_thinning_matches_oracle(prl, oracle, cuda_device, method, shape):
    import torch

    fn = prl.thinZhangSuen if method == 0 else prl.thinGuoHall
    kinds = ["doc", "noise", "blobs", "full", "odd_values"]
    imgs = [_mask(shape, seed=i + 1, kind=k) for i, k in enumerate(kinds)]
    got = fn(torch.from_numpy(np.stack(imgs)).to(cuda_device)).cpu().numpy()
    for i, img in enumerate(imgs):
        want = oracle.thin(img, method)
        assert np.array_equal(got[i], want), f"{kinds[i]}: {int((got[i] != want).sum())} mismatching pixels"


def test_thinning_in_place_host_entry_and_chain(prl, oracle, cuda_device):
    import torch

    img = _mask((120, 200), seed=9, kind="blobs")
    t = torch.from_numpy(img).to(cuda_device)
    prl.thinZhangSuen(t, out=t)                         # inputImage.data == outputImage.data branch (:73-76)
    assert np.array_equal(t.cpu().numpy(), oracle.thin(img, 0))
    assert np.array_equal(prl.thinGuoHall(img), oracle.thin(img, 1))   # host entry point
    # config-5 style hand-off on the device: Sauvola mask -> invert -> thinning, no host round trip
    from prlib_amd import synth

    page = synth.page_numpy(300, 400, index=3)
    mask = prl.binarizeSauvola(torch.from_numpy(page).to(cuda_device), 31, 0.34, 0)
    skel = prl.thinZhangSuen((255 - mask).contiguous())
    want = oracle.thin(255 - oracle.binarize(page, oracle.make_params(oracle.SAUVOLA, 31, 0.34, 0)), 0)
    assert np.array_equal(skel.cpu().numpy(), want)
    with pytest.raises(ValueError):
        prl.thinZhangSuen(np.zeros((0, 0), np.uint8))


def test_thinning_full_page(prl, oracle, cuda_device):
    import torch
    from prlib_amd import synth

    page = synth.page_numpy(1500, 2000, index=5)
    img = np.where(page < 150, 255, 0).astype(np.uint8)
    got = prl.thinGuoHall(torch.from_numpy(img).to(cuda_device)).cpu().numpy()
    assert np.array_equal(got, oracle.thin(img, 1))


@pytest.mark.parametrize("off", [1, 3, 5, 8])
def test_thinning_strided_views_keep_their_surroundings(prl, oracle, cuda_device, off):
    """ROI-style views (unaligned rows, step > width): aligned over-reads must not leak in, nothing may be written outside."""
    import torch

    h, w = 70, 123
    img = _mask((h, w), seed=4, kind="blobs") | _mask((h, w), seed=5, kind="doc")
    src = torch.full((2, h + 2, w + 16), 255, dtype=torch.uint8, device=cuda_device)   # odd surroundings = foreground
    dst = torch.full((2, h + 2, w + 16), 7, dtype=torch.uint8, device=cuda_device)
    src[:, 1:h + 1, off:off + w] = torch.from_numpy(img).to(cuda_device)
    prl.thinGuoHall(src[:, 1:h + 1, off:off + w], out=dst[:, 1:h + 1, off:off + w])
    got = dst.cpu().numpy()
    want = oracle.thin(img, 1)
    for i in range(2):
        assert np.array_equal(got[i, 1:h + 1, off:off + w], want)
        guard = got[i].copy()
        guard[1:h + 1, off:off + w] = 7
        assert (guard == 7).all()


@pytest.mark.parametrize("method", [0, 1], ids=["zhangsuen", "guohall"])
def test_thinning_many_passes_on_a_multi_tile_page(prl, oracle, cuda_device, method):
    """Thick blobs next to thin strokes: tens of passes, during most of which most tiles are idle (activity tracking)."""
    import torch

    h, w = 700, 4300            # three 1920-pixel strips, many row segments
    rng = np.random.default_rng(12)
    img = np.where(_mask((h, w), seed=2, kind="doc") > 0, 255, 0).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    for cy, cx, r in [(120, 300, 60), (400, 1900, 45), (600, 1925, 30), (350, 4200, 80), (20, 2500, 25)]:
        img[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 255
    img[500:560, 3000:3600] = 255                      # a thick bar inside the second strip (columns 1920 .. 3839)
    img[230:270, 1700:2150] = 255                      # bars across the strip boundaries at x = 1920 and x = 3840
    img[610:650, 3700:3990] = 255
    img[rng.random((h, w)) < 0.001] = 255
    fn = prl.thinZhangSuen if method == 0 else prl.thinGuoHall
    got = fn(torch.from_numpy(img).to(cuda_device)).cpu().numpy()
    want, passes = oracle.thin(img, method, return_passes=True)
    assert passes > 20
    assert np.array_equal(got, want), f"{int((got != want).sum())} mismatching pixels after {passes} passes"


@pytest.mark.parametrize("seed", range(int(__import__("os").environ.get("PRL_SWEEP_SEEDS", "12"))))
def test_thinning_random_sweep(prl, oracle, cuda_device, seed):
    """Seeded random shapes (word- and strip-ragged), densities and both methods, as a batch of two pages."""
    import torch

    rng = np.random.default_rng(9000 + seed)
    h, w = int(rng.integers(1, 200)), int(rng.integers(1, 2300))
    method = int(rng.integers(0, 2))
    kinds = ["noise", "blobs", "doc", "full", "odd_values"]
    imgs = [_mask((h, w), seed=seed * 3 + i, kind=kinds[int(rng.integers(0, len(kinds)))]) for i in range(2)]
    fn = prl.thinZhangSuen if method == 0 else prl.thinGuoHall
    got = fn(torch.from_numpy(np.stack(imgs)).to(cuda_device)).cpu().numpy()
    for i in range(2):
        want = oracle.thin(imgs[i], method)
        assert np.array_equal(got[i], want), f"seed {seed} page {i}: {int((got[i] != want).sum())} mismatches ({h}x{w}, method {method})"


@pytest.mark.parametrize("method", [0, 1])
def test_thinning_needs_more_passes_than_the_page_is_large(prl, oracle, cuda_device, method):
    """a 2-pixel-thick zigzag erodes from its free ends only, about one row per pass and end; on a small page
    that takes more passes than max(width, height) + 2, the cap round 1 used.  No cap now: the loop runs until a pass
    changes nothing, as the reference's do-while does."""
    import torch

    h, w = 40, 24
    img = np.zeros((h, w), np.uint8)
    x, dx = 3, 1
    for y in range(2, h - 2):       # 2-pixel-thick diagonal bouncing between the margins
        img[y, x:x + 2] = 255
        x += dx
        if x >= w - 5 or x <= 3:
            dx = -dx
    want, passes = oracle.thin(img, method, return_passes=True)
    got = (prl.thinZhangSuen if method == 0 else prl.thinGuoHall)(torch.from_numpy(img).to(cuda_device)).cpu().numpy()
    assert np.array_equal(got, want), passes
    # a long thin stroke on a wide, very low page: passes > max(w, h) + 2 by construction is hard to hit in general, so also
    # check a page where the oracle itself reports many passes
    big = np.zeros((12, 300), np.uint8)
    big[4:8, 5:295] = 255
    want, passes = oracle.thin(big, method, return_passes=True)
    got = (prl.thinZhangSuen if method == 0 else prl.thinGuoHall)(torch.from_numpy(big).to(cuda_device)).cpu().numpy()
    assert np.array_equal(got, want), passes
