"""GPU parity of the NL-means stage (prl::denoise) against the CPU oracle.

The NLM core is integer arithmetic => bit-exact.  The Lab conversions are restated identically on both
sides (integer forward, float32 inverse with one rounding per operation) => also compared bit-exactly;
the documented tolerance of 1 LSB/channel is against a *real* OpenCV build, which is not available.

These tests call the public entries at a few strengths.  tests/test_nlm_gpu.py runs every kernel instantiation by name at the edges
of the weight table's length, both Lab conversions on all 2^24 triples, and strided / odd-addressed views of the C entries.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _noisy(shape, seed, sigma=12.0, channels=None):
    from prlib_amd import synth

    rng = np.random.default_rng(seed)
    h, w = shape
    base = synth.page_numpy(h, w, index=seed).astype(np.float64)
    if channels is None:
        return np.clip(np.rint(base + rng.normal(0, sigma, (h, w))), 0, 255).astype(np.uint8)
    img = base[:, :, None] + rng.normal(0, sigma, (h, w, channels))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("shape", [(64, 64), (70, 130), (33, 47), (129, 65), (20, 200)])
@pytest.mark.parametrize("h", [3.0, 10.0])
def test_nlm_one_plane(prl, oracle, cuda_device, shape, h):
    import torch

    img = _noisy(shape, seed=1)
    got = prl.nlm_planes(torch.from_numpy(img).to(cuda_device), h).cpu().numpy()
    want = oracle.nlm_planes(img, h, threads=8)
    assert np.array_equal(got, want), f"{int((got != want).sum())} mismatching pixels"


@pytest.mark.parametrize("channels,h", [(2, 3.0), (2, 7.5), (3, 5.0)])
def test_nlm_interleaved_planes(prl, oracle, cuda_device, channels, h):
    import torch

    img = _noisy((75, 101), seed=2, sigma=6.0, channels=channels)
    got = prl.nlm_planes(torch.from_numpy(img).to(cuda_device), h).cpu().numpy()
    want = oracle.nlm_planes(img, h, threads=8)
    assert np.array_equal(got, want), f"{int((got != want).sum())} mismatching samples"


def test_nlm_tiny_and_flat_pages(prl, oracle, cuda_device):
    import torch

    for img in [np.full((9, 11), 77, np.uint8), np.zeros((5, 70), np.uint8), _noisy((14, 15), seed=3)]:
        got = prl.nlm_planes(torch.from_numpy(img).to(cuda_device), 10.0).cpu().numpy()
        assert np.array_equal(got, oracle.nlm_planes(img, 10.0))


def test_nlm_large_h_uses_global_table(prl, oracle, cuda_device):
    import torch

    img = _noisy((48, 64), seed=4, sigma=25.0)
    got = prl.nlm_planes(torch.from_numpy(img).to(cuda_device), 40.0).cpu().numpy()   # > 1024 non-zero weights
    assert np.array_equal(got, oracle.nlm_planes(img, 40.0))


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("strength", [5.5, 10.0])
def test_denoise_colored(prl, oracle, cuda_device, channels, strength):
    import torch

    img = _noisy((90, 120), seed=5, sigma=15.0, channels=channels)
    batch = np.stack([img, img[::-1].copy()])
    got = prl.denoise(torch.from_numpy(batch).to(cuda_device), strength).cpu().numpy()
    for i in range(2):
        want = oracle.denoise(batch[i], strength, threads=8)
        assert np.array_equal(got[i], want), f"page {i}: max diff {np.abs(got[i].astype(int) - want).max()}"
    # host entry point (prl::denoise's default strength)
    got_h = prl.denoise(img)
    assert np.array_equal(got_h, oracle.denoise(img, 5.5, threads=8))


def test_denoise_rejects_other_channel_counts(prl, cuda_device):
    from prlib_amd import _capi

    with pytest.raises(_capi.PrlError) as e:
        prl.denoise(np.zeros((10, 10, 1), np.uint8))
    assert e.value.status == _capi.PRL_ERR_BAD_CHANNELS


def test_golden_nlm_fixture_on_device(prl, cuda_device):
    import os

    import torch

    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nlm_0050_crop.npz"))
    lab = z["lab"]
    dev_l = torch.from_numpy(np.ascontiguousarray(lab[:, :, 0])).to(cuda_device)
    dev_ab = torch.from_numpy(np.ascontiguousarray(lab[:, :, 1:])).to(cuda_device)
    assert np.array_equal(prl.nlm_planes(dev_l, 10.0).cpu().numpy(), z["l_h10"])
    assert np.array_equal(prl.nlm_planes(dev_ab, 3.0).cpu().numpy(), z["ab_h3"])
    assert np.array_equal(prl.denoise(torch.from_numpy(z["noisy"]).to(cuda_device), 10.0).cpu().numpy(), z["denoised_s10"])


@pytest.mark.parametrize("seed", range(int(__import__("os").environ.get("PRL_SWEEP_SEEDS", "12"))))
def test_nlm_random_sweep(prl, oracle, cuda_device, seed):
    """Seeded random shapes (tile-ragged, narrower than the halo), channel counts, strengths and noise levels."""
    import torch

    rng = np.random.default_rng(7000 + seed)
    h, w = int(rng.integers(1, 150)), int(rng.integers(1, 200))
    channels = int(rng.choice([1, 1, 2, 2, 3]))
    strength = float(rng.choice([1.0, 3.0, 5.5, 10.0, 14.0, 25.0]))
    sigma = float(rng.choice([0.0, 4.0, 15.0, 40.0]))
    img = _noisy((h, w), seed=seed, sigma=sigma, channels=None if channels == 1 else channels)
    got = prl.nlm_planes(torch.from_numpy(img).to(cuda_device), strength).cpu().numpy()
    want = oracle.nlm_planes(img, strength, threads=8)
    assert np.array_equal(got, want), f"seed {seed}: {int((got != want).sum())} mismatches ({h}x{w}x{channels}, h={strength}, sigma={sigma})"
    if seed % 3 == 0:  # the colour pipeline on the same geometry
        c = 3 + (seed % 2)
        col = _noisy((h, w), seed=seed + 1, sigma=sigma, channels=c)
        got = prl.denoise(torch.from_numpy(col).to(cuda_device), strength).cpu().numpy()
        assert np.array_equal(got, oracle.denoise(col, strength, threads=8))


def test_weight_table_cache_survives_interleaved_calls(prl, oracle, cuda_device):
    """The NL-means weight tables are cached in a workspace the binarizers also use: same / different strengths with
    binarizer calls in between must keep giving the oracle's result."""
    import torch
    from prlib_amd import synth

    col = _noisy((60, 90), seed=21, sigma=10.0, channels=3)
    t = torch.from_numpy(col).to(cuda_device)
    page = torch.from_numpy(synth.page_numpy(300, 400, index=2)).to(cuda_device)
    want10, want4 = oracle.denoise(col, 10.0, threads=8), oracle.denoise(col, 4.0, threads=8)
    for strength, want in [(10.0, want10), (10.0, want10), (4.0, want4), (10.0, want10)]:
        assert np.array_equal(prl.denoise(t, strength).cpu().numpy(), want)
        prl.binarizeSauvola(page, 31, 0.34, 2)          # overwrites the shared workspace
        assert np.array_equal(prl.denoise(t, strength).cpu().numpy(), want)


def test_nlm_more_pages_than_one_grid_dimension(prl, oracle, cuda_device):
    """70 000 tiny pages: the per-page grid dimension holds 65 535, so the launch is chunked."""
    import torch

    rng = np.random.default_rng(0)
    pages = rng.integers(0, 256, (70000, 6, 7), dtype=np.uint8)
    got = prl.nlm_planes(torch.from_numpy(pages[..., None]).to(cuda_device), 10.0).cpu().numpy()[..., 0]   # N x H x W x 1
    for i in (0, 1, 65534, 65535, 65536, 69999):
        assert np.array_equal(got[i], oracle.nlm_planes(pages[i], 10.0)), i
