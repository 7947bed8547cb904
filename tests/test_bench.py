"""bench.py's plain run and --dump-outputs: a plain run times the steps and prints the headline line without the --full legs;
the dumped masks are the last timed step's, bounded in size, and the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fake_masks(n, h, pitch, seed):
    import torch

    return torch.from_numpy(np.random.default_rng(seed).choice(np.array([0, 255], np.uint8), (n, h, pitch)))


def test_dump_outputs_writes_the_whole_batch_when_it_fits(tmp_path):
    import bench

    n, h, w = 2, 30, 40
    out = _fake_masks(n, h, 64, 3)
    bench.dump_outputs(str(tmp_path), out, n, h, w)
    mask, counts = np.load(tmp_path / "mask.npy"), np.load(tmp_path / "mask_row_counts.npy")
    assert mask.dtype == np.float32 and counts.dtype == np.float32
    assert np.array_equal(mask, out.numpy()[:, :, :w].astype(np.float32))     # (the pitch padding is not the caller's)
    assert np.array_equal(counts, (out.numpy()[:, :, :w] != 0).sum(axis=2).astype(np.float32))


def test_dump_outputs_samples_a_large_batch_within_the_budget(tmp_path, monkeypatch):
    import bench

    monkeypatch.setattr(bench, "DUMP_BYTES", 40_000)
    n, h, w = 3, 50, 70                                    # 42 000 B of float32 masks: more than half the budget
    out = _fake_masks(n, h, 128, 4)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), out, n, h, w)
    mask, counts = np.load(tmp_path / "a" / "mask.npy"), np.load(tmp_path / "a" / "mask_row_counts.npy")
    assert mask.nbytes + counts.nbytes <= 40_000
    idx = np.unique(np.random.default_rng(0).integers(0, n * h * w, 20_000 // 4, dtype=np.int64))
    assert np.array_equal(mask, out.numpy()[:, :, :w].reshape(-1)[idx].astype(np.float32))
    assert counts.shape == (n, h) and np.array_equal(counts, (out.numpy()[:, :, :w] != 0).sum(axis=2).astype(np.float32))
    for f in ("mask.npy", "mask_row_counts.npy"):          # a fixed sample: the same positions every run
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(prl, oracle, cuda_device, tmp_path):
    from prlib_amd import synth

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--pages", "3",
                        "--size", "1024", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "Mpixels/s" and d["higher_is_better"] is True and d["dtype"].startswith("u8")
    # the --full legs did not run
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["worst_case"] is None and d["end_to_end"] is None
    assert d["parity"]["checked_pages"] == [] and d["parity"]["mismatching_pixels"] is None

    params = prl.make_params(prl.SAUVOLA, 31, 0.34, 0)
    g = prl.geometry(params, 1024, 1024)
    mask = np.load(tmp_path / "mask.npy")
    assert mask.dtype == np.float32 and mask.shape == (3, g.out_h, g.out_w)
    pages = synth.pages_torch(3, 1024, 1024, cuda_device, seed=1000).cpu().numpy()   # bench.py's pages (seed 1000 + first page)
    want = oracle.binarize_batch(pages.copy(), oracle.make_params(prl.SAUVOLA, 31, 0.34, 0), threads=3)
    assert np.array_equal(mask, want.astype(np.float32))
    counts = np.load(tmp_path / "mask_row_counts.npy")
    assert np.array_equal(counts, (want != 0).sum(axis=2).astype(np.float32))
