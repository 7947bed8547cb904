"""The cases of tests/bgnorm_cases.py on the CPU: oracle.bgnorm equals the independent numpy model on every one (0 differing bytes),
and every case has the feature it is named for - read from the oracle's stage entries and from plain numpy tile counts."""
import numpy as np
import pytest

import bgnorm_cases as bc
from oracle import numpy_model

CASES = bc.all_cases()
IDS = [x["name"] for x in CASES]


def test_names_are_unique_and_every_list_is_covered():
    assert len(set(IDS)) == len(IDS)
    maps = [x for x in CASES if x["stage"] == "map"]
    assert {x["extra"] for x in maps} == {(False, False), (True, False), (False, True), (True, True)}
    assert {-(-x["page"].shape[1] // bc.SX) for x in maps} >= {257, 513}
    assert max(x["page"].shape[1] for x in CASES) == 5130 and max(x["page"].shape[0] for x in CASES) <= 135
    for kind in ("columns", "pixels"):
        seam = [x for x in CASES if x["name"].startswith("seam_" + kind)]
        assert [x["page"].shape[1] for x in seam] == bc.TILE_WIDTHS
        assert {1 if x["page"].ndim == 2 else x["page"].shape[2] for x in seam} == {1, 3, 4}
    assert sum(x["name"].startswith("edge_") for x in CASES) == 15
    for c, widths in ((1, bc.APPLY_GRAY_WIDTHS), (3, bc.APPLY_COLOUR_WIDTHS), (4, bc.APPLY_COLOUR_WIDTHS)):
        assert [x["page"].shape[1] for x in CASES if x["stage"] == "apply" and x["name"].endswith(f"_c{c}")] == widths


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_equals_the_numpy_model(oracle, case):
    page = case["page"]
    want = numpy_model.bgnorm_model(page)
    got = oracle.bgnorm(page)
    assert got.shape == want.shape and np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_has_its_feature(oracle, case):
    page = case["page"]
    cnt, fg = bc.tile_counts(oracle, page)
    h, w = fg.shape
    good = cnt >= bc.MINCOUNT
    failed = bc.oracle_failed(oracle, page)
    assert failed == case["failed"]
    out = oracle.bgnorm(page)
    if failed:
        assert np.array_equal(out, page if page.ndim == 2 else page[:, :, :3])
    else:
        assert not np.array_equal(out, page if page.ndim == 2 else page[:, :, :3])
    if "extra" in case:
        assert (w % bc.SX > 0, h % bc.SY > 0) == case["extra"]
    if "zero_tiles" in case:
        assert sorted((int(i), int(j)) for i, j in zip(*np.nonzero(~good))) == sorted(case["zero_tiles"])
    if "missing" in case:
        assert [j for j in range(cnt.shape[1]) if not good[:, j].any()] == case["missing"]
        if not case["failed"]:
            assert good.any()
    for (i, j), n in case.get("counts", {}).items():
        assert cnt[i, j] == n
        raw = bc.oracle_raw_maps(oracle, page)
        assert all((raw[ch, i, j] != 0) == (n >= bc.MINCOUNT) for ch in range(raw.shape[0]))
    if case.get("marks"):
        assert fg.any() and not case["failed"]
    if case.get("no_foreground"):
        assert not fg.any() and (page.min(axis=(0, 1)) < bc.THRESH).any()
    if case.get("clamp"):
        # blockconvLow's corner: one row x two columns of the 3 x 5 window, rescaled by 3 / 1 and 5 / 2 in float32
        _, m = oracle.bgnorm_bgmap(page, 0)
        val = np.float32(int(np.float64(np.float32(1.0 / 15) * np.float32(int(m[1, 1]) + int(m[1, 2]))) + 0.5))
        tv = val * (np.float32(3) / np.float32(1)) * (np.float32(5) / np.float32(2))
        assert tv >= np.float32(255.0)
        assert oracle.bgnorm_blockconv(m)[0, 0] == 255 and oracle.bgnorm_invmap(m)[1][0, 0] == 51200 // 255


def test_mixed_and_small_batches(oracle):
    pages, fails = bc.mixed_batch()
    assert len({p.shape for p in pages}) == 1 and pages[0].shape[2] == 4
    for p, f in zip(pages, fails):
        assert bc.oracle_failed(oracle, p) == f
        assert np.array_equal(oracle.bgnorm(p), p[:, :, :3]) == f
        assert np.array_equal(oracle.bgnorm(p), numpy_model.bgnorm_model(p))
    for p in bc.small_batch():
        assert bc.oracle_failed(oracle, p) and np.array_equal(oracle.bgnorm(p), p[:, :, :3])
    for c in (1, 3, 4):
        for p in bc.view_pages(c):
            assert not bc.oracle_failed(oracle, p)
            assert np.array_equal(oracle.bgnorm(p), numpy_model.bgnorm_model(p))
