"""GPU parity of prl::backgroundNormalization against the CPU oracle: bit-exact."""
import glob
import os

import numpy as np
import pytest

from prlib_amd import synth

pytestmark = pytest.mark.gpu

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "0*.npz")))


def _gray_cases():
    yield "synthetic", synth.page_numpy(203, 317, index=11)
    yield "text_shaded", synth.text_page_numpy(330, 250, 3, skew_deg=1.5, shading=0.6)
    p = synth.page_numpy(150, 200, index=5)
    p[30:110, 40:160] = 20
    yield "holes", p
    p = synth.page_numpy(160, 120, index=6)
    p[:, :35] = 10
    p[:, 95:] = 0
    yield "missing_columns", p
    yield "flat", np.full((90, 70), 100, np.uint8)
    yield "all_dark", np.full((90, 80), 30, np.uint8)                # map not made -> copy
    yield "too_small_map", synth.page_numpy(60, 49, index=1)         # 4 x 4 tiles -> copy
    yield "no_complete_tile", synth.page_numpy(14, 9, index=1)
    yield "exact_multiple", synth.page_numpy(150, 100, index=2)      # no incomplete tile row / column
    yield "one_px", np.array([[200]], np.uint8)
    yield "wide", synth.text_page_numpy(80, 1300, 4, shading=0.3)    # several 250-column workgroups per tile row
    yield "minimal", synth.page_numpy(75, 50, index=3)               # exactly 5 x 5 tiles


@pytest.mark.parametrize("name,page", list(_gray_cases()), ids=[n for n, _ in _gray_cases()])
def test_bgnorm_gray_matches_oracle(prl, oracle, cuda_device, name, page):
    import torch

    got = prl.backgroundNormalization(torch.from_numpy(page).to(cuda_device)).cpu().numpy()
    want = oracle.bgnorm(page)
    assert got.shape == want.shape and np.array_equal(got, want), f"{name}: {(got != want).sum()} bytes differ"


@pytest.mark.parametrize("c", [3, 4])
def test_bgnorm_colour_batch_matches_oracle(prl, oracle, cuda_device, c):
    import torch

    rng = np.random.default_rng(c)
    pages = []
    for i in range(3):
        g = synth.text_page_numpy(211, 167, 10 + i, skew_deg=i, shading=0.5)
        col = np.stack([g, np.clip(g.astype(int) + 10, 0, 255).astype(np.uint8), g // 2 + 100] +
                       ([rng.integers(0, 256, g.shape, dtype=np.uint8)] if c == 4 else []), axis=-1)
        pages.append(col)
    pages.append(rng.integers(0, 256, pages[0].shape, dtype=np.uint8))   # noise: many tiles below mincount
    batch = np.stack(pages)
    got = prl.backgroundNormalization(torch.from_numpy(batch).to(cuda_device)).cpu().numpy()
    assert got.shape == batch.shape[:3] + (3,)
    for i in range(len(pages)):
        want = oracle.bgnorm(batch[i])
        assert np.array_equal(got[i], want), f"page {i}: {(got[i] != want).sum()} bytes differ"


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_bgnorm_reference_test_images(prl, oracle, cuda_device, path):
    """The reference's own test_data/binarize images (inputs held in tests/golden/*.npz)."""
    import torch

    img = np.load(path)["gray"]
    got = prl.backgroundNormalization(torch.from_numpy(img).to(cuda_device)).cpu().numpy()
    assert np.array_equal(got, oracle.bgnorm(img))


def test_bgnorm_views_and_host_entry(prl, oracle, cuda_device):
    import torch

    # a pitched batch (row step > width) and an output with its own pitch, guard bytes untouched
    pages = np.stack([synth.text_page_numpy(95, 131, i, shading=0.4) for i in range(3)])
    big = torch.full((3, 95, 160), 7, dtype=torch.uint8, device=cuda_device)
    big[:, :, 3:134] = torch.from_numpy(pages).to(cuda_device)
    from prlib_amd import _capi
    L = _capi.lib()
    out = torch.full((3, 95, 144), 9, dtype=torch.uint8, device=cuda_device)
    src = big[:, :, 3:134]
    dst = out[:, :, 5:136]
    _capi.check(L.prl_hip_bgnorm_batch_device(3, 1, src.data_ptr(), src.stride(0), src.stride(1), 131, 95, dst.data_ptr(),
                                              dst.stride(0), dst.stride(1), torch.cuda.current_stream().cuda_stream))
    o = out.cpu().numpy()
    for i in range(3):
        assert np.array_equal(o[i, :, 5:136], oracle.bgnorm(pages[i]))
    o[:, :, 5:136] = 9
    assert (o == 9).all()
    # host entry (what the cv::Mat wrapper calls), gray and colour
    assert np.array_equal(prl.backgroundNormalization(pages[0]), oracle.bgnorm(pages[0]))
    col = np.stack([pages[1], pages[2], pages[0]], axis=-1)
    assert np.array_equal(prl.backgroundNormalization(col), oracle.bgnorm(col))


def test_bgnorm_argument_errors(prl, cuda_device):
    import torch

    from prlib_amd import _capi
    L = _capi.lib()
    t = torch.zeros((10, 10), dtype=torch.uint8, device=cuda_device)
    assert L.prl_hip_bgnorm_batch_device(1, 1, t.data_ptr(), 100, 10, 0, 10, t.data_ptr(), 100, 10, None) == _capi.PRL_ERR_EMPTY
    assert L.prl_hip_bgnorm_batch_device(1, 2, t.data_ptr(), 100, 10, 5, 10, t.data_ptr(), 100, 10, None) == _capi.PRL_ERR_BAD_CHANNELS
    assert L.prl_hip_bgnorm_batch_device(1, 1, t.data_ptr(), 100, 4, 5, 10, t.data_ptr(), 100, 10, None) == _capi.PRL_ERR_BAD_ARG
    assert L.prl_hip_bgnorm_out_channels(1) == 1 and L.prl_hip_bgnorm_out_channels(3) == 3 and L.prl_hip_bgnorm_out_channels(4) == 3


# ---- kernel by kernel: the cases of tests/bgnorm_cases.py (each shown on the CPU to have its feature: tests/test_bgnorm_cpu.py) -------
import bgnorm_cases as bc  # noqa: E402

CASES = bc.all_cases()
# what runs again on the global-memory path of k_bg_maps: the map stage's cases and two colour cases of the tile stage
LDS0_CASES = [x["name"] for x in CASES if x["stage"] == "map"] + ["dark_red_and_blue_only", "mincount_40_tile24_c4"]


@pytest.mark.parametrize("stage", ["map", "tile", "apply"])
def test_bgnorm_cases_match_oracle(prl, oracle, cuda_device, stage):
    """every case through the public entry: 0 differing bytes"""
    import torch

    mine = [x for x in CASES if x["stage"] == stage]
    assert len(mine) >= 17
    for x in mine:
        got = prl.backgroundNormalization(torch.from_numpy(x["page"]).to(cuda_device)).cpu().numpy()
        want = oracle.bgnorm(x["page"])
        assert got.shape == want.shape and np.array_equal(got, want), f"{x['name']}: {(got != want).sum()} bytes differ"


def maps_row(oracle, case, out, raw, inv, fail):
    """What the tests assert on, for one case run through the hooks entry (runs in the child): the differing bytes of the page, of
    the raw tile maps against numpy tile averages outside the oracle's foreground mask, and of the inverse maps against the
    oracle's; the fail flag and the oracle's."""
    page = case["page"]
    failed, want_inv = bc.oracle_inv_maps(oracle, page)
    want_raw = bc.oracle_raw_maps(oracle, page)
    row = dict(name=case["name"], out_bad=int((out != oracle.bgnorm(page)).sum()), raw_shape=list(raw.shape) == list(want_raw.shape),
               raw_bad=int((raw != want_raw).sum()), raw_nonzero=int((want_raw != 0).sum()), fail_dev=int(fail), fail_ref=int(failed))
    row["inv_bad"] = 0 if failed else int((inv != want_inv).sum())
    return row


_MAPS_CHILD = r'''
import ctypes as C, json, sys
import numpy as np, torch
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from prlib_amd import _capi
_capi.use_library(_capi.HOOKS_LIB_PATH)
from oracle import capi as oracle
import test_bgnorm_gpu as T
L = _capi.lib()
vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
L.prl_hip_internal_bgnorm_maps.argtypes = [i, i, vp, sz, sz, i, i, vp, sz, sz, vp, vp, vp, vp]
dev = torch.device("cuda:0")
_capi.check(L.prl_hip_set_device(0))
stream = torch.cuda.current_stream(dev).cuda_stream
names = %(names)r
rows = []
for case in T.CASES:
    if names is not None and case["name"] not in names:
        continue
    page = case["page"]
    h, w = page.shape[:2]
    c = 1 if page.ndim == 2 else page.shape[2]
    och = 1 if c == 1 else 3
    mh, mw = -(-h // 15), -(-w // 10)
    src = torch.from_numpy(page).to(dev)
    dst = torch.full((h, w, och), 9, dtype=torch.uint8, device=dev)
    raw = torch.full((och, mh, mw), 3, dtype=torch.uint8, device=dev)
    inv = torch.full((och, mh, mw), 5, dtype=torch.int16, device=dev)
    fail = torch.full((1,), -1, dtype=torch.int32, device=dev)
    _capi.check(L.prl_hip_internal_bgnorm_maps(1, c, src.data_ptr(), h * w * c, w * c, w, h, dst.data_ptr(), h * w * och, w * och,
                                               raw.data_ptr(), inv.data_ptr(), fail.data_ptr(), stream))
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    rows.append(T.maps_row(oracle, case, out[:, :, 0] if c == 1 else out, raw.cpu().numpy(), inv.cpu().numpy().view(np.uint16),
                           int(fail.cpu().numpy()[0])))
# more than one chunk of pages, or a missing output, is an argument error of the entry
one = torch.zeros((1, 4, 4), dtype=torch.uint8, device=dev)
m8 = torch.zeros((16,), dtype=torch.int32, device=dev)
errs = [L.prl_hip_internal_bgnorm_maps(16385, 1, one.data_ptr(), 0, 4, 4, 4, one.data_ptr(), 0, 4, m8.data_ptr(), m8.data_ptr(), m8.data_ptr(), stream),
        L.prl_hip_internal_bgnorm_maps(1, 1, one.data_ptr(), 16, 4, 4, 4, one.data_ptr(), 16, 4, None, m8.data_ptr(), m8.data_ptr(), stream),
        L.prl_hip_internal_bgnorm_maps(1, 2, one.data_ptr(), 16, 4, 2, 4, one.data_ptr(), 16, 4, m8.data_ptr(), m8.data_ptr(), m8.data_ptr(), stream)]
torch.cuda.synchronize()
print("ROWS " + json.dumps(dict(rows=rows, errs=errs)))
'''
_maps_result = {}


def _maps_child(variant):
    """The rows of the one child of a variant ("default": every case; "lds0": LDS0_CASES with PRL_HIP_BGNORM_LDS_MAP=0), run once per
    session.  A child that died (signal, abort, GPU fault, time limit) fails its test and every later one of the variant without
    another process being started."""
    import json
    import subprocess
    import sys
    import time

    if variant in _maps_result:
        assert not isinstance(_maps_result[variant], str), f"the child failed before and is not started again: {_maps_result[variant]}"
        return _maps_result[variant]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = None if variant == "default" else LDS0_CASES
    code = _MAPS_CHILD % dict(root=root, tests=os.path.join(root, "tests"), names=names)
    env = {k: v for k, v in os.environ.items() if k != "PRL_HIP_BGNORM_LDS_MAP"}
    if variant == "lds0":
        env["PRL_HIP_BGNORM_LDS_MAP"] = "0"
    _maps_result[variant] = "did not finish"
    t0 = time.time()
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env)
    print(f"bgnorm maps child ({variant}): {time.time() - t0:.1f} s")
    if r.returncode != 0 or "illegal memory access" in r.stderr:
        _maps_result[variant] = f"exit {r.returncode}: {r.stderr[-2000:]}"
    assert r.returncode == 0 and "illegal memory access" not in r.stderr, (r.returncode, r.stdout[-2000:] + r.stderr[-2000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("ROWS ")]
    assert lines, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(lines[0][5:])
    assert [x["name"] for x in res["rows"]] == ([x["name"] for x in CASES] if names is None else [x["name"] for x in CASES if x["name"] in names])
    _maps_result[variant] = res
    return res


def test_hook_raw_tile_maps(prl, cuda_device):
    """k_bg_tiles alone: the maps as it left them, copied before k_bg_maps fills them in, equal sum // count of the pixels outside
    the oracle's foreground mask per complete tile, 0 where fewer than 40 remain and in the row and column of incomplete tiles."""
    rows = _maps_child("default")["rows"]
    for x in rows:
        assert x["raw_shape"] and x["raw_bad"] == 0, x
    assert sum(x["raw_nonzero"] > 0 for x in rows) >= len(rows) - 3     # (all but the pages without a good tile)


def test_hook_inverse_maps_and_fail_flags(prl, cuda_device):
    """k_bg_maps alone: the u16 inverse maps equal the oracle's bgnorm_bgmap -> bgnorm_invmap on every page whose map can be made; the
    fail flag equals the oracle's; the page the same call wrote equals oracle.bgnorm."""
    res = _maps_child("default")
    by_name = {x["name"]: x for x in CASES}
    for x in res["rows"]:
        assert x["fail_dev"] == x["fail_ref"] == int(by_name[x["name"]]["failed"]), x
        assert x["inv_bad"] == 0 and x["out_bad"] == 0, x
    assert sum(x["fail_ref"] for x in res["rows"]) == sum(x["failed"] for x in CASES) >= 5
    assert res["errs"] == [5, 5, 3]     # PRL_ERR_BAD_ARG twice, PRL_ERR_BAD_CHANNELS


def test_global_memory_map_path(prl, cuda_device):
    """PRL_HIP_BGNORM_LDS_MAP=0 (test-hooks build): k_bg_maps works on the map in global memory, as it does in the product for maps
    above 60000 bytes.  Pages, raw maps, inverse maps and fail flags equal the oracle's, hence the default path's."""
    rows = _maps_child("lds0")["rows"]
    assert len(rows) == len(LDS0_CASES)
    for x in rows:
        assert x["raw_shape"] and x["raw_bad"] == 0 and x["inv_bad"] == 0 and x["out_bad"] == 0 and x["fail_dev"] == x["fail_ref"], x


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("dst_off", [0, 1, 2, 3])
def test_bgnorm_unaligned_views_and_guard_bytes(prl, oracle, cuda_device, c, dst_off):
    """Source pages that are views at byte offset 0 .. 3 into random bytes with an odd pitch, into a destination view at byte offset
    0 .. 3 with an odd pitch in a buffer of 7s: the oracle's pages, and every byte outside them still 7."""
    import torch

    from prlib_amd import _capi

    pages = bc.view_pages(c)
    n, h, w, och = len(pages), bc.VIEW_H, bc.VIEW_W, 1 if c == 1 else 3
    src_off = (3 * dst_off + 1) % 4
    rng = np.random.default_rng(70 + dst_off)
    s_step = w * c + 5
    s_step += 1 - s_step % 2                    # odd
    s_page = h * s_step + 11
    d_step = w * och + 7
    d_step += 1 - d_step % 2                    # odd
    d_page = h * d_step + 13
    assert s_step % 2 == 1 and d_step % 2 == 1
    src = rng.integers(0, 256, src_off + n * s_page + 64, dtype=np.uint8)
    want = np.full(dst_off + n * d_page + 64, 7, np.uint8)
    for i, p in enumerate(pages):
        np.lib.stride_tricks.as_strided(src[src_off + i * s_page:], (h, w * c), (s_step, 1))[:] = p.reshape(h, w * c)
        np.lib.stride_tricks.as_strided(want[dst_off + i * d_page:], (h, w * och), (d_step, 1))[:] = oracle.bgnorm(p).reshape(h, w * och)
    tsrc = torch.from_numpy(src).to(cuda_device)
    tdst = torch.full((len(want),), 7, dtype=torch.uint8, device=cuda_device)
    assert tsrc.data_ptr() % 4 == 0 and tdst.data_ptr() % 4 == 0
    _capi.check(_capi.lib().prl_hip_bgnorm_batch_device(n, c, tsrc.data_ptr() + src_off, s_page, s_step, w, h, tdst.data_ptr() + dst_off,
                                                        d_page, d_step, torch.cuda.current_stream().cuda_stream))
    got = tdst.cpu().numpy()
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(tsrc.cpu().numpy(), src)


def test_fail_flag_is_per_page(prl, oracle, cuda_device):
    """Four 4-channel pages in one call - good, all green dark, good, all green dark: the failing pages come back as their first
    three channels, the good ones normalised, neither leaking to its neighbour.  (The pages of a call share one size, so pages too
    small for a map make a call of their own: all copied.)"""
    import torch

    pages, fails = bc.mixed_batch()
    got = prl.backgroundNormalization(torch.from_numpy(np.stack(pages)).to(cuda_device)).cpu().numpy()
    for i, (p, f) in enumerate(zip(pages, fails)):
        assert np.array_equal(got[i], oracle.bgnorm(p)), (i, int((got[i] != oracle.bgnorm(p)).sum()))
        assert np.array_equal(got[i], p[:, :, :3]) == f, i
    small = bc.small_batch()
    got = prl.backgroundNormalization(torch.from_numpy(np.stack(small)).to(cuda_device)).cpu().numpy()
    for i, p in enumerate(small):
        assert np.array_equal(got[i], p[:, :, :3]) and np.array_equal(got[i], oracle.bgnorm(p)), i
