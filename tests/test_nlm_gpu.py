"""NL-means (nlm.hip) kernel by kernel on the GPU, every comparison byte for byte against the CPU oracle.

  - every instantiation launch_nlm can pick, named through prl_hip_internal_nlm_variant of the test-hooks build (numbering:
    tests/nlm_cases.py), at strengths that put the weight table on the edges of the rule - 639 entries for the 4-byte-element kernel's
    LDS table, 1024 for the 8-byte one's, 1025 for the table read from memory - on pages that are ragged, single tiles, narrower than
    the halo, and on contents that drive the SSD to both ends of the table;
  - the product library's own choice at those strengths (tests/test_nlm_cpu.py shows which kernel that is);
  - pitched and odd-addressed views of both C entries with guard bytes, in-place denoise, the argument errors;
  - k_lbgr2lab / k_lab2lbgr on all 2^24 triples through prl_hip_internal_lab_convert, and prl.denoise on colours far from gray.

One process, no environment knobs: the hooks library is loaded beside the product library (each has its own workspace).
"""
import ctypes as C

import numpy as np
import pytest

import nlm_cases as nc

pytestmark = pytest.mark.gpu

GUARD = 0xA5
PRL_OK, PRL_ERR_EMPTY, PRL_ERR_BAD_CHANNELS, PRL_ERR_BAD_ARG = 0, 1, 3, 5


@pytest.fixture(scope="module")
def hooks(prl, cuda_device):
    L = nc.hooks()
    assert L.prl_hip_set_device(0) == PRL_OK
    return L


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _strength(oracle, channels, key):
    return key if isinstance(key, float) else nc.edge_strength(oracle, channels, key)


_REF = {}


def _reference(oracle, channels, h, shape):
    """[(name, page, oracle's result)] of nc.pages(shape, channels), computed once per (channels, h, shape)."""
    key = (channels, h, shape)
    if key not in _REF:
        out = []
        for name, page in nc.pages(shape, channels):
            want = oracle.nlm_planes(page, h, threads=8)
            page.setflags(write=False)
            want.setflags(write=False)
            out.append((name, page, want))
        _REF[key] = out
    return _REF[key]


def _run_variant(hooks, cuda_device, variant, channels, h, batch):
    """batch: N x H x W x C -> (status, N x H x W x C result, number of guard bytes changed); the destination rows are 3 bytes
    longer than the page's and the pages 5 bytes apart."""
    import torch

    n, hh, w, c = batch.shape
    src = torch.from_numpy(np.ascontiguousarray(batch)).to(cuda_device)
    step = w * c + 3
    dst = torch.full((n * (hh * step + 5),), GUARD, dtype=torch.uint8, device=cuda_device)
    st = hooks.prl_hip_internal_nlm_variant(variant, n, channels, h, src.data_ptr(), hh * w * c, w * c, w, hh, dst.data_ptr(), hh * step + 5,
                                            step, _stream())
    torch.cuda.synchronize()
    o = dst.cpu().numpy().reshape(n, hh * step + 5)
    rows = o[:, :hh * step].reshape(n, hh, step)
    touched = int((rows[:, :, w * c:] != GUARD).sum() + (o[:, hh * step:] != GUARD).sum())
    return st, rows[:, :, :w * c].reshape(n, hh, w, c).copy(), touched


# (variant, channels, strength): a float, or the table length the strength is searched for
VARIANT_CASES = [(v, ch, s) for ch in (1, 2) for v, ss in ((nc.XL_LDS, (3.0, 639)), (nc.XL_MEM, (639, 1025)), (nc.Y_LDS, (640, 1024)),
                                                          (nc.Y_MEM, (3.0, 1025))) for s in ss]
VARIANT_CASES += [(nc.C3_LDS, 3, 3.0), (nc.C3_LDS, 3, 1024), (nc.C3_MEM, 3, 3.0), (nc.C3_MEM, 3, 1025)]


@pytest.mark.parametrize("variant,channels,strength", VARIANT_CASES)
def test_every_variant_on_every_page(hooks, oracle, cuda_device, variant, channels, strength):
    h = _strength(oracle, channels, strength)
    if not isinstance(strength, float):
        st, n_lut, _, _ = nc.plan(channels, h)
        assert (st, n_lut) == (PRL_OK, strength)          # the library's table has the length the case is about
    for shape in nc.SHAPES:
        ref = _reference(oracle, channels, h, shape)
        assert len(ref) >= 3
        st, got, touched = _run_variant(hooks, cuda_device, variant, channels, h, np.stack([p for _, p, _ in ref]))
        assert st == PRL_OK, (shape, st)
        for i, (name, page, want) in enumerate(ref):
            bad = int((got[i] != want).sum())
            assert bad == 0, f"variant {variant}, {channels} channels, h = {h}, {shape[0]} x {shape[1]} page {i} ({name}): {bad} samples differ"
            if name == "flat255":
                assert (got[i] == 255).all()
        assert touched == 0, (shape, touched)


@pytest.mark.parametrize("variant,channels", [(v, ch) for ch in (1, 2) for v in range(4)] + [(nc.C3_LDS, 3), (nc.C3_MEM, 3)])
def test_strength_zero_returns_the_input(hooks, oracle, cuda_device, variant, channels):
    """h = 0: weight 19096 for an SSD below 64 and nothing else (a table of one entry, which fits every variant)."""
    for shape in [(45, 70), (33, 65), (5, 3), (1, 1)]:
        ref = _reference(oracle, channels, 0.0, shape)
        batch = np.stack([p for _, p, _ in ref])
        for name, page, want in ref:
            assert np.array_equal(want, page), (shape, name)          # the oracle agrees that this is the identity on these pages
        st, got, touched = _run_variant(hooks, cuda_device, variant, channels, 0.0, batch)
        assert st == PRL_OK and touched == 0 and np.array_equal(got, batch), (shape, st, touched, int((got != batch).sum()))


def test_two_pages_against_the_definition(hooks, oracle, cuda_device):
    """Not through the oracle: the by-the-definition loops of tests/test_oracle.py on two 12 x 14 pages, at the strengths that fill
    the 8-byte-element kernel's LDS table (the kernel no product call reached in the suite before this file)."""
    from test_oracle import _nlm_naive

    rng = np.random.default_rng(5)
    for channels, sigma in ((1, 20.0), (2, 9.0)):
        h = nc.edge_strength(oracle, channels, nc.LUT_MAX)
        page = np.clip(rng.normal(128, sigma, (12, 14, channels)), 0, 255).astype(np.uint8)
        want = _nlm_naive(page, h, oracle.nlm_weights(channels, h))
        st, got, touched = _run_variant(hooks, cuda_device, nc.Y_LDS, channels, h, page[None])
        assert st == PRL_OK and touched == 0 and np.array_equal(got[0], want)


def test_variant_entry_refuses_what_does_not_fit(hooks, oracle, cuda_device):
    page = np.zeros((1, 4, 4, 1), np.uint8)
    for channels in (1, 2):
        b = np.repeat(page, channels, 3)
        h640, h1025 = nc.edge_strength(oracle, channels, 640), nc.edge_strength(oracle, channels, 1025)
        for variant, h in [(nc.XL_LDS, h640), (nc.Y_LDS, h1025), (nc.C3_LDS, 3.0), (nc.C3_MEM, 3.0), (-1, 3.0), (6, 3.0)]:
            st, _, touched = _run_variant(hooks, cuda_device, variant, channels, h, b)
            assert st == PRL_ERR_BAD_ARG and touched == 0, (channels, variant, h, st)
    b = np.repeat(page, 3, 3)
    for variant, h in [(nc.XL_LDS, 3.0), (nc.Y_MEM, 3.0), (nc.C3_LDS, nc.edge_strength(oracle, 3, 1025))]:
        st, got, _ = _run_variant(hooks, cuda_device, variant, 3, h, b)
        assert st == PRL_ERR_BAD_ARG and (got == GUARD).all(), (variant, h, st)


@pytest.mark.parametrize("channels", [1, 2, 3])
def test_product_dispatch_at_the_table_edges(prl, oracle, cuda_device, channels):
    """prl.nlm_planes (the product library, its own rule) on either side of both thresholds; with test_kernel_choice_at_the_table_edges
    this is k_nlm_y_xl<C, true> | k_nlm_y<C, true> | k_nlm_y<C, true> | k_nlm_y<C, false> for one and two channels."""
    import torch

    for length in nc.EDGES:
        h = nc.edge_strength(oracle, channels, length)
        for shape in [(45, 70), (13, 14)]:
            ref = _reference(oracle, channels, h, shape)
            got = prl.nlm_planes(torch.from_numpy(np.stack([p for _, p, _ in ref])).to(cuda_device), h).cpu().numpy()
            for i, (name, _, want) in enumerate(ref):
                assert np.array_equal(got[i], want), (length, h, shape, name)


# ---- views ---------------------------------------------------------------------------------------------------------------------

def _strided(buf, off, n, page_stride, step, rows, row_bytes):
    return np.lib.stride_tricks.as_strided(buf[off:], (n, rows, row_bytes), (page_stride, step, 1))


def _call_on_views(cuda_device, entry, head, pages, src_off):
    """pages (N x H x W x C) laid out in a larger source buffer from byte `src_off` on, rows 7 bytes and pages 11 bytes further apart
    than they need be (so steps are odd where the row is even); the destination likewise from byte 3 with 5 and 13.  Returns
    (status, result, guard bytes changed)."""
    import torch

    n, hh, w, c = pages.shape
    row = w * c
    s_step, d_step = row + 7, row + 5
    s_page, d_page = hh * s_step + 11, hh * d_step + 13
    sbuf = np.random.default_rng(src_off).integers(0, 256, src_off + n * s_page + 16, dtype=np.uint8)
    _strided(sbuf, src_off, n, s_page, s_step, hh, row)[:] = pages.reshape(n, hh, row)
    dbuf = np.full(3 + n * d_page + 16, GUARD, np.uint8)
    d_src, d_dst = torch.from_numpy(sbuf).to(cuda_device), torch.from_numpy(dbuf).to(cuda_device)
    st = entry(n, c, *head, d_src.data_ptr() + src_off, s_page, s_step, w, hh, d_dst.data_ptr() + 3, d_page, d_step, _stream())
    torch.cuda.synchronize()
    assert np.array_equal(d_src.cpu().numpy(), sbuf)
    o = d_dst.cpu().numpy()
    view = _strided(o, 3, n, d_page, d_step, hh, row)
    got = view.reshape(n, hh, w, c).copy()
    view[:] = GUARD
    return st, got, int((o != GUARD).sum())


@pytest.mark.parametrize("src_off", [1, 2, 3, 5])
def test_planes_entry_on_pitched_odd_views(prl, oracle, cuda_device, src_off):
    """prl_hip_nlm_planes_device with row steps and page strides larger than the data and a source that starts at an odd / even
    unaligned byte.  The two-channel staging reads a pixel's two bytes at any address: its source is written as two byte loads (the
    compiler joins them into one 16-bit load, which gfx950 serves unaligned)."""
    from prlib_amd import _capi

    L = _capi.lib()
    for channels in (1, 2, 3):
        for length in ((3.0, nc.LUT_MAX) if channels < 3 else (3.0,)):          # the 4-byte- and the 8-byte-element kernel
            h = _strength(oracle, channels, length)
            ref = _reference(oracle, channels, h, (33, 65))[:3]
            st, got, touched = _call_on_views(cuda_device, L.prl_hip_nlm_planes_device, (float(h),), np.stack([p for _, p, _ in ref]), src_off)
            assert st == PRL_OK and touched == 0, (channels, h, st, touched)
            for i, (name, _, want) in enumerate(ref):
                assert np.array_equal(got[i], want), (channels, h, name)


def _colour_pages(channels, shape=(40, 70)):
    """Three pages far from gray: uniformly random colours, saturated primaries in 8 x 8 blocks, both mixed; alpha random."""
    h, w = shape
    rng = np.random.default_rng(17)
    rand = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    prim = np.array([[0, 0, 255], [0, 255, 0], [255, 0, 0], [255, 255, 0], [255, 0, 255], [0, 255, 255], [0, 0, 0], [255, 255, 255]], np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    blocks = rand.copy()
    blocks[:, :, :3] = prim[((yy // 8) * 3 + xx // 8) % 8]
    mixed = np.where(((yy + xx) % 5 == 0)[:, :, None], rand, blocks)
    return np.stack([rand, blocks, mixed])[:, :, :, :channels].copy()


_DENOISE_REF = {}


def _denoise_reference(oracle, channels, strength):
    key = (channels, strength)
    if key not in _DENOISE_REF:
        pages = _colour_pages(channels)
        _DENOISE_REF[key] = (pages, np.stack([oracle.denoise(p, strength, threads=8) for p in pages]))
    return _DENOISE_REF[key]


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("strength", [5.5, 12.0])
def test_denoise_on_colours_far_from_gray(prl, oracle, cuda_device, channels, strength):
    """The whole stage where a and b leave 128 by far and the inverse conversion clips; strength 12 filters L with k_nlm_y<1, true>.
    Also in place (out is the input)."""
    import torch

    pages, want = _denoise_reference(oracle, channels, strength)
    t = torch.from_numpy(pages).to(cuda_device)
    got = prl.denoise(t, strength)
    assert np.array_equal(got.cpu().numpy(), want), np.abs(got.cpu().numpy().astype(int) - want).max()
    assert np.array_equal(t.cpu().numpy(), pages)
    assert prl.denoise(t, strength, out=t) is t
    assert np.array_equal(t.cpu().numpy(), want)


@pytest.mark.parametrize("src_off", [1, 2, 3, 5])
def test_denoise_entry_on_pitched_odd_views(prl, oracle, cuda_device, src_off):
    from prlib_amd import _capi

    L = _capi.lib()
    for channels in (3, 4):
        pages, want = _denoise_reference(oracle, channels, 12.0)
        st, got, touched = _call_on_views(cuda_device, L.prl_hip_denoise_batch_device, (12.0,), pages, src_off)
        assert st == PRL_OK and touched == 0, (channels, st, touched)
        assert np.array_equal(got, want), channels


def test_argument_errors(prl, oracle, cuda_device):
    import torch

    from prlib_amd import _capi

    L = _capi.lib()
    src = torch.zeros(4096, dtype=torch.uint8, device=cuda_device)
    dst = torch.full((4096,), GUARD, dtype=torch.uint8, device=cuda_device)
    s, d = src.data_ptr(), dst.data_ptr()

    def planes(channels, src_step=40, dst_step=40, src_ptr=s, dst_ptr=d, width=10, height=10):
        return L.prl_hip_nlm_planes_device(1, channels, 3.0, src_ptr, 400, src_step, width, height, dst_ptr, 400, dst_step, None)

    def denoise(channels, src_step=40, dst_step=40, width=10, height=10):
        return L.prl_hip_denoise_batch_device(1, channels, 5.5, s, 400, src_step, width, height, d, 400, dst_step, None)

    assert planes(1, src_ptr=s, dst_ptr=s) == PRL_ERR_BAD_ARG                       # the tile's halo is read while other tiles write
    assert planes(0) == PRL_ERR_BAD_CHANNELS and planes(4) == PRL_ERR_BAD_CHANNELS
    assert denoise(1) == PRL_ERR_BAD_CHANNELS and denoise(2) == PRL_ERR_BAD_CHANNELS
    for ch in (1, 2, 3):
        assert planes(ch, src_step=10 * ch - 1) == PRL_ERR_BAD_ARG and planes(ch, dst_step=10 * ch - 1) == PRL_ERR_BAD_ARG
    for ch in (3, 4):
        assert denoise(ch, src_step=10 * ch - 1) == PRL_ERR_BAD_ARG and denoise(ch, dst_step=10 * ch - 1) == PRL_ERR_BAD_ARG
    assert planes(1, width=0) == PRL_ERR_EMPTY and denoise(3, height=0) == PRL_ERR_EMPTY
    assert denoise(3, src_step=4, dst_step=4, width=1, height=65536) == PRL_ERR_BAD_ARG   # one grid row per image row in the conversions
    # the weight table that does not fit its workspace slot (found as in tests/test_nlm_cpu.py) is refused; the one before it runs
    h_bad = nc.first_strength_with(oracle, 3, nc.SLOT_ENTRIES)
    tiny = nc.pages((5, 3), 3)[0][1]
    t = torch.from_numpy(tiny).to(cuda_device)
    with pytest.raises(_capi.PrlError) as e:
        prl.nlm_planes(t, h_bad)
    assert e.value.status == PRL_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert (dst == GUARD).all() and (src == 0).all()
    h_ok = h_bad - nc.H_STEP
    assert np.array_equal(prl.nlm_planes(t, h_ok).cpu().numpy(), oracle.nlm_planes(tiny, h_ok))


# ---- the Lab conversions on their whole domain ----------------------------------------------------------------------------------------

_LAB = {}


def _lab_reference(oracle):
    """All 2^24 triples as one 4096 x 4096 page, read as BGR (forward) and as Lab (inverse), with the oracle's results."""
    if not _LAB:
        c = nc.all_colours()
        _LAB.update(colours=c, lab=oracle.lbgr2lab(c), bgr=oracle.lab2lbgr(c, 3))
        for a in _LAB.values():
            a.setflags(write=False)
    return _LAB["colours"], _LAB["lab"], _LAB["bgr"]


def _convert(hooks, cuda_device, inverse, channels, width, t_bgr, step, t_l, t_ab):
    import torch

    st = hooks.prl_hip_internal_lab_convert(inverse, 1, channels, t_bgr.data_ptr(), t_bgr.numel(), step, width, 4096, t_l.data_ptr(),
                                            t_ab.data_ptr(), _stream())
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize("channels,width", [(3, 4096), (4, 4096), (3, 4095), (4, 4095)])
def test_lab_conversions_on_all_colours(hooks, oracle, cuda_device, channels, width):
    """k_lbgr2lab and k_lab2lbgr against the oracle on every triple.  The inverse is float32 with one rounding per operation: it
    equals the host's only while the device code is built without contraction and divides and rounds as the host does.  Width 4095:
    the same triples but for the last column, in pitched pages (the rows keep their 4096-pixel step) with guard bytes."""
    import torch

    colours, lab, bgr = _lab_reference(oracle)
    rng = np.random.default_rng(channels)
    page = np.empty((4096, 4096, channels), np.uint8)
    page[:, :, :3] = colours
    if channels == 4:
        page[:, :, 3] = rng.integers(0, 256, (4096, 4096), dtype=np.uint8)
    step = 4096 * channels
    # forward: BGR(A) page -> planes
    t_page = torch.from_numpy(page).to(cuda_device)
    t_l = torch.full((4096 * width + 64,), GUARD, dtype=torch.uint8, device=cuda_device)
    t_ab = torch.full((2 * 4096 * width + 64,), GUARD, dtype=torch.uint8, device=cuda_device)
    assert _convert(hooks, cuda_device, 0, channels, width, t_page, step, t_l, t_ab) == PRL_OK
    assert torch.equal(t_page, torch.from_numpy(page).to(cuda_device))
    got_l, got_ab = t_l.cpu().numpy(), t_ab.cpu().numpy()
    assert (got_l[4096 * width:] == GUARD).all() and (got_ab[2 * 4096 * width:] == GUARD).all()
    want = lab[:, :width]
    bad = got_l[:4096 * width].reshape(4096, width) != want[:, :, 0]
    assert not bad.any(), f"L differs for {int(bad.sum())} colours, first (B, G, R) = {colours[:, :width][bad][0]}"
    bad = (got_ab[:2 * 4096 * width].reshape(4096, width, 2) != want[:, :, 1:]).any(axis=2)
    assert not bad.any(), f"a / b differ for {int(bad.sum())} colours, first (B, G, R) = {colours[:, :width][bad][0]}"
    # inverse: the same triples read as (L, a, b) -> BGR(A) page
    t_l = torch.from_numpy(np.ascontiguousarray(colours[:, :width, 0])).to(cuda_device)
    t_ab = torch.from_numpy(np.ascontiguousarray(colours[:, :width, 1:])).to(cuda_device)
    t_out = torch.full((4096, 4096, channels), GUARD, dtype=torch.uint8, device=cuda_device)
    assert _convert(hooks, cuda_device, 1, channels, width, t_out, step, t_l, t_ab) == PRL_OK
    got = t_out.cpu().numpy()
    assert (got[:, width:] == GUARD).all()
    bad = (got[:, :width, :3] != bgr[:, :width]).any(axis=2)
    assert not bad.any(), (f"{int(bad.sum())} of the (L, a, b) triples differ, first {colours[:, :width][bad][0]}: "
                           f"{got[:, :width, :3][bad][0]} instead of {bgr[:, :width][bad][0]}")
    if channels == 4:
        assert (got[:, :width, 3] == 255).all()


def test_lab_entry_argument_errors(hooks, cuda_device):
    import torch

    t = torch.zeros(4096, dtype=torch.uint8, device=cuda_device)
    p = t.data_ptr()
    f = hooks.prl_hip_internal_lab_convert
    assert f(0, 1, 2, p, 400, 40, 10, 10, p, p, None) == PRL_ERR_BAD_CHANNELS
    assert f(0, 1, 3, p, 400, 29, 10, 10, p, p, None) == PRL_ERR_BAD_ARG
    assert f(1, 1, 3, p, 400, 40, 10, 0, p, p, None) == PRL_ERR_EMPTY
    assert f(1, 1, 3, p, 400, 40, 10, 10, None, p, None) == PRL_ERR_BAD_ARG
