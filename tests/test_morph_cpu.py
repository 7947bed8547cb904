"""tests/morph_ref.py against the two CPU restatements of the mask morphology, the information its pattern pages carry, and the case
list of tests/test_morph_gpu.py (plain data: its sizes, its buffers and the kernel each case is meant for are checked here)."""
import os
import re

import numpy as np
import pytest

import morph_ref as mr
import test_morph_gpu as tg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADII = [s * m for m in range(1, 9) for s in (1, -1)]


def _frac(a):
    return float(a.mean())


@pytest.mark.parametrize("n", RADII)
def test_reference_equals_both_restatements(oracle, n):
    """close_open (the OR / AND over all (2|n|+1)^2 offsets, taps outside the page ignored) equals oracle.morph (C) and
    oracle.numpy_model.morph (scipy's max / min filters) on every pattern page, on the flat pages and on pages thinner than the
    window"""
    from oracle import numpy_model

    pages = mr.pages_for(n, 70, 150, [16, 64, 100], [8, 32, 64], seed=3, max_phases=2) + mr.flat_pages(9, 33)
    pages += mr.pages_for(n, 3, 40, [16], [2], seed=4, max_phases=1) + mr.pages_for(n, 40, 2, [1], [8], seed=5, max_phases=1)
    pages += [("one", np.ones((1, 1), bool)), ("zero", np.zeros((1, 1), bool))]
    for name, p in pages:
        want = mr.to_bytes(mr.close_open(p, n))
        src = mr.to_bytes(p)
        assert np.array_equal(want, oracle.morph(src, n)), (name, p.shape)
        assert np.array_equal(want, numpy_model.morph(src, n)), (name, p.shape)


@pytest.mark.parametrize("m", range(1, 9))
def test_random_pages_are_not_vacuous(m):
    """A random page of density 2.5 / (2m+1)^2 (its complement for the opening): the reference output is 20..80 % set, differs
    from the input on >= 20 % of the pixels and from the reference at radius m - 1 (the input for m = 1) and m + 1 on >= 5 %.
    (A 50 % mask, which is what a thresholded noise page is, closes to 98.6 % set for n = 1 and to all set for every n >= 2.)"""
    page = mr.random_mask(300, 600, m, seed=20 + m)
    for n, p in ((m, page), (-m, ~page)):
        s = 1 if n > 0 else -1
        out = mr.close_open(p, n)
        assert 0.2 <= _frac(out) <= 0.8, (n, _frac(out))
        assert _frac(out != p) >= 0.2, (n, _frac(out != p))
        below = p if m == 1 else mr.close_open(p, s * (m - 1))
        above = mr.close_open(p, s * (m + 1))
        assert _frac(out != below) >= 0.05 and _frac(out != above) >= 0.05, (n, _frac(out != below), _frac(out != above))
    half = np.random.default_rng(1).random((300, 600)) < 0.5
    assert _frac(mr.close_open(half, 1)) > 0.97 and mr.close_open(half, 2).all() and not mr.close_open(~half, -2).any()


@pytest.mark.parametrize("m", range(1, 9))
def test_a_gap_of_2m_fuses_and_one_of_2m_plus_1_does_not(m):
    """what the gap pairs and the bars are built on, on one pair and one hole of each length, at every split"""
    for j in range(2 * m + 1):
        for g in (2 * m, 2 * m + 1):
            a = np.zeros((4 * m + 3, 8 * m + 8), bool)
            y, left = 2 * m + 1, 4 * m + 3 - j
            a[y, left] = a[y, left + g + 1] = True
            out = mr.close_open(a, m)
            want = a.copy()
            if g == 2 * m:
                want[y, left:left + g + 2] = True
            assert np.array_equal(out, want), (m, j, g)
            assert np.array_equal(mr.close_open(~a, -m), ~want)
            hole = np.ones((6 * m + 3, 8 * m + 8), bool)
            hole[2 * m + 1:4 * m + 2, left:left + g] = False
            assert np.array_equal(mr.close_open(hole, m), hole if g == 2 * m + 1 else np.ones_like(hole)), (m, j, g)
            assert np.array_equal(mr.close_open(~hole, -m), ~hole if g == 2 * m + 1 else np.zeros_like(hole)), (m, j, g)


@pytest.mark.parametrize("n", RADII)
def test_gap_and_bar_pages_tell_the_radius(n):
    """on every gap-pair and bar page the reference output differs from the input and from the reference at |n| - 1 and |n| + 1;
    together the pages of a pattern show every split at both lengths"""
    m, s = abs(n), (1 if n > 0 else -1)
    pages = mr.pages_for(n, 90, 300, [16, 100, 240], [8, 32, 64], seed=6, max_phases=40)
    names = [name for name, _ in pages]
    assert sum(x.startswith("gap_h") for x in names) == mr.n_phases(90, m, m + 1)
    assert sum(x.startswith("bar_h") for x in names) == mr.n_phases(90, m, 2 * m + 2)
    for name, p in pages:
        if not name.startswith(("gap", "bar")):
            continue
        out = mr.close_open(p, n)
        assert (out != p).any(), name
        assert (out != mr.close_open(p, s * (m + 1))).any(), name
        if m > 1:
            assert (out != mr.close_open(p, s * (m - 1))).any(), name
    # every (split, length) of the horizontal pairs around column 100 occurs on some page
    seen = set()
    for p in range(mr.n_phases(90, m, m + 1)):
        a = mr.gap_pairs_h(90, 300, m, [100], p)
        for y in range(0, 90, m + 1):
            x = np.flatnonzero(a[y])
            assert len(x) == 2
            seen.add((99 - int(x[0]), int(x[1] - x[0]) - 1))
    assert seen == {(j, g) for j in range(2 * m + 1) for g in (2 * m, 2 * m + 1)}


def test_bit_plane_layout_round_trip():
    """np.packbits(bitorder="little") is the bit plane the tests feed: pixel x of a row is bit x & 7 of byte x >> 3"""
    rng = np.random.default_rng(7)
    for w in (1, 7, 8, 9, 16, 17, 2049):
        a = rng.random((3, w)) < 0.5
        bits = mr.pack_rows(a)
        assert bits.shape == (3, (w + 7) // 8)
        assert np.array_equal(mr.unpack_rows(bits, w), a)
        for x in range(w):
            assert bool((bits[1, x >> 3] >> (x & 7)) & 1) == bool(a[1, x])


def test_geometry_constants_are_the_kernels():
    """the constants the GPU cases are aimed with, against prlib_amd/csrc/morph.hip"""
    src = open(os.path.join(ROOT, "prlib_amd", "csrc", "morph.hip")).read()
    for pattern in (rf"constexpr int kBitsMaxN = {tg.BITS_MAX_N};", rf"constexpr int kBitsAdvance = {tg.BITS_ADVANCE};",
                    rf"base_px = strip \* kBitsAdvance - {tg.BITS_LEAD};", rf"gx1 = gx0 \+ {64 * tg.BITS_CHUNK};",
                    rf"constexpr int RB = {tg.BITS_RB};", rf"int rps = {tg.BITS_RPS[0]};", rf"while \(rps > {tg.BITS_RPS[1]} &&",
                    rf"int rps = {tg.STREAM_RPS[0]};", rf"while \(rps > {tg.STREAM_RPS[1]} &&", rf"constexpr int kMaxN = {tg.MAX_N};",
                    rf"constexpr int BND = {tg.BND};", rf"constexpr int BTH = {tg.BTH};",
                    r"const int hd = 2 \* \(\(n \+ 3\) / 4\), useful = \(64 - 2 \* hd\) \* 4;",
                    r"const int h4 = \(\(2 \* n \+ 3\) / 4\) \* 4 \+ 8;", r"const int btw = BND \* 4 - 2 \* h4;"):
        assert re.search(pattern, src), pattern
    assert [tg.stream_useful(m) for m in (1, 4, 5, 8)] == [240, 240, 224, 224]
    assert [tg.binary_btw(m) for m in range(1, 9)] == [232, 232, 224, 224, 216, 216, 208, 208]


def test_case_list_is_well_formed():
    """every case of the GPU matrix: sizes within the limits, buffers that hold what each kernel reads and writes, the alignment
    class its name says, and together the 64 (kernel, radius, direction, source) combinations"""
    cs = tg.cases()
    assert len({c["name"] for c in cs}) == len(cs)
    combos = set()
    for c in cs:
        w, h, n = c["w"], c["h"], c["n"]
        assert 1 <= h <= 140 and 1 <= w <= 4100 and 1 <= abs(n) <= 8, c["name"]
        assert c["dst_step"] >= w and c["dst_off"] >= c["dst_step"], c["name"]                       # a guard row above page 0
        assert c["dst_page_stride"] >= (h + 1) * c["dst_step"] + w, c["name"]                       # pages (and a guard row) apart
        if c["form"] == 0:
            assert c["src_step"] >= w and c["src_page_stride"] >= (h - 1) * c["src_step"] + w, c["name"]
        else:
            assert c["src_step"] % 2 == 0 and c["src_off"] % 2 == 0 and c["src_page_stride"] % 2 == 0, c["name"]
            assert c["src_step"] >= tg.ceil_to(w, 16) // 8, c["name"]
        if c["dst"] == "a":
            assert c["dst_step"] % 16 == 0 and c["dst_off"] % 16 == c["a"], c["name"]
        combos.add((c["expect"], abs(n), n > 0, c["tag"]))
        family = c["name"].split("/")[0]
        assert c["expect"] in {"bits": (1, 2), "stream": (3,), "binary": (4,)}[family], c["name"]
    assert {(k, m, d) for k, m, d, _ in combos if k <= 2} == {(k, m, d) for k in (1, 2) for m in range(1, 5) for d in (True, False)}
    assert {(m, d) for k, m, d, _ in combos if k == 3} == {(m, d) for m in range(1, 9) for d in (True, False)}
    assert {(m, d, t) for k, m, d, t in combos if k == 4} == {(m, d, t) for m in range(1, 9) for d in (True, False)
                                                             for t in ("base+1", "oddstep")}
    c = [c for c in cs if c["name"].startswith("bits/align/w2033/a15/") and abs(c["n"]) == 4]
    assert len(c) == 4 and all(2000 - 15 in x["xs"] and 2000 in x["xs"] for x in c)     # A = 15, N = 4: the tightest margin
    # the buffers of a case: the source holds its pages where the layout says, everything else is the fill
    c = next(x for x in cs if x["name"].startswith("bits/pad/w17/fill255/") and x["form"] == 1)
    pages = tg.case_pages(c)[:3]
    buf = tg.source_buffer(c, pages)
    row = buf[c["src_off"] + c["src_page_stride"] + 2 * c["src_step"]:][:c["src_step"]]
    assert np.array_equal(mr.unpack_rows(row[None, :4], 32)[0, :17], pages[1][1][2]) and mr.unpack_rows(row[None, :4], 32)[0, 17:].all()
    assert (row[4:] == 255).all()
    exp = tg.expected_buffer(c, pages)
    assert (exp == tg.GUARD).sum() == exp.size - 3 * c["h"] * c["w"]
