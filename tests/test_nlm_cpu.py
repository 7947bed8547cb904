"""Host side of NL-means (nlm.hip) without a GPU: the weight table and the kernel choice of the library through
prl_hip_internal_nlm_plan of the test-hooks build, and the CPU oracle's Lab conversions against the colour space they claim.

Lab: prl_oracle_lbgr2lab is "restated from memory" of OpenCV's 8-bit fixed-point RGB2Lab_b and pinned by no OpenCV build, and the
device conversion is compared with it byte for byte (tests/test_nlm_gpu.py).  test_oracle_lab_against_the_definition measures
how far the oracle sits from CIE L*a*b* itself, evaluated in float64 for all 2^24 colours (values in 8-bit levels: L * 255 / 100,
a + 128, b + 128).  Measured when this test was written, with the (B, G, R) that attains each (one colour each):
    L  1.0287117299351607 at (11, 2, 1)      oracle (23, 138, 103), definition (21.971, 138.982, 102.864)
    a  2.021555773415301  at (1, 4, 0)       oracle (26, 112, 138), definition (25.970, 109.978, 137.554)
    b  0.9890393315086783 at (0, 4, 14)      oracle (43, 141, 154), definition (43.192, 140.913, 153.011)
- all three at very dark colours, where f(t) is steepest and the cube-root table is entered with an index rounded to 1 / 2040.
Half of all colours are within 0.25 levels in every channel (rounding alone gives 0.25 on average), 99.99 % within 0.71 / 0.85 / 0.64.
The round trip lab2lbgr(lbgr2lab(c)) moves B, G, R by at most 4, 3, 5 levels; 106 colours reach 5, all in R, for example
(246, 193, 191) -> Lab (231, 133, 116) -> (246, 194, 196).  The same CPU code runs on both sides of each comparison, so the
assertions carry no margin beyond 1e-9 for another numpy's cbrt.
"""
import numpy as np
import pytest

import nlm_cases as nc

PRL_OK, PRL_ERR_BAD_CHANNELS, PRL_ERR_BAD_ARG = 0, 3, 5


def _strengths(oracle, channels):
    edges = [nc.edge_strength(oracle, channels, n) for n in nc.EDGES]
    return [0.0, 0.25, 1.0, 3.0, 5.5, 10.0, 14.0, 40.0] + edges + sorted(nc.RECORDED[channels].values())


@pytest.mark.parametrize("channels", [1, 2, 3])
def test_weight_table_equals_the_oracle(prl, oracle, channels):
    for h in _strengths(oracle, channels):
        want = oracle.nlm_weights(channels, h)
        st, n, variant, lut = nc.plan(channels, h)
        assert st == PRL_OK, (channels, h)
        assert n == nc.oracle_n_lut(oracle, channels, h) and len(lut) == n, (channels, h, n)
        assert np.array_equal(lut, want[:n]) and not want[n:].any(), (channels, h)
        assert variant == nc.expected_variant(channels, n), (channels, h, n, variant)
    assert nc.plan(channels, 0.0)[1] == 1 and nc.plan(channels, 0.0)[3][0] == 19096          # exp(-0 / 0) = NaN -> weight 1; the rest exp(-inf)
    # a short buffer receives the head of the table, the length is reported in full
    st, n, _, lut = nc.plan(channels, 10.0, cap=7)
    assert st == PRL_OK and n > 7 and np.array_equal(lut, oracle.nlm_weights(channels, 10.0)[:7])


def test_recorded_strengths_still_sit_on_their_edges(oracle):
    for channels, rec in nc.RECORDED.items():
        for length, h in rec.items():
            assert float(np.float32(h)) == h
            assert nc.oracle_n_lut(oracle, channels, h) == length, (channels, length, h)


@pytest.mark.parametrize("channels", [1, 2, 3])
def test_kernel_choice_at_the_table_edges(prl, oracle, channels):
    want = {1: [nc.XL_LDS, nc.Y_LDS, nc.Y_LDS, nc.Y_MEM], 2: [nc.XL_LDS, nc.Y_LDS, nc.Y_LDS, nc.Y_MEM],
            3: [nc.C3_LDS, nc.C3_LDS, nc.C3_LDS, nc.C3_MEM]}[channels]
    for length, v in zip(nc.EDGES, want):
        h = nc.edge_strength(oracle, channels, length)
        st, n, variant, _ = nc.plan(channels, h)                    # the product's knobs
        assert (st, n, variant) == (PRL_OK, length, v), (channels, length, h)
        # the knobs: bit channels - 1 of knob_xl admits the 4-byte-element kernel, the same bit of knob_glut moves ITS table to
        # memory; no other bit and no other variant depends on them
        for knob_xl in range(4):
            for knob_glut in range(4):
                got = nc.plan(channels, h, knob_xl, knob_glut)
                assert got[:2] == (PRL_OK, length) and got[2] == nc.expected_variant(channels, length, knob_xl, knob_glut), (channels, length, knob_xl, knob_glut)
    if channels < 3:
        bit, other = 1 << (channels - 1), 1 << (2 - channels)
        h = nc.edge_strength(oracle, channels, nc.LUT_MAX_XL)
        assert nc.plan(channels, h, bit, 0)[2] == nc.XL_LDS and nc.plan(channels, h, other, 0)[2] == nc.Y_LDS
        assert nc.plan(channels, h, 3, bit)[2] == nc.XL_MEM and nc.plan(channels, h, 3, other)[2] == nc.XL_LDS
        assert nc.plan(channels, h, other, bit)[2] == nc.Y_LDS      # without the 4-byte kernel the table knob selects nothing


def test_plan_rejects_other_channel_counts(prl):
    assert nc.plan(0, 3.0)[0] == PRL_ERR_BAD_CHANNELS and nc.plan(4, 3.0)[0] == PRL_ERR_BAD_CHANNELS


def test_oversized_table_is_refused_not_truncated(prl, oracle):
    """The first h whose trimmed 3-channel table (with its closing zero) exceeds the 512 KiB workspace slot: found by bisection with
    the oracle.  One and two channels cannot get there (their full tables have 49 785 and 99 570 entries)."""
    assert len(oracle.nlm_weights(1, 1e4)) < nc.SLOT_ENTRIES and len(oracle.nlm_weights(2, 1e4)) < nc.SLOT_ENTRIES
    h_bad = nc.first_strength_with(oracle, 3, nc.SLOT_ENTRIES)
    h_ok = h_bad - nc.H_STEP
    assert nc.oracle_n_lut(oracle, 3, h_ok) + 1 <= nc.SLOT_ENTRIES < nc.oracle_n_lut(oracle, 3, h_bad) + 1
    st, n, variant, lut = nc.plan(3, h_ok)
    assert (st, n, variant) == (PRL_OK, nc.oracle_n_lut(oracle, 3, h_ok), nc.C3_MEM)
    assert np.array_equal(lut, oracle.nlm_weights(3, h_ok)[:n])
    st, n, _, _ = nc.plan(3, h_bad)
    assert st == PRL_ERR_BAD_ARG and n == nc.oracle_n_lut(oracle, 3, h_bad)
    assert nc.plan(3, 1e4)[0] == PRL_ERR_BAD_ARG


# ---- the oracle's Lab conversions ----------------------------------------------------------------------------------------------

# max |oracle - float64 definition| over all 2^24 colours, in 8-bit levels, when the test was written (module docstring)
LAB_DISTANCE = (1.0287117299351607, 2.021555773415301, 0.9890393315086783)
ROUND_TRIP = (4, 3, 5)      # B, G, R


def _lab_definition(bgr):
    """CIE L*a*b* of linear BGR bytes in float64, scaled as 8-bit Lab stores it; no rounding, no clamp."""
    m = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
    white = np.array([0.950456, 1.0, 1.088754])
    rgb = bgr[:, ::-1].astype(np.float64) / 255.0
    xyz = rgb @ m.T / white
    f = np.where(xyz > 0.008856, np.cbrt(xyz), 7.787 * xyz + 16.0 / 116.0)
    L = 116.0 * f[:, 1] - 16.0
    return np.stack([L * 255.0 / 100.0, 500.0 * (f[:, 0] - f[:, 1]) + 128.0, 200.0 * (f[:, 1] - f[:, 2]) + 128.0], axis=1)


def test_oracle_lab_against_the_definition(oracle):
    """Figures and colours: module docstring.  The bound is what was measured."""
    colours = nc.all_colours()
    lab = oracle.lbgr2lab(colours).reshape(-1, 3)
    flat = colours.reshape(-1, 3)
    worst, where = np.zeros(3), [None] * 3
    for lo in range(0, 1 << 24, 1 << 20):
        d = np.abs(lab[lo:lo + (1 << 20)] - _lab_definition(flat[lo:lo + (1 << 20)]))
        for c in range(3):
            i = int(d[:, c].argmax())
            if d[i, c] > worst[c]:
                worst[c], where[c] = d[i, c], tuple(int(v) for v in flat[lo + i])
    print("max |oracle - definition| (L, a, b):", worst, "at (B, G, R)", where)
    for c in range(3):
        assert worst[c] <= LAB_DISTANCE[c] + 1e-9, (c, worst[c], where[c])


def test_oracle_lab_round_trip_on_all_colours(oracle):
    """lab2lbgr(lbgr2lab(c)) over all 2^24 colours: 8-bit Lab cannot hold every colour; the result is within 4, 3, 5 levels in B, G, R
    (test_oracle.py asserts 4 on a sample of 1024 colours, which holds none of the 106 colours that reach 5).  4-channel output:
    alpha 255."""
    colours = nc.all_colours()
    lab = oracle.lbgr2lab(colours)
    back = oracle.lab2lbgr(lab)
    d = np.abs(back.astype(np.int16) - colours).reshape(-1, 3)
    worst = d.max(axis=0)
    i = int(d.max(axis=1).argmax())
    print("round trip: max per channel (B, G, R)", worst, "e.g.", colours.reshape(-1, 3)[i], "->", back.reshape(-1, 3)[i], "; colours off by 5:",
          int((d.max(axis=1) == 5).sum()))
    assert all(int(v) <= m for v, m in zip(worst, ROUND_TRIP)), worst
    four = oracle.lab2lbgr(lab[:64], 4)
    assert np.array_equal(four[:, :, :3], back[:64]) and (four[:, :, 3] == 255).all()
