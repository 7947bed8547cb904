"""oracle.rotate - the only thing the device's prl::rotate is compared with - pinned by an independently written model
(tests/rotate_ref.py: the 10-bit coordinates, the 5-bit weights, the (sum + 2^14) >> 15 rounding, the quarter-turn branches) on
every page and angle tests/test_rotate_gpu.py uses: 0 differing bytes, the matrix to the last bit."""
import numpy as np
import pytest

import rotate_cases as rc
import rotate_ref as rr

CASES = rc.all_cpu_cases()
LOOP_FULL_PIXELS = 100 * 100      # canvases up to this size go through the per-pixel loop whole, larger ones on a sample of rows


def _loop_rows(oh):
    """the first and last rows, the rows round every multiple of 256 and a stride of 97 in between (coprime to 4 and to 32)"""
    rows = set(range(min(oh, 3))) | set(range(max(0, oh - 3), oh)) | set(range(0, oh, 97))
    for m in range(256, oh, 256):
        rows |= {m - 1, m, m + 1} & set(range(oh))
    return sorted(rows)


def test_case_lists_cover_what_they_name():
    warp = rc.warp_cases()
    for side in rc.SIDES:
        mine = [x for x in warp if max(x[1], x[2]) == side and (x[1], x[2]) not in rc.THIN]
        assert sorted(x[3] for x in mine) == [1, 2, 3, 4], side
        if side > 1:
            assert any(x[1] < x[2] for x in mine) and any(x[1] > x[2] for x in mine), side
    assert {s % 4 for s in rc.SIDES} == {0, 1, 2, 3}
    assert {(s + 255) // 256 for s in rc.SIDES} == {1, 2, 3, 4}
    for a in rc.ANGLES:
        assert rr.kind(a) == 0, a
        assert {x[3] for x in warp if a in x[4]} >= {1, 2, 3, 4}, a
        assert any(a in x[4] and max(x[1], x[2]) >= 255 for x in warp), a
    assert {(x[1], x[2]) for x in warp} >= set(rc.THIN) | {(1, 1)}
    rot = rc.rot90_cases()
    assert {(x[1], x[2], x[3]) for x in rot if not x[0].startswith("half")} == {(h, w, c) for h, w in rc.ROT90_SHAPES for c in (1, 2, 3, 4)}
    assert [rr.kind(a) for a in rc.ROT90_ANGLES] == [1, 3, 1, 1]
    assert [rr.kind(a) for a in rc.VIEW_ANGLES] == [0, 1, 2, 3, 0]
    assert [rr.out_size(rc.VIEW_W, rc.VIEW_H, a) for a in rc.VIEW_ANGLES] == [(300, 300), (77, 300), (300, 77), (77, 300), (300, 300)]
    assert len({cid for cid, _, _ in CASES}) == len(CASES)


_both = {}


def _oracle_and_numpy(oracle, cid, p, a):
    """(oracle.rotate, rotate_numpy) of a case, computed once for the tests of this file"""
    if cid not in _both:
        _both[cid] = (oracle.rotate(p, a), rr.rotate_numpy(p, a))
    return _both[cid]


def test_numpy_form_equals_the_oracle_on_every_gpu_case(oracle):
    for cid, p, a in CASES:
        want, got = _oracle_and_numpy(oracle, cid, p, a)
        assert got.shape == want.shape and np.array_equal(got, want), (cid, int((got != want).sum()))


def test_loop_form_equals_the_numpy_form_and_the_oracle(oracle):
    for cid, p, a in CASES:
        ow, oh = rr.out_size(p.shape[1], p.shape[0], a)
        rows = None if ow * oh <= LOOP_FULL_PIXELS else _loop_rows(oh)
        got = rr.rotate_loop(p, a, rows)
        sel = slice(None) if rows is None else rows
        want, plane = _oracle_and_numpy(oracle, cid, p, a)
        assert np.array_equal(got, plane[sel]), cid
        assert np.array_equal(got, want[sel]), cid


def test_matrix_to_the_last_bit(oracle):
    sizes = sorted({(p.shape[1], p.shape[0]) for _, p, _ in CASES})
    n = 0
    for w, h in sizes:
        for a in rc.ANGLES + rc.KIND_ANGLES + [12.5, 2.0, -33.0]:
            if rr.kind(a):
                continue
            got = np.array(rr.matrix(w, h, a), np.float64)
            want = oracle.rotate_matrix(w, h, a)
            assert got.view(np.uint64).tolist() == want.view(np.uint64).tolist(), (w, h, a, got, want)
            n += 1
    assert n > 500


@pytest.mark.parametrize("w,h", [(300, 77), (77, 300), (1, 1), (64, 64)])
def test_kind_and_result_size_at_the_edges_of_the_quarter_turns(oracle, w, h):
    from oracle import capi

    for a in rc.KIND_ANGLES:
        assert capi.lib().prl_oracle_rotate_kind(a) == rr.kind(a), a
        assert oracle.rotate_size(w, h, a) == rr.out_size(w, h, a), a
    # the model's own answers, from the definition: within 1e-7 of the quarter turn after fmod, which keeps the sign
    assert [rr.kind(a) for a in rc.KIND_ANGLES] == [1, 1, 0, 0, 2, 2, 0, 0, 3, 3, 0, 0, 1, 0, 0, 0]
    p = rc.page(h, w, 3, 7)
    for a in rc.KIND_ANGLES:
        want = oracle.rotate(p, a)
        assert np.array_equal(rr.rotate_numpy(p, a), want), a


def test_model_sees_the_coordinate_rounding(monkeypatch):
    """The pages can tell the + 16 of the coordinates apart: without it the model gives other bytes on a small random page."""
    p = rc.page(40, 57, 3, 11)
    base = rr.rotate_numpy(p, 3.0)
    monkeypatch.setattr(rr, "ROUND_DELTA", 0)
    assert (rr.rotate_numpy(p, 3.0) != base).any()
