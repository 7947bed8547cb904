"""The thinning stage (thin.hip) kernel by kernel on the GPU, bit-exact against the numpy reference of tests/thin_ref.py:
k_thin_pack / k_thin_unpack alone, single passes of k_thin_pass over every 3 x 3 neighbourhood at every bit and row position and
across the strip seam, the page borders, the activity tracking pass by pass, the host loop's convergence groups, and every tile
geometry.  tests/test_thin_cpu.py shows on the CPU that the inputs have the features they are chosen for.

Everything but the product-entry check runs through prl_hip_internal_thin_passes of the test-hooks library, in one child process per
section (the hooks library cannot be loaded beside the product library).  A child stops at its first failing row; a child that died
(signal, GPU fault, time limit) fails its test, and no further child is started in the session."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import thin_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRL_ERR_BAD_ARG = 5

PACK_WIDTHS = list(range(1, 71)) + [1919, 1920, 1921, 1922]
PACK_FULL_WIDTHS = [1, 31, 32, 33, 65, 1921]          # all 8 x 8 alignment pairs
PACK_H, PACK_N = 5, 2
NB_RPS4_YSHIFT = 5
GEOM_RPS, GEOM_WPB = (4, 8, 16, 32, 64, 256), (1, 2, 3, 4)


# ---- what runs in the child --------------------------------------------------------------------------------------------------------

class Layout:
    """n pages of h x w bytes in a flat buffer: a guard row above and below every page, guard columns left and right of it up to the
    (odd) row step, the first pixel of page 0 at an address that is `align` modulo 8 (the buffer itself is 256-byte aligned; with an
    odd step the rows below take every other alignment in turn)."""

    def __init__(self, n, h, w, align, pad):
        self.n, self.h, self.w = n, h, w
        self.step = w + pad + (w + pad + 1) % 2
        self.page_stride = (h + 2) * self.step + 5
        self.left = 3
        self.off = (align - (self.step + self.left)) % 8 + 8
        self.first = self.off + self.step + self.left
        self.size = self.off + n * self.page_stride + 16
        assert self.step % 2 == 1 and self.first % 8 == align % 8

    def view(self, flat):
        return np.lib.stride_tricks.as_strided(flat[self.first:], (self.n, self.h, self.w), (self.page_stride, self.step, 1))


class Hook:
    def __init__(self):
        import ctypes as C

        import torch

        from prlib_amd import _capi

        _capi.use_library(_capi.HOOKS_LIB_PATH)
        self.C, self.torch, self.capi, self.L = C, torch, _capi, _capi.lib()
        vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
        self.L.prl_hip_internal_thin_passes.argtypes = [i, i, vp, sz, sz, i, i, vp, sz, sz, i, i, i, i, vp, vp, C.POINTER(C.c_int), vp]
        self.dev = torch.device("cuda:0")
        _capi.check(self.L.prl_hip_set_device(0))
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream

    def put(self, pages, align=0, fill=255):
        """Upload [n, h, w] bytes into a Layout whose guard bytes are `fill`: (device tensor, layout, the host copy)."""
        n, h, w = pages.shape
        lay = Layout(n, h, w, align, pad=9)
        flat = np.full(lay.size, fill, np.uint8)
        lay.view(flat)[:] = pages
        t = self.torch.from_numpy(flat).to(self.dev)
        assert t.data_ptr() % 256 == 0
        return t, lay, flat

    def raw(self, method, n, src_ptr, s_page, s_step, w, h, dst_ptr, d_page, d_step, n_passes, invert, rps, wpb, act_ptr, done_ptr):
        geom = (self.C.c_int * 4)()
        st = self.L.prl_hip_internal_thin_passes(method, n, src_ptr, s_page, s_step, w, h, dst_ptr, d_page, d_step, n_passes, invert, rps, wpb,
                                                 act_ptr, done_ptr, geom, self.stream)
        return st, list(geom)

    def run(self, src, method, n_passes, invert=0, rps=0, wpb=0, dst_align=0, flags=False):
        """One call of the hook on an uploaded batch.  Returns dict(out [n, h, w], guard: the destination's guard bytes are untouched,
        geom, and with flags: act [n, n_segs, n_strips], done [n], spare: the bytes after the activity bytes are untouched)."""
        torch = self.torch
        t, sl, _ = src
        n, h, w = sl.n, sl.h, sl.w
        dl = Layout(n, h, w, dst_align, pad=11)
        dst = torch.full((dl.size,), 7, dtype=torch.uint8, device=self.dev)
        assert dst.data_ptr() % 256 == 0
        cap = n * -(-h // 4) * -(-w // R.STRIP_PX) + 32
        act = torch.full((cap,), 9, dtype=torch.uint8, device=self.dev) if flags else None
        done = torch.full((n,), 5, dtype=torch.int32, device=self.dev) if flags else None
        st, geom = self.raw(method, n, t.data_ptr() + sl.first, sl.page_stride, sl.step, w, h, dst.data_ptr() + dl.first, dl.page_stride, dl.step,
                            n_passes, invert, rps, wpb, act.data_ptr() if flags else None, done.data_ptr() if flags else None)
        self.capi.check(st)
        torch.cuda.synchronize()
        g = dst.cpu().numpy()
        res = dict(out=dl.view(g).copy(), geom=geom)
        dl.view(g)[:] = 7
        res["guard"] = bool((g == 7).all())
        if flags:
            tiles = n * geom[3] * geom[1]
            a = act.cpu().numpy()
            res["act"], res["spare"] = a[:tiles].reshape(n, geom[3], geom[1]).copy(), bool((a[tiles:] == 9).all())
            res["done"] = done.cpu().numpy().copy()
        return res


class Rows:
    """The rows a child reports; add() is False from the first row that is not ok on, and the job stops there."""

    def __init__(self):
        self.rows = []

    def add(self, ok, **what):
        self.rows.append(dict(ok=bool(ok), **what))
        return bool(ok)


def u8(planes):
    return np.asarray(planes, bool).astype(np.uint8) * 255


def job_pack(hk, rows):
    """A: n_passes = 0.  Random bytes, source padding 255; want ((src & 1) ^ invert) * 255, guard bytes and the source untouched."""
    rng = np.random.default_rng(31)
    for w in PACK_WIDTHS:
        pages = rng.integers(0, 256, (PACK_N, PACK_H, w), dtype=np.uint8)
        for sa in range(8):
            src = hk.put(pages, sa)
            for da in (range(8) if w in PACK_FULL_WIDTHS else [(3 * sa + 1) % 8]):
                for invert in (0, 1):
                    r = hk.run(src, 0, 0, invert=invert, dst_align=da)
                    want = ((pages & 1) ^ invert) * 255
                    if not rows.add(np.array_equal(r["out"], want) and r["guard"], w=w, sa=sa, da=da, invert=invert,
                                    bad=int((r["out"] != want).sum()), guard=r["guard"]):
                        return
            if not rows.add(np.array_equal(src[0].cpu().numpy(), src[2]), w=w, sa=sa, source_unchanged=True):
                return


def job_single(hk, rows, seam):
    """B: the neighbourhood block as a batch of its 32 x-shifts, per y-shift and method after 1, 2 and 3 passes; one y-shift again on
    tiles of 4 rows."""
    for ys in range(R.NB_YSHIFTS):
        win, pages = R.nb_batch(seam, ys)
        src = hk.put(u8(win.paste(pages)), ys % 8)
        for method in (0, 1):
            for rps in ((0, 4) if ys == NB_RPS4_YSHIFT else (0,)):
                want = pages
                for n in (1, 2, 3):
                    want = R.one_pass(want, method, win.edges)
                    r = hk.run(src, method, n, rps=rps, dst_align=(ys + n) % 8)
                    got = r["out"]
                    bad = int((win.cut(got) != u8(want)).sum())
                    geom_ok = r["geom"] == [-(-win.width // 32), 2 if seam else 1, rps or 16, -(-win.height // (rps or 16))]
                    if not rows.add(bad == 0 and win.outside_is_zero(got) and r["guard"] and geom_ok, ys=ys, method=method, rps=rps, n=n,
                                    bad=bad, guard=r["guard"], geom=r["geom"], changed=int((want != pages).sum())):
                        return


def job_borders(hk, rows):
    """C: foreground on all four page edges, after one pass and at convergence."""
    for h, w in R.border_shapes():
        pages = np.stack(R.border_pages(h, w))
        src = hk.put(u8(pages), (h + w) % 8)
        for method in (0, 1):
            for n, want in ((1, R.one_pass(pages, method)), (-1, R.passes(pages, method)[-1])):
                r = hk.run(src, method, n, dst_align=(3 * w + h) % 8)
                bad = int((r["out"] != u8(want)).sum())
                if not rows.add(bad == 0 and r["guard"], h=h, w=w, method=method, n=n, bad=bad, guard=r["guard"]):
                    return


def activity_scenarios():
    """(name, method, rps asked of the hook, rps in force, window, content)"""
    for x_start in (32, 33):
        yield (f"zigzag{x_start}", 0, R.ZIGZAG_RPS, R.ZIGZAG_RPS) + R.zigzag(x_start)
    for method in (0, 1):
        yield (f"slab{method}", method, 0, 16) + R.seam_slab()
        yield (f"block{method}", method, R.BLOCK_RPS, R.BLOCK_RPS) + R.anchored_block()


def job_activity(hk, rows):
    """D: after every pass count the plane, the activity bytes the last pass wrote and the done flag; two counts past convergence."""
    for name, method, rps_arg, rps, win, im in activity_scenarios():
        seq, maps = R.change_maps(im, method, win, rps)
        src = hk.put(u8(win.paste(im))[None], 3)
        acts = []
        for n in range(1, len(seq) + 3):
            r = hk.run(src, method, n, rps=rps_arg, flags=True, dst_align=n % 8)
            k = min(n, len(seq))
            bad = int((win.cut(r["out"][0]) != u8(seq[k - 1])).sum())
            ok = bad == 0 and win.outside_is_zero(r["out"]) and r["guard"] and r["spare"] and r["geom"][2] == rps
            ok = ok and int(r["done"][0]) == (1 if n >= len(seq) else 0)
            act_bad = -1
            if n <= len(seq):
                act_bad = int((r["act"][0] != maps[n - 1]).sum()) if r["act"][0].shape == maps[n - 1].shape else 10 ** 6
                ok = ok and act_bad == 0
                acts.append(r["act"][0])
            if not rows.add(ok, name=name, n=n, passes=len(seq), bad=bad, act_bad=act_bad, done=int(r["done"][0]), guard=r["guard"],
                            spare=r["spare"], geom=r["geom"]):
                return
        a = np.stack(acts)                               # [pass, seg, strip]
        idle_then_active = False
        for p in range(len(a) - 1):
            idle_then_active = idle_then_active or bool(((a[p] == 0) & (a[p + 1:] == 1).any(axis=0)).any())
        if not rows.add(idle_then_active, name=name, idle_then_active=idle_then_active):
            return


def bar_batch():
    return np.stack([R.bar_page(t) for t in R.BAR_THICKNESS] + [np.zeros((R.BAR_H, R.BAR_W), bool)])


BAR_COUNTS = R.BAR_PASSES + (1,)       # (the empty page's first pass changes nothing)


def job_groups(hk, rows):
    """E: the ten bars and an empty page in one batch: the product's loop equals the oracle; with exact counts every page equals the
    reference after that many passes and its done flag flips at its own count."""
    from oracle import capi as oracle

    pages = bar_batch()
    src = hk.put(u8(pages), 5)
    for method in (0, 1):
        seqs = [R.passes(p, method) for p in pages]
        counts = [len(s) for s in seqs]
        if not rows.add(tuple(counts) == BAR_COUNTS, method=method, counts=counts):
            return
        r = hk.run(src, method, -1, flags=True)
        bad = [int((r["out"][i] != oracle.thin(u8(pages[i]), method)).sum()) for i in range(len(pages))]
        if not rows.add(not any(bad) and r["guard"] and (r["done"] == 1).all(), method=method, n=-1, bad=bad, guard=r["guard"],
                        done=r["done"].tolist()):
            return
        for n in range(0, max(counts) + 2):
            r = hk.run(src, method, n, flags=True, dst_align=n % 8)
            want = np.stack([pages[i] if n == 0 else seqs[i][min(n, counts[i]) - 1] for i in range(len(pages))])
            bad = int((r["out"] != u8(want)).sum())
            done_want = [1 if n >= c else 0 for c in counts]
            if not rows.add(bad == 0 and r["guard"] and r["done"].tolist() == done_want, method=method, n=n, bad=bad, guard=r["guard"],
                            done=r["done"].tolist()):
                return


def job_geometry(hk, rows, env_knobs):
    """F: one page on every tile height and workgroup size; or (env_knobs) on what PRL_THIN_RPS / PRL_THIN_WPB say."""
    im = R.geometry_page()
    src = hk.put(u8(im)[None], 1)
    for method in (0, 1):
        want = u8(R.passes(im, method)[-1])
        combos = [(0, 0)] if env_knobs else [(0, 0)] + [(rps, wpb) for rps in GEOM_RPS for wpb in GEOM_WPB]
        for rps, wpb in combos:
            r = hk.run(src, method, -1, rps=rps, wpb=wpb, dst_align=(rps + wpb) % 8)
            bad = int((r["out"][0] != want).sum())
            rps_want = rps or (4 if env_knobs else 16)
            geom_ok = r["geom"] == [63, 2, rps_want, -(-70 // rps_want)]
            if not rows.add(bad == 0 and r["guard"] and geom_ok, method=method, rps=rps, wpb=wpb, bad=bad, guard=r["guard"], geom=r["geom"]):
                return
    if env_knobs:
        return
    # what the entry refuses, before anything is enqueued: more pages than one chunk, rps 1 .. 3, wpb outside 0 .. 4, n_passes < -1
    t, sl, _ = src
    d = hk.torch.zeros((sl.size,), dtype=hk.torch.uint8, device=hk.dev)

    def status(n_pages=1, n_passes=1, rps=0, wpb=0, method=0):
        return hk.raw(method, n_pages, t.data_ptr() + sl.first, sl.page_stride if n_pages == 1 else 0, sl.step, sl.w, sl.h,
                      d.data_ptr() + sl.first, sl.page_stride if n_pages == 1 else 0, sl.step, n_passes, 0, rps, wpb, None, None)[0]

    errs = [status(n_pages=32769), status(rps=3), status(rps=1), status(wpb=5), status(wpb=-1), status(n_passes=-2), status(method=2)]
    hk.torch.cuda.synchronize()
    rows.add(errs == [PRL_ERR_BAD_ARG] * 7 and not bool(d.any()), errs=errs)


JOBS = {"pack": lambda hk, rows: job_pack(hk, rows), "single_near": lambda hk, rows: job_single(hk, rows, False),
        "single_seam": lambda hk, rows: job_single(hk, rows, True), "borders": job_borders, "activity": job_activity, "groups": job_groups,
        "geometry": lambda hk, rows: job_geometry(hk, rows, False), "geometry_env": lambda hk, rows: job_geometry(hk, rows, True)}


def child_main(section):
    t0 = time.time()
    hk, rows = Hook(), Rows()
    t1 = time.time()
    JOBS[section](hk, rows)
    print("ROWS " + json.dumps(dict(rows=rows.rows, start_s=round(t1 - t0, 2), job_s=round(time.time() - t1, 2))))


# ---- the parent --------------------------------------------------------------------------------------------------------------------

_CHILD = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_thin_gpu as T; T.child_main(%r)"
_results = {}


def _child(section):
    """The rows of a section's child, run once per session, every row ok."""
    if section in _results:
        assert not isinstance(_results[section], str), f"the child failed before and is not started again: {_results[section]}"
        return _results[section]
    dead = [f"{k}: {v}" for k, v in _results.items() if isinstance(v, str)]
    assert not dead, f"an earlier child died; no further child is started: {dead}"
    env = {k: v for k, v in os.environ.items() if k not in ("PRL_THIN_RPS", "PRL_THIN_WPB", "PRL_HIP_STAGE_CHUNK")}
    if section == "geometry_env":
        env.update(PRL_THIN_RPS="4", PRL_THIN_WPB="1")
    _results[section] = "did not finish"
    t0 = time.time()
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"), section)], capture_output=True, text=True,
                       timeout=120, env=env)
    if r.returncode != 0 or "illegal memory access" in r.stderr:
        _results[section] = f"exit {r.returncode}: {r.stderr[-2000:]}"
    assert r.returncode == 0 and "illegal memory access" not in r.stderr, (r.returncode, r.stdout[-2000:] + r.stderr[-2000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("ROWS ")]
    assert lines, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(lines[0][5:])
    print(f"thin child {section}: {time.time() - t0:.1f} s (start {res['start_s']} s, job {res['job_s']} s), {len(res['rows'])} rows")
    _results[section] = res["rows"]
    bad = [x for x in res["rows"] if not x["ok"]]
    assert not bad, bad[0]
    return res["rows"]


def _all_ok(rows, count):
    bad = [x for x in rows if not x["ok"]]
    assert not bad, bad[0]
    assert len(rows) == count, (len(rows), count)


def test_pack_and_unpack_at_every_alignment(prl, cuda_device):
    """k_thin_pack and k_thin_unpack alone (no pass): widths 1 .. 70 and 1919 .. 1922, source rows at every address modulo 8 (odd row
    steps), destination alignment (3 i + 1) % 8 - all 8 x 8 pairs at widths 1, 31, 32, 33, 65, 1921 - plain and inverted; random
    bytes of which only bit 0 counts, 255 around the source; the destination's guard bytes and the source stay as they were."""
    rows = _child("pack")
    calls = [x for x in rows if "invert" in x]
    _all_ok(rows, sum(8 * (8 if w in PACK_FULL_WIDTHS else 1) * 2 + 8 for w in PACK_WIDTHS))
    assert {(x["sa"], x["da"]) for x in calls if x["w"] == 1921} == {(a, b) for a in range(8) for b in range(8)}
    assert {x["w"] for x in calls} == set(PACK_WIDTHS) and {x["invert"] for x in calls} == {0, 1}


@pytest.mark.parametrize("seam", [False, True], ids=["near_x0", "across_the_seam"])
def test_single_passes_over_every_neighbourhood(prl, cuda_device, seam):
    """k_thin_pass after exactly 1, 2 and 3 passes on all 512 neighbourhoods at every bit and row position, both methods, the block
    near x = 0 and across the seam at x = 1920 (lanes 61 and 2 take their neighbour words from halo lanes); y-shift 5 also on tiles
    of 4 rows.  Nothing appears outside the block's window."""
    rows = _child("single_seam" if seam else "single_near")
    _all_ok(rows, (R.NB_YSHIFTS + 1) * 2 * 3)
    assert {(x["ys"], x["method"], x["n"]) for x in rows} == {(y, m, n) for y in range(16) for m in (0, 1) for n in (1, 2, 3)}
    assert sum(x["rps"] == 4 for x in rows) == 6 and all(x["changed"] > 1000 for x in rows)


def test_borders_at_every_ragged_size(prl, cuda_device):
    """Rows 0 and height - 1, columns 0 and width - 1 are never marked: pages with foreground on all four edges (full, frame,
    noise) at every width of {1 .. 3, 31 .. 34, 63 .. 65, 1919 .. 1922} and height of {1 .. 4, 15 .. 18, 31 .. 33}: the last column on
    bit 0, bit 31, the first word of the second strip; after one pass and at convergence."""
    rows = _child("borders")
    _all_ok(rows, len(R.border_shapes()) * 4)
    assert {x["w"] for x in rows} == set(R.BORDER_WIDTHS) and {x["h"] for x in rows} == set(R.BORDER_HEIGHTS)


def test_activity_tracking_pass_by_pass(prl, cuda_device):
    """The scenarios of test_thin_cpu.py (wake-ups from the same strip, the same segment, diagonally, the other strip only; tiles
    that idle and run again): after every pass count the plane equals the reference's, the activity bytes equal the reference's
    change map of that pass (a skipped tile reads 0), the done flag is 0 before the reference's pass count and 1 from there on, and
    some tile reads 0 in one pass and 1 in a later one."""
    rows = _child("activity")
    per = {}
    for name, method, _, rps, win, im in activity_scenarios():
        per[name] = len(R.passes(im, method, win.edges)) + 2
    _all_ok(rows, sum(per.values()) + len(per))
    assert {x["name"] for x in rows} == set(per)
    for name in per:
        assert sum(1 for x in rows if x["name"] == name and "n" in x) == per[name]
        assert [x for x in rows if x["name"] == name and "idle_then_active" in x][0]["idle_then_active"]


@pytest.mark.parametrize("method", [0, 1], ids=["zhangsuen", "guohall"])
def test_convergence_groups(prl, oracle, cuda_device, method):
    """Pages of one batch that converge after 1, 2, 4, 5, 12, 13, 28, 29, 60 and 61 passes - either side of every host check of the
    loop (4, 12, 28, 60), odd and even - and an empty page: the product entry and the hook's loop equal the oracle on every page;
    with exact counts 0 .. 62 every page equals the reference and its done flag flips at its own count."""
    import torch

    pages = u8(bar_batch())
    fn = prl.thinZhangSuen if method == 0 else prl.thinGuoHall
    got = fn(torch.from_numpy(pages).to(cuda_device)).cpu().numpy()
    for i in range(len(pages)):
        want = oracle.thin(pages[i], method)
        assert np.array_equal(got[i], want), (i, int((got[i] != want).sum()))
    rows = [x for x in _child("groups") if x["method"] == method]
    _all_ok(rows, 2 + max(BAR_COUNTS) + 2)
    assert [x["n"] for x in rows[1:]] == [-1] + list(range(0, 63))
    for x in rows[2:]:
        assert x["done"] == [1 if x["n"] >= c else 0 for c in BAR_COUNTS]


def test_every_tile_geometry(prl, cuda_device):
    """Text and discs across x = 1920 on a 70 x 2000 page: the same skeleton on tiles of 4, 8, 16, 32, 64 and 256 rows with 1 .. 4
    wavefronts per workgroup, and the geometry the entry reports is the one asked for; the entry's argument errors."""
    rows = _child("geometry")
    _all_ok(rows, 2 * (1 + len(GEOM_RPS) * len(GEOM_WPB)) + 1)
    assert {(x["rps"], x["wpb"]) for x in rows if "rps" in x} == {(0, 0)} | {(r, w) for r in GEOM_RPS for w in GEOM_WPB}
    assert rows[-1]["errs"] == [PRL_ERR_BAD_ARG] * 7


def test_geometry_from_the_environment_knobs(prl, cuda_device):
    """PRL_THIN_RPS=4 PRL_THIN_WPB=1 (read by the test-hooks library only) with rps = wpb = 0: tiles of 4 rows, the same skeleton."""
    rows = _child("geometry_env")
    _all_ok(rows, 2)
    assert all(x["geom"] == [63, 2, 4, 18] for x in rows)
