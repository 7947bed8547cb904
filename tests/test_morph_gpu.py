"""The mask morphology kernels of morph.hip, each launched directly on masks that aim at its boundaries
(prl_hip_internal_mask_morph / prl_hip_internal_pack_mask of the test-hooks build), against tests/morph_ref.py.

The binarizers hand the morphology pass their own mask buffer, which is always 16-byte aligned: through them only k_morph_bits
(radius <= 4) and k_morph_stream (radius 5..8) can run, and a thresholded noise page closes to all white for every radius >= 2
(morphology).  Here the caller's mask decides: the product's dispatch (morph_binary_run / morph_bitplane_run) picks the
kernel from the alignment of the source and the radius, the entry reports which one ran, and every comparison is exact.

One child process runs all cases (the case list below is plain data and is checked on the CPU by tests/test_morph_cpu.py)."""
import zlib

import numpy as np
import pytest

import morph_ref as mr

# ---- the kernels' geometry (constants of prlib_amd/csrc/morph.hip; test_morph_cpu.py checks them against the source) -------------------
BITS_MAX_N = 4          # kBitsMaxN
BITS_ADVANCE = 2000     # kBitsAdvance: output pixels per strip of k_morph_bits
BITS_LEAD = 32          # base_px = strip * kBitsAdvance - 32
BITS_CHUNK = 16         # pixels per chunk; a lane owns chunks L and 64 + L: chunk 63 | 64 meets at base_px + 1024
BITS_RB = 4             # RB: rows fetched together
BITS_RPS = (64, 8)      # launch_morph_bits: rows per segment, and what it shrinks to on a small batch
STREAM_RPS = (128, 32)  # morph_binary_run, k_morph_stream
MAX_N = 8               # kMaxN
BND, BTH = 64, 32       # k_morph_binary: staged dwords per row, tile height
GUARD = 0x5A            # what every destination buffer is filled with (neither 0 nor 255)

KERNEL_NAMES = {1: "k_morph_bits<byte source>", 2: "k_morph_bits<bit source>", 3: "k_morph_stream", 4: "k_morph_binary"}


def stream_useful(m):   # output pixels per strip of k_morph_stream: 240 for m <= 4, 224 above
    return (64 - 2 * (2 * ((m + 3) // 4))) * 4


def binary_btw(m):      # output pixels per tile row of k_morph_binary: 232, 232, 224, 224, 216, 216, 208, 208
    return BND * 4 - 2 * (((2 * m + 3) // 4) * 4 + 8)


def ceil_to(x, a):
    return (x + a - 1) // a * a


def predicted_kernel(form, n, src_off, src_step, src_page_stride, w):
    """the dispatch rule of morph_binary_run / morph_bitplane_run, restated: the coverage test holds the library to it"""
    if form == 1:
        return 2
    al = src_off | src_step | src_page_stride
    if abs(n) <= BITS_MAX_N and al % 16 == 0 and src_step >= ceil_to(w, 16):
        return 1
    return 3 if al % 4 == 0 else 4


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
BITS_WIDTHS = [1, 15, 16, 17, 33, 991, 992, 993, 1008, 1009, 1985, 2000, 2001, 2016, 2033, 2993, 4001]
HEIGHTS = [1, 2, "m", "2m", "2m+1", 7, 8, 9, 13, 63, 64, 65, 129]
STREAM_WIDTHS = [1, 3, 4, 5, 223, 224, 225, 239, 240, 241, 449, 481, 700]
ALIGN_WIDTHS = [17, 993, 2001, 2033]
PACK_WIDTHS = [1, 7, 8, 9, 2047, 2048, 2049]


def _height(hh, m):
    return {"m": m, "2m": 2 * m, "2m+1": 2 * m + 1}.get(hh, hh)


def heights(m):
    return sorted({_height(hh, m) for hh in HEIGHTS})


def _tall(m):
    """rows that show every (split, gap) combination of the horizontal gap pairs on one page, at most 140"""
    return min(140, 2 * (2 * m + 1) * (m + 1))


def bits_xs(w, a):
    """chunk edges near both page edges, chunk 63 | 64 of strips 0 and 1, the strip seams (as the source and as the destination
    sees them: the destination's 16-byte chunks lie `a` pixels to the left of the source's)"""
    c = [BITS_CHUNK, 2 * BITS_CHUNK, BITS_CHUNK - a, (w // 16) * 16, ((w - 1) // 16) * 16, (w // 16) * 16 - a,
         1024 - BITS_LEAD, 1024 - BITS_LEAD - a, BITS_ADVANCE + 1024 - BITS_LEAD,
         BITS_ADVANCE - BITS_LEAD, BITS_ADVANCE - a, BITS_ADVANCE, 2 * BITS_ADVANCE - a, 2 * BITS_ADVANCE]
    return sorted({b for b in c if 0 < b < w})


def seg_ys(h, seg, extra=()):
    """every multiple of the segment height, and the first row block"""
    return sorted({y for y in list(range(seg, h + 1, seg)) + list(extra) if 0 < y <= h})


def _src_layout(kind, w, h, form):
    """(offset of page 0 row 0 in the buffer, row step, page stride) for a source of the given alignment class"""
    if form == 1:
        step = ceil_to(w, 16) // 8 + {"bits": 0, "bits+2": 2, "bits+6": 6}[kind]
        return (2 if kind != "bits" else 0), step, ceil_to(step * h + 2, 2)
    if kind == "a16":
        step = ceil_to(w, 16)
        return 0, step, step * h + 32
    if kind == "a16wide":
        step = ceil_to(w, 16) + 48
        return 16, step, step * h + 16
    if kind == "a4":            # 4-byte aligned and not 16
        step = ceil_to(w, 4) + 4
        return 4, step, ceil_to(step * h + 4, 4)
    if kind == "a4row":         # 16-byte aligned base, rows 4 mod 16 apart
        step = ceil_to(w, 16) + 4
        return 0, step, ceil_to(step * h, 16)
    if kind == "base+1":
        step = ceil_to(w, 4) + 8
        return 1, step, step * h + 4
    if kind == "oddstep":
        step = w + 1 + (w % 2)    # odd for every w
        return 0, step, step * h + 1
    raise ValueError(kind)


def _dst_layout(kind, w, h, a=0):
    """(offset of page 0 row 0, row step, page stride); `a` = address of row 0 mod 16 where the step is a multiple of 16"""
    if kind == "a":             # every row has address a mod 16
        step = ceil_to(w + a, 16) + 16
        return step + a, step, step * (h + 2) + 48
    if kind == "w":             # rows back to back: the address mod 16 changes every row (for a width that is no multiple of 16)
        return w + 16, w, w * (h + 2) + 7
    if kind == "w+1":
        return w + 1 + 16, w + 1, (w + 1) * (h + 2) + 3
    if kind == "a4":
        step = ceil_to(w, 4) + 4
        return step + 4, step, step * (h + 2)
    if kind == "base+1":
        step = ceil_to(w, 4) + 4
        return step + 1, step, step * (h + 2)
    if kind == "odd":
        step = w + 1 + (w % 2)    # odd for every w
        return step, step, step * (h + 2) + 2
    raise ValueError(kind)


def _case(name, form, n, w, h, xs, ys, src, dst, a=0, rps=0, fill=0, seed=1, kinds=None, flat=False, tag=None, max_phases=6, phase0=0):
    so, ss, sp = _src_layout(src, w, h, form)
    do, ds, dp = _dst_layout(dst, w, h, a)
    return dict(name=f"{name}/n{n}/f{form}", form=form, n=n, w=w, h=h, xs=list(xs), ys=list(ys), rps=rps, fill=fill, seed=seed,
                kinds=kinds, flat=flat, max_phases=max_phases, phase0=phase0, src=src, src_off=so, src_step=ss, src_page_stride=sp, dst=dst, a=a,
                dst_off=do, dst_step=ds, dst_page_stride=dp, expect=predicted_kernel(form, n, so, ss, sp, w), tag=tag or src)


def cases():
    """every call family of the issue, as plain dictionaries"""
    out = []
    # -- k_morph_bits: 4 radii x closing / opening x byte / bit source
    for form in (0, 1):
        srcs = ("a16", "a16wide") if form == 0 else ("bits", "bits+2", "bits+6")
        for n in [s * m for m in range(1, BITS_MAX_N + 1) for s in (1, -1)]:
            m = abs(n)
            # widths: the pages are tall enough for every split around every boundary column
            for i, w in enumerate(BITS_WIDTHS):
                a = (5 * i + 3 * m + form) % 16
                h = _tall(m)
                out.append(_case(f"bits/w{w}", form, n, w, h, bits_xs(w, a), seg_ys(h, BITS_RPS[1], (BITS_RB, h - 1)),
                                 srcs[i % len(srcs)], "a", a, fill=255 * (i & 1), seed=10 + i, flat=w in (1, 17, 2033),
                                 kinds=("gap_h", "bar_h", "random", "edges")))
            # heights x rows per segment (0: the library's choice, which is 8 for calls this small)
            for rps in (0, 8, 64):
                seg = rps or BITS_RPS[1]
                for k, h in enumerate(heights(m)):
                    a = (7 * k + m) % 16
                    out.append(_case(f"bits/h{h}/rps{rps}", form, n, 100, h, [BITS_CHUNK, 96], seg_ys(h, seg, (BITS_RB, h - 1)),
                                     srcs[k % len(srcs)], "a", a, rps=rps, seed=40 + k, kinds=("gap_v", "bar_v", "random"),
                                     max_phases=1, phase0=k + rps // 8))
            # destination alignment: every a with a step that keeps it, and steps that change it every row
            for w in (ALIGN_WIDTHS if m in (1, BITS_MAX_N) else ALIGN_WIDTHS[-1:]):
                h = _tall(m)
                for a in range(16):
                    out.append(_case(f"bits/align/w{w}/a{a}", form, n, w, h, bits_xs(w, a), [], srcs[a % len(srcs)], "a", a,
                                     fill=255 * (a & 1), seed=70 + a, kinds=("gap_h", "bar_h")))
                for dst in ("w", "w+1"):
                    xs = sorted({b - a for b in (BITS_CHUNK, (w // 16) * 16, BITS_ADVANCE) for a in (0, 5, 10, 15) if 0 < b - a < w})
                    out.append(_case(f"bits/align/w{w}/{dst}", form, n, w, h, xs, [], srcs[0], dst, seed=90,
                                     kinds=("gap_h", "bar_h", "random")))
            # source row padding: the same pages with the padding all ones and all zeros
            for w in (17, 993, 2001):
                for fill in (0, 255):
                    out.append(_case(f"bits/pad/w{w}/fill{fill}", form, n, w, 2 * m + 5, bits_xs(w, 0), [BITS_RB], srcs[-1], "a", 9,
                                     fill=fill, seed=95, kinds=("gap_h", "random", "edges"), tag="pad"))
    # -- k_morph_stream: 8 radii x closing / opening
    for n in [s * m for m in range(1, MAX_N + 1) for s in (1, -1)]:
        m = abs(n)
        use = stream_useful(m)
        dsts = ("a4", "base+1", "odd")
        for i, w in enumerate(STREAM_WIDTHS):
            h = _tall(m)
            xs = sorted({b for b in (4, 8, use - 4, use, use + 4, 2 * use, (w // 4) * 4, ((w - 1) // 4) * 4) if 0 < b < w})
            out.append(_case(f"stream/w{w}", 0, n, w, h, xs, seg_ys(h, STREAM_RPS[1], (1, h - 1)), "a4" if i % 3 else "a4row",
                             dsts[i % 3], fill=255 * (i & 1), seed=110 + i, flat=w in (1, 241),
                             kinds=("gap_h", "bar_h", "random", "edges")))
        for rps in (0, 32, 128):
            seg = rps or STREAM_RPS[1]
            for k, h in enumerate(heights(m)):
                out.append(_case(f"stream/h{h}/rps{rps}", 0, n, 100, h, [48], seg_ys(h, seg, (1, h - 1)), "a4", dsts[k % 3],
                                 rps=rps, seed=140 + k, kinds=("gap_v", "bar_v", "random"), max_phases=1, phase0=k + rps // 32))
        if m > BITS_MAX_N:   # what the binarizers reach: a 16-byte aligned source
            out.append(_case("stream/a16", 0, n, 481, 65, [use, 2 * use], [STREAM_RPS[1], 64], "a16", "a", 0, seed=170, tag="a16"))
    # -- k_morph_binary: 8 radii x closing / opening, from a source at base + 1 and from one with an odd row step
    for n in [s * m for m in range(1, MAX_N + 1) for s in (1, -1)]:
        m = abs(n)
        btw = binary_btw(m)
        full = m in (1, 2, 3, 8)
        shapes = [(w, h) for w in (btw - 1, btw, btw + 1, 2 * btw + 1) for h in (BTH - 1, BTH, BTH + 1, 2 * BTH + 1)] if full \
            else [(btw + 1, BTH + 1), (2 * btw, 2 * BTH)]
        for k, (w, h) in enumerate(shapes):
            for j, src in enumerate(("base+1", "oddstep")):
                xs = sorted({b for b in (4, btw - 4, btw, btw + 4, 2 * btw, (w // 4) * 4) if 0 < b < w})
                out.append(_case(f"binary/{src}/{w}x{h}", 0, n, w, h, xs, seg_ys(h, BTH), src, ("a4", "base+1", "odd")[(k + j) % 3],
                                 fill=255 * (k & 1), seed=200 + k, flat=k == 0, max_phases=2 if full else 1))
    return out


_page_cache = {}


def case_pages(c):
    """[(name, page, reference)] of a case; pages and references are computed once per (radius, shape, boundaries, seed)"""
    key = (c["n"], c["h"], c["w"], tuple(c["xs"]), tuple(c["ys"]), c["seed"], c["max_phases"], c["phase0"], c["flat"])
    if key not in _page_cache:
        pages = mr.pages_for(c["n"], c["h"], c["w"], c["xs"], c["ys"], c["seed"], c["max_phases"], c["phase0"])
        if c["flat"]:
            pages += mr.flat_pages(c["h"], c["w"])
        _page_cache[key] = [(name, p, None) for name, p in pages]
    got = _page_cache[key]
    if c["kinds"]:
        keep = [i for i, (name, _, _) in enumerate(got) if name.rstrip("0123456789") in c["kinds"] or name.startswith("all")]
    else:
        keep = list(range(len(got)))
    for i in keep:
        if got[i][2] is None:
            got[i] = (got[i][0], got[i][1], mr.close_open(got[i][1], c["n"]))
    return [got[i] for i in keep]


def batches(pages, size=3):
    return [pages[i:i + size] for i in range(0, len(pages), size)]


def _rows_view(buf, off, step, h, w):
    return np.lib.stride_tricks.as_strided(buf[off:], shape=(h, w), strides=(step, 1))


def source_buffer(c, pages):
    """the caller's source buffer of one call: pages at their stride, every other byte (and every padding bit) = fill"""
    h, w = c["h"], c["w"]
    size = c["src_off"] + len(pages) * c["src_page_stride"] + c["src_step"] + 64
    buf = np.full(size, c["fill"], np.uint8)
    for k, (_, p, _) in enumerate(pages):
        off = c["src_off"] + k * c["src_page_stride"]
        if c["form"] == 0:
            _rows_view(buf, off, c["src_step"], h, w)[:] = mr.to_bytes(p)
        else:
            padded = np.full((h, ceil_to(w, 16)), bool(c["fill"]))
            padded[:, :w] = p
            bits = mr.pack_rows(padded)
            _rows_view(buf, off, c["src_step"], h, bits.shape[1])[:] = bits
    return buf


def expected_buffer(c, pages):
    size = c["dst_off"] + len(pages) * c["dst_page_stride"] + c["dst_step"] + 64
    buf = np.full(size, GUARD, np.uint8)
    for k, (_, _, ref) in enumerate(pages):
        _rows_view(buf, c["dst_off"] + k * c["dst_page_stride"], c["dst_step"], c["h"], c["w"])[:] = mr.to_bytes(ref)
    return buf


def result_row(c, b, pages, status, kernel_run, got):
    """what the tests assert on, for one call (runs in the child)"""
    want = expected_buffer(c, pages)
    bad = got != want
    diff, not01, crc = [], 0, 0
    for k in range(len(pages)):
        off = c["dst_off"] + k * c["dst_page_stride"]
        diff.append(int(_rows_view(bad, off, c["dst_step"], c["h"], c["w"]).sum()))
        inside = np.ascontiguousarray(_rows_view(got, off, c["dst_step"], c["h"], c["w"]))
        not01 += int(((inside != 0) & (inside != 255)).sum())
        crc = zlib.crc32(inside.tobytes(), crc)
    return dict(case=c["name"], batch=b, pages=[name for name, _, _ in pages], n=c["n"], form=c["form"], tag=c["tag"], w=c["w"],
                h=c["h"], a=c["a"], dst=c["dst"], rps=c["rps"], expect=c["expect"], status=int(status), kernel_run=int(kernel_run),
                diff=diff, not01=not01, guard=int(bad.sum()) - sum(diff), crc=crc,
                distinct=len({p.tobytes() for _, p, _ in pages}))


def pack_cases():
    out = []
    for w in PACK_WIDTHS:
        for values in ((0, 255), (0, 1, 254, 255)):
            src = np.random.default_rng(w).choice(np.array(values, np.uint8), size=(5, w))
            out.append((w, values, src, mr.pack_rows((src & 1).astype(bool))))
    return out


def bad_arg_calls():
    """(name, form, iterations, width, src_step): the argument errors of the two *_run functions; 16 x 40 pages otherwise"""
    return [("radius 0", 0, 0, 40, 48), ("radius 9", 0, 9, 40, 48), ("radius -9", 0, -9, 40, 48), ("bit plane radius 5", 1, 5, 40, 6),
            ("bit plane radius 0", 1, 0, 40, 6), ("bit plane odd step", 1, 2, 40, 7), ("bit plane short step", 1, -2, 40, 4)]


_CHILD = r'''
import ctypes as C, json, sys, time
import numpy as np, torch
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from prlib_amd import _capi
_capi.use_library(_capi.HOOKS_LIB_PATH)
import test_morph_gpu as T
L = _capi.lib()
vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
L.prl_hip_internal_mask_morph.argtypes = [i, i, i, i, vp, sz, sz, i, i, vp, sz, sz, C.POINTER(C.c_int), vp]
L.prl_hip_internal_pack_mask.argtypes = [vp, sz, i, i, vp, sz, vp]
dev = torch.device("cuda:0")
_capi.check(L.prl_hip_set_device(0))
stream = torch.cuda.current_stream(dev).cuda_stream
t0 = time.time()
rows = []
for c in T.cases():
    for b, pages in enumerate(T.batches(T.case_pages(c))):
        src = torch.from_numpy(T.source_buffer(c, pages)).to(dev)
        dst = torch.full((c["dst_off"] + len(pages) * c["dst_page_stride"] + c["dst_step"] + 64,), T.GUARD, dtype=torch.uint8, device=dev)
        assert src.data_ptr() %% 16 == 0 and dst.data_ptr() %% 16 == 0
        kr = C.c_int(-1)
        st = L.prl_hip_internal_mask_morph(c["form"], c["n"], c["rps"], len(pages), src.data_ptr() + c["src_off"], c["src_page_stride"],
                                           c["src_step"], c["w"], c["h"], dst.data_ptr() + c["dst_off"], c["dst_page_stride"],
                                           c["dst_step"], C.byref(kr), stream)
        torch.cuda.synchronize()
        rows.append(T.result_row(c, b, pages, st, kr.value, dst.cpu().numpy()))
packs = []
for w, values, src, want in T.pack_cases():
    h, step, bstep = src.shape[0], w + 3, want.shape[1] + 2
    sbuf = np.full(h * step + 8, 255, np.uint8)
    T._rows_view(sbuf, 0, step, h, w)[:] = src
    d_src = torch.from_numpy(sbuf).to(dev)
    d_bits = torch.full((h * bstep + 8,), T.GUARD, dtype=torch.uint8, device=dev)
    st = L.prl_hip_internal_pack_mask(d_src.data_ptr(), step, w, h, d_bits.data_ptr(), bstep, stream)
    torch.cuda.synchronize()
    got = d_bits.cpu().numpy()
    exp = np.full(h * bstep + 8, T.GUARD, np.uint8)
    T._rows_view(exp, 0, bstep, h, want.shape[1])[:] = want
    inside = int((T._rows_view(got, 0, bstep, h, want.shape[1]) != want).sum())
    packs.append(dict(w=w, values=list(values), status=int(st), diff=inside, guard=int((got != exp).sum()) - inside))
errs = []
one = torch.zeros((4096,), dtype=torch.uint8, device=dev)
for name, form, it, w, step in T.bad_arg_calls():
    out = torch.full((4096,), T.GUARD, dtype=torch.uint8, device=dev)
    kr = C.c_int(-1)
    st = L.prl_hip_internal_mask_morph(form, it, 0, 1, one.data_ptr(), step * 16, step, w, 16, out.data_ptr(), 64 * 16, 64, C.byref(kr), stream)
    torch.cuda.synchronize()
    errs.append(dict(name=name, status=int(st), kernel_run=kr.value, touched=int((out != T.GUARD).sum().item())))
print("ROWS " + json.dumps(dict(rows=rows, packs=packs, errs=errs, seconds=time.time() - t0)))
'''
_result = []


def _child():
    """The result of the one child of _CHILD (run once per session).  A child that died (signal, abort, GPU fault, time limit) fails its
    test and every later one without another process being started."""
    import json
    import os
    import subprocess
    import sys
    import time

    if _result:
        assert not isinstance(_result[0], str), f"the child failed before and is not started again: {_result[0]}"
        return _result[0]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = _CHILD % dict(root=root, tests=os.path.join(root, "tests"))
    _result.append("did not finish")
    t0 = time.time()
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    if r.returncode != 0 or "illegal memory access" in r.stderr:
        _result[0] = f"exit {r.returncode}: {r.stderr[-2000:]}"
    assert r.returncode == 0 and "illegal memory access" not in r.stderr, (r.returncode, r.stdout[-2000:] + r.stderr[-2000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("ROWS ")]
    assert lines, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(lines[0][5:])
    print(f"morph child: {time.time() - t0:.1f} s in all, {res['seconds']:.1f} s for {len(res['rows'])} calls of the entry")
    _result[0] = res
    return res


def _exact(rows):
    """every call ran the predicted kernel and wrote the reference, bytes of 0 / 255 only, and nothing else"""
    assert rows
    bad = [x for x in rows if x["status"] != 0 or x["kernel_run"] != x["expect"] or any(x["diff"]) or x["not01"] or x["guard"]]
    assert not bad, (len(bad), len(rows), bad[:5])


def _family(prefix, **kw):
    rows = [x for x in _child()["rows"] if x["case"].startswith(prefix) and all(x[k] == v for k, v in kw.items())]
    return rows


pytestmark = pytest.mark.gpu


def test_every_call_of_the_matrix_came_back(prl, cuda_device):
    """one row per batch of every case, in the order of the case list"""
    rows = _child()["rows"]
    want = [(c["name"], b) for c in cases() for b in range(len(batches(case_pages(c))))]
    assert [(x["case"], x["batch"]) for x in rows] == want


@pytest.mark.parametrize("form", [0, 1])
def test_bits_kernel_widths(prl, cuda_device, form):
    """all 8 instantiations of a source form at the 17 widths around chunks, the chunk 63 | 64 join and the strip seams, with gap
    pairs and bars at every split around each of them"""
    rows = _family("bits/w", form=form)
    assert {(x["w"], x["n"]) for x in rows} == {(w, s * m) for w in BITS_WIDTHS for m in range(1, 5) for s in (1, -1)}
    assert {x["expect"] for x in rows} == {1 + form}
    _exact(rows)


@pytest.mark.parametrize("form", [0, 1])
def test_bits_kernel_heights_and_segments(prl, cuda_device, form):
    """heights around the radius, the row block of 4 and the segment heights 8 and 64, at rows_per_seg 0 (= 8 here), 8 and 64"""
    rows = _family("bits/h", form=form)
    want = {(_height(hh, m), rps, s * m) for hh in HEIGHTS for rps in (0, 8, 64) for m in range(1, 5) for s in (1, -1)}
    assert {(x["h"], x["rps"], x["n"]) for x in rows} == want
    _exact(rows)


@pytest.mark.parametrize("form", [0, 1])
def test_bits_kernel_destination_alignment(prl, cuda_device, form):
    """A = 0..15 with a row step that keeps it (fixed_a), and row steps of width and width + 1 that change it every row (classify per
    row); the strip seam as the destination sees it, 2000 - A, is one of the boundary columns"""
    rows = _family("bits/align", form=form)
    for n in (1, -1, 4, -4):
        for w in ALIGN_WIDTHS:
            assert {x["a"] for x in rows if x["n"] == n and x["w"] == w and x["dst"] == "a"} == set(range(16)), (n, w)
            assert {x["dst"] for x in rows if x["n"] == n and x["w"] == w} == {"a", "w", "w+1"}, (n, w)
    for n in (2, -2, 3, -3):
        assert {x["a"] for x in rows if x["n"] == n and x["w"] == 2033 and x["dst"] == "a"} == set(range(16)), n
    _exact(rows)


@pytest.mark.parametrize("form", [0, 1])
def test_bits_kernel_ignores_source_padding(prl, cuda_device, form):
    """bits beyond the width in the last 16-bit word and bytes up to the row step (bit source), bytes between the width and the next
    multiple of 16 (byte source): all ones and all zeros give the same bytes"""
    rows = _family("bits/pad", form=form)
    _exact(rows)
    by = {}
    for x in rows:
        by.setdefault((x["w"], x["n"], x["batch"]), {})[x["case"].split("/fill")[1].split("/")[0]] = x["crc"]
    assert len(by) >= 3 * 8
    for k, v in by.items():
        assert set(v) == {"0", "255"} and v["0"] == v["255"], (k, v)


def test_pack_mask(prl, cuda_device):
    """k_pack_mask writes np.packbits(bitorder="little") of bit 0 of every byte, and nothing beyond the last byte of a row"""
    packs = _child()["packs"]
    assert {(x["w"], tuple(x["values"])) for x in packs} == {(w, v) for w in PACK_WIDTHS for v in ((0, 255), (0, 1, 254, 255))}
    for x in packs:
        assert x["status"] == 0 and x["diff"] == 0 and x["guard"] == 0, x


def test_stream_kernel(prl, cuda_device):
    """k_morph_stream at radius 1..8, both directions: widths around its dwords and its strips of 240 / 224 pixels, heights around its
    segments at rows_per_seg 0 (= 32 here), 32 and 128, destinations on the dword-store and on the byte-store path"""
    rows = _family("stream/")
    ns = {s * m for m in range(1, 9) for s in (1, -1)}
    assert {(x["w"], x["n"]) for x in rows if x["case"].startswith("stream/w")} == {(w, n) for w in STREAM_WIDTHS for n in ns}
    assert {(x["h"], x["rps"], x["n"]) for x in rows if x["case"].startswith("stream/h")} == \
        {(_height(hh, abs(n)), rps, n) for hh in HEIGHTS for rps in (0, 32, 128) for n in ns}
    for n in ns:
        assert {x["dst"] for x in rows if x["n"] == n} >= {"a4", "base+1", "odd"}
    assert {x["n"] for x in rows if x["tag"] == "a16"} == {n for n in ns if abs(n) > 4}     # the binarizers' own way in
    assert {x["expect"] for x in rows} == {3}
    _exact(rows)


def test_binary_kernel(prl, cuda_device):
    """k_morph_binary at radius 1..8, both directions, from a source at base + 1 and from one with an odd row step: widths and heights
    around its tile (btw x 32) for radius 1, 2, 3 and 8, destinations aligned and not"""
    rows = _family("binary/")
    for m in (1, 2, 3, 8):
        btw = binary_btw(m)
        for n in (m, -m):
            assert {(x["w"], x["h"]) for x in rows if x["n"] == n} == \
                {(w, h) for w in (btw - 1, btw, btw + 1, 2 * btw + 1) for h in (31, 32, 33, 65)}
    assert {(x["n"], x["tag"]) for x in rows} == {(s * m, t) for m in range(1, 9) for s in (1, -1) for t in ("base+1", "oddstep")}
    assert {x["dst"] for x in rows} == {"a4", "base+1", "odd"}
    assert {x["expect"] for x in rows} == {4}
    _exact(rows)


def test_guard_bytes_and_batches(prl, cuda_device):
    """no call changed a byte outside its pages (a guard row above and below every page, guard columns up to the row step, the gap
    between pages); calls of three pages hold three different pages, each compared on its own"""
    rows = _child()["rows"]
    assert all(x["guard"] == 0 for x in rows)
    three = [x for x in rows if len(x["pages"]) == 3]
    assert len(three) >= len(rows) // 3
    for x in three:     # (on a page of a few pixels two patterns can coincide)
        assert x["distinct"] == 3 or x["w"] * x["h"] < 256 or not x["pages"][0].startswith("gap"), x
    for kernel in (1, 2, 3, 4):
        assert sum(x["distinct"] == 3 for x in three if x["kernel_run"] == kernel) >= 100, kernel
    assert all(len(x["diff"]) == len(x["pages"]) for x in rows)


def test_coverage_is_the_full_matrix(prl, cuda_device):
    """From what the entry reported (not from what the case list intended): the set of (kernel, radius, direction, source) that ran is
    the full one - k_morph_bits 4 x 2 x {byte, bit} = 16, k_morph_stream 8 x 2 = 16 from a 4-byte aligned source, k_morph_binary
    8 x 2 from a source at base + 1 and 8 x 2 from one with an odd row step.  A change of the dispatch rule moves cases and fails
    here."""
    ran = {(x["kernel_run"], abs(x["n"]), x["n"] > 0, "bits" if x["form"] else
            {"a16": "bytes16", "a16wide": "bytes16", "pad": "bytes16", "a4": "bytes4", "a4row": "bytes4"}.get(x["tag"], x["tag"]))
           for x in _child()["rows"] if x["status"] == 0 and not (x["tag"] == "a16" and x["kernel_run"] == 3)}
    want = {(1, m, d, "bytes16") for m in range(1, 5) for d in (True, False)} | \
           {(2, m, d, "bits") for m in range(1, 5) for d in (True, False)} | \
           {(3, m, d, "bytes4") for m in range(1, 9) for d in (True, False)} | \
           {(4, m, d, s) for m in range(1, 9) for d in (True, False) for s in ("base+1", "oddstep")}
    assert len(want) == 64
    print("\n".join(f"{KERNEL_NAMES[k]:28s} radius {m} {'closing' if d else 'opening'} from {s}" for k, m, d, s in sorted(ran)))
    assert ran == want, sorted(ran ^ want)


def test_argument_errors(prl, cuda_device):
    """radius 0 or above 8, a bit plane with an odd step, with a step below ceil16(width) / 8 or with a radius above 4:
    PRL_ERR_BAD_ARG, no kernel reported, the destination untouched"""
    from prlib_amd import _capi

    errs = _child()["errs"]
    assert [e["name"] for e in errs] == [c[0] for c in bad_arg_calls()]
    for e in errs:
        assert e["status"] == _capi.PRL_ERR_BAD_ARG and e["kernel_run"] == 0 and e["touched"] == 0, e


@pytest.mark.parametrize("h", [31, 32, 33])
@pytest.mark.parametrize("w", [63, 64, 65, 129])
def test_public_morph_on_pattern_pages(prl, cuda_device, w, h):
    """prl.morph (k_morph for radius <= 8, chained k_rect passes above) on 0 / 255 gray images that carry information: gap pairs around
    its 64 x 32 tile and the random page of the radius (uniform random gray is >= 250 almost everywhere after a 17 x 17 maximum)"""
    import torch

    for n in [s * m for m in (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 17) for s in (1, -1)]:
        pages = [(name, p) for name, p in mr.pages_for(n, h, w, [64, 128], [32], seed=300 + abs(n), max_phases=2)
                 if name.startswith(("gap", "random"))]
        src = np.stack([mr.to_bytes(p) for _, p in pages])
        got = prl.morph(torch.from_numpy(src).to(cuda_device), n).cpu().numpy()
        for k, (name, p) in enumerate(pages):
            assert np.array_equal(got[k], mr.to_bytes(mr.close_open(p, n))), (n, name)
