"""The pages and angles of tests/test_rotate_cpu.py (oracle.rotate against tests/rotate_ref.py) and tests/test_rotate_gpu.py (the
kernels of rotate.hip against oracle.rotate): every GPU case is a CPU case.

k_warp works in workgroups of 256 canvas columns x kWarpRows = 4 canvas rows and stores each row segment as head bytes, dwords and
tail bytes; k_rot90 turns 32 x 32 tiles.  The canvas of a general angle is max(w, h) square.
"""
import numpy as np

from prlib_amd import synth

# 0.0 is not special-cased: it goes through the warp.  90 + 2e-7 and -90 (fmod keeps the sign) are general angles too.
ANGLES = [0.0, 1e-9, 0.57, 3.0, -7.25, 45.0, 89.9999, 90 + 2e-7, -90.0, 123.456, -180.5, 359.999, 720.3]
SIDES = [1, 2, 255, 256, 257, 511, 513, 770]      # one to four 256-column workgroups, every residue modulo 4
THIN = [(1, 40), (40, 1), (1, 300), (300, 1)]      # 1 x N and N x 1 (1 x 1 is side 1)

ROT90_SHAPES = [(1, 1), (1, 70), (70, 1), (31, 33), (32, 32), (33, 64), (65, 97)]      # (h, w)
ROT90_ANGLES = [90.0, 270.0, 450.0, 90 + 5e-8]
HALF_TURN_SHAPES = [(77, 300), (300, 77)]                                              # (h, w)

KIND_ANGLES = [90 - 5e-8, 90 + 5e-8, 90 - 2e-7, 90 + 2e-7, 180 - 5e-8, 180 + 5e-8, 180 - 2e-7, 180 + 2e-7,
               270 - 5e-8, 270 + 5e-8, 270 - 2e-7, 270 + 2e-7, 450.0, -90.0, 360.0, 720.3]

VIEW_W, VIEW_H = 300, 77
VIEW_ANGLES = [2.0, 90.0, 180.0, 270.0, -33.0]     # results 300 x 300, 77 x 300, 300 x 77, 77 x 300, 300 x 300 in one grid


def page(h, w, c, seed, text=False):
    """random bytes, or a text page in channel 0 with random bytes in the others"""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    if text:
        p[:, :, 0] = synth.text_page_numpy(h, w, seed, skew_deg=1.0)
    return p[:, :, 0].copy() if c == 1 else p


def _landscape(side):
    return max(1, side // 3), side


def _portrait(side):
    return side, max(1, side // 3)


def warp_cases():
    """[(id, h, w, c, angles, seed, text)]: every side with every channel count, each side twice as landscape and twice as portrait,
    and four angles per case taken round the list, so that every angle occurs with every channel count and on a large canvas."""
    out, k = [], 0
    for i, side in enumerate(SIDES):
        for c in (1, 2, 3, 4):
            h, w = _landscape(side) if (i + c) % 2 else _portrait(side)
            angles = [ANGLES[(5 * k + j) % len(ANGLES)] for j in range(4)]
            out.append((f"{h}x{w}x{c}", h, w, c, angles, 100 + k, side in (255, 513) and min(h, w) >= 64))
            k += 1
    for h, w in THIN:
        for c in (1, 3):
            angles = [ANGLES[(5 * k + j) % len(ANGLES)] for j in range(4)]
            out.append((f"{h}x{w}x{c}", h, w, c, angles, 100 + k, False))
            k += 1
    return out


def rot90_cases():
    """[(id, h, w, c, angles, seed)]: the quarter turns of k_rot90, and the half turn (kind 2 inside k_warp)"""
    out = []
    for n, (h, w) in enumerate(ROT90_SHAPES):
        for c in (1, 2, 3, 4):
            out.append((f"{h}x{w}x{c}", h, w, c, ROT90_ANGLES, 300 + 4 * n + c))
    for n, (h, w) in enumerate(HALF_TURN_SHAPES):
        for c in (1, 2, 3, 4):
            out.append((f"half_{h}x{w}x{c}", h, w, c, [180.0], 400 + 4 * n + c))
    return out


def view_pages(c):
    """the five pages of the views-and-guards test"""
    return [page(VIEW_H, VIEW_W, c, 500 + 10 * c + i, text=(i == 0)) for i in range(len(VIEW_ANGLES))]


def host_cases():
    """prl_hip_rotate_host with two channels: a general angle and a quarter turn"""
    return [(page(60, 91, 2, 600), 12.5), (page(60, 91, 2, 601), 90.0)]


def all_cpu_cases():
    """[(id, page, angle)] - every (page, angle) the GPU tests compare with the oracle"""
    out = []
    for cid, h, w, c, angles, seed, text in warp_cases():
        p = page(h, w, c, seed, text)
        out += [(f"warp_{cid}_{a!r}", p, a) for a in angles]
    for cid, h, w, c, angles, seed in rot90_cases():
        p = page(h, w, c, seed)
        out += [(f"rot90_{cid}_{a!r}", p, a) for a in angles]
    for c in (1, 3):
        out += [(f"view_{c}_{a!r}", p, a) for p, a in zip(view_pages(c), VIEW_ANGLES)]
    out += [(f"host_{a!r}", p, a) for p, a in host_cases()]
    return out
