"""Restatements of the reference's tone functions for the tests of tone.hip (test infrastructure; numpy and the host's libm only).

    prl::gammaCorrection         src/balance/gammaCorrection.cpp:52-106
    prl::simpleWhiteBalance      src/balance/balanceSimpleWhite.cpp:33-142
    prl::grayWorldWhiteBalance   src/balance/balanceGrayWorldWhite.cpp:37-115
    prl::cleanBackgroundToWhite  src/cleanBackgroundToWhite.cpp:39-64

Three layers, held equal by tests/test_tone_cpu.py:
  *_loops    the reference's statements loop for loop in plain Python (small pages only);
  *_literal  the same per-pixel arithmetic with numpy element-wise operations of the same types (float32 / float64 products,
             comparisons, truncation) and a strictly sequential raster-order sum (np.cumsum) - no histogram shortcut;
  *_model    histogram -> 256-entry table per channel -> table[src]: what tone.hip computes.
pow is the host libm's, called through ctypes (numpy's vectorised power may differ from it in the last bit).  The choices where
the reference's behaviour is undefined are those of include/prl_hip.h.
"""
import ctypes
import ctypes.util
import math

import numpy as np

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.pow.restype = ctypes.c_double
_libm.pow.argtypes = [ctypes.c_double, ctypes.c_double]


def pow_libm(x, y):
    return _libm.pow(float(x), float(y))


F32, F64 = np.float32, np.float64


def sat_u8(t):
    """saturate_cast<uchar> of a double or a float: round half to even; NaN, +-inf and what is outside int32 -> 0"""
    t = float(t)
    if t != t or math.isinf(t):
        return 0
    r = round(t)   # half to even
    if not -2 ** 31 <= r <= 2 ** 31 - 1:
        return 0
    return min(max(r, 0), 255)


def histograms(img):
    """H x W [x C] -> C x 256 counts"""
    a = img if img.ndim == 3 else img[:, :, None]
    return np.stack([np.bincount(a[:, :, c].ravel(), minlength=256) for c in range(a.shape[2])]).astype(np.int64)


def apply_luts(img, luts):
    """luts: C x 256 (or 256 for every channel)"""
    a = img if img.ndim == 3 else img[:, :, None]
    luts = np.asarray(luts, np.uint8)
    if luts.ndim == 1:
        luts = np.broadcast_to(luts, (a.shape[2], 256))
    out = np.stack([luts[c][a[:, :, c]] for c in range(luts.shape[0])], axis=2)
    return out if img.ndim == 3 else out[:, :, 0]


# ---- gammaCorrection -----------------------------------------------------------------------------------------------------------

def eq_d(a, b, delta=1e-7):
    return abs(a - b) <= delta


def gamma_only_lut(gamma):
    return np.array([sat_u8(pow_libm(i / 255.0, gamma) * 255.0) for i in range(256)], np.uint8)


def k_step_lut(k):
    """Mat *= k on 8U = convertTo(8U, k): sat_u8((float)v * (float)k) [upstream]; the identity when eq_d(k, 1.0)"""
    if eq_d(k, 1.0):
        return np.arange(256, dtype=np.uint8)
    with np.errstate(all="ignore"):
        return np.array([sat_u8(F32(v) * F32(k)) for v in range(256)], np.uint8)


def gamma_lut(k, gamma):
    """both steps composed: what prl_hip_gamma_lut returns"""
    return k_step_lut(k)[gamma_only_lut(gamma)]


def gamma_out_channels(c):
    return 3 if c == 4 else c


def gamma_literal(img, k, gamma):
    a = img if img.ndim == 3 else img[:, :, None]
    c = a.shape[2]
    lut = gamma_only_lut(gamma)
    out = a.copy()
    if c == 4:
        out = out[:, :, :3].copy()   # cvtColor(BGRA2BGR); the switch below has no case for 4
    if c in (1, 2, 3):
        out = lut[out]
    if not eq_d(k, 1.0):
        with np.errstate(all="ignore"):
            prod = out.astype(F32) * F32(k)
        flat = prod.ravel()
        uniq, inv = np.unique(flat.view(np.uint32), return_inverse=True)
        res = np.array([sat_u8(x) for x in uniq.view(F32)], np.uint8)   # sat_u8 per distinct product (a pure function of it)
        out = res[inv].reshape(out.shape)
    return out if img.ndim == 3 else out[:, :, 0]


def gamma_loops(img, k, gamma):
    a = img if img.ndim == 3 else img[:, :, None]
    h, w, c = a.shape
    lut = [sat_u8(pow_libm(i / 255.0, gamma) * 255.0) for i in range(256)]
    oc = gamma_out_channels(c)
    out = np.zeros((h, w, oc), np.uint8)
    for y in range(h):
        for x in range(w):
            for j in range(oc):
                v = int(a[y, x, j])
                if c in (1, 2, 3):
                    v = lut[v]
                if not eq_d(k, 1.0):
                    with np.errstate(all="ignore"):
                        v = sat_u8(F32(v) * F32(k))
                out[y, x, j] = v
    return out if img.ndim == 3 else out[:, :, 0]


def gamma_model(img, k, gamma):
    a = img if img.ndim == 3 else img[:, :, None]
    lut = k_step_lut(k) if a.shape[2] == 4 else gamma_lut(k, gamma)
    out = apply_luts(a[:, :, :gamma_out_channels(a.shape[2])], lut)
    return out if img.ndim == 3 else out[:, :, 0]


# ---- simpleWhiteBalance --------------------------------------------------------------------------------------------------------

def swb_range(k, hist, total):
    """cumulative histogram as int; both scans stop at the array's ends (the reference reads outside it there)"""
    cum = [0] * 256
    acc = 0
    for j in range(256):
        acc += int(hist[j])
        cum[j] = acc
    vmin, vmax = 0, 255
    while vmin < 255 and cum[vmin] < k * total:
        vmin += 1
    while vmax > 0 and cum[vmax] > (1 - k) * total:
        vmax -= 1
    if vmax < 255 - 1:
        vmax += 1
    return vmin, vmax


def swb_scale(vmin, vmax):
    with np.errstate(all="ignore"):
        return F32(255.0) / F32(vmax - vmin)


def swb_entry(v, vmin, vmax, scale):
    val = v
    if val < vmin:
        val = vmin
    if val > vmax:
        val = vmax
    with np.errstate(all="ignore"):
        f = F32(val - vmin) * scale
    if f != f:
        return 0   # 0 * inf: the x86 conversion's 0x80000000, low byte 0
    return int(f) & 0xFF


def swb_luts(k, hist, total=None):
    hist = np.asarray(hist).reshape(3, 256)
    total = int(hist[0].sum()) if total is None else total
    luts = np.zeros((3, 256), np.uint8)
    for c in range(3):
        vmin, vmax = swb_range(k, hist[c], total)
        scale = swb_scale(vmin, vmax)
        luts[c] = [swb_entry(v, vmin, vmax, scale) for v in range(256)]
    return luts


def _need3(img):
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("3 channels only")
    if img.size == 0:
        raise ValueError("empty")


def swb_literal(img, k):
    _need3(img)
    total = img.shape[0] * img.shape[1]
    hist = histograms(img)
    out = np.empty_like(img)
    for c in range(3):
        vmin, vmax = swb_range(k, hist[c], total)
        scale = swb_scale(vmin, vmax)
        val = img[:, :, c].astype(np.int32)
        val = np.where(val < vmin, vmin, val)
        val = np.where(val > vmax, vmax, val)
        with np.errstate(all="ignore"):
            f = (val - vmin).astype(F32) * scale
            out[:, :, c] = np.where(np.isnan(f), 0, f.astype(np.int64) & 0xFF).astype(np.uint8)
    return out


def swb_loops(img, k):
    _need3(img)
    h, w, _ = img.shape
    hists = [[0] * 256 for _ in range(3)]
    for y in range(h):
        for x in range(w):
            for j in range(3):
                hists[j][int(img[y, x, j])] += 1
    total = w * h
    rng = [swb_range(k, hists[j], total) for j in range(3)]
    scale = [swb_scale(*rng[j]) for j in range(3)]
    out = np.empty_like(img)
    for y in range(h):
        for x in range(w):
            for j in range(3):
                out[y, x, j] = swb_entry(int(img[y, x, j]), rng[j][0], rng[j][1], scale[j])
    return out


def swb_model(img, k):
    _need3(img)
    return apply_luts(img, swb_luts(k, histograms(img), img.shape[0] * img.shape[1]))


# ---- grayWorldWhiteBalance -----------------------------------------------------------------------------------------------------

def gw_ratios(m, with_max):
    """m = (ml, ma, mb) = the means of channels 0, 1, 2 as float64"""
    ml, ma, mb = (F64(x) for x in m)
    with np.errstate(all="ignore"):
        r = (ma + mb + ml) / F64(3.0)
        if with_max:
            inner = ml if mb < ml else mb      # std::max(mb, ml)
            r = inner if ma < inner else ma    # std::max(ma, ...)
        return [r / ml, r / ma, r / mb]


def gw_entry(v, ratio):
    with np.errstate(all="ignore"):
        l = F64(v) * ratio
    l = l if l < 255.0 else F64(255.0)   # std::min(255.0, l): a NaN gives 255
    return int(l)


def gw_means_hist(p, hist, total):
    """the canonical sum: ascending bins, (double)hist[v] * pow(v, p), empty bins add nothing; p == 1 skips pow"""
    m = []
    for c in range(3):
        s = 0.0
        for v in range(256):
            if hist[c][v]:
                s += float(hist[c][v]) * (float(v) if p == 1.0 else pow_libm(v, p))
        with np.errstate(all="ignore"):
            m.append(F64(s) / F64(total) if p == 1.0 else F64(pow_libm(F64(s) / F64(total), F64(1.0) / F64(p))))
    return m


def gw_means_raster(img, p):
    """getAverageValues: three accumulators, each summed in raster order (np.cumsum adds strictly one after the other)"""
    total = img.shape[0] * img.shape[1]
    pw = np.array([pow_libm(v, p) for v in range(256)], F64)
    m = []
    for c in range(3):
        s = np.cumsum(pw[img[:, :, c].ravel()])[-1]
        with np.errstate(all="ignore"):
            m.append(F64(pow_libm(F64(s) / F64(total), F64(1.0) / F64(p))))
    return m


def gw_luts(p, with_max, hist, total=None):
    hist = np.asarray(hist).reshape(3, 256)
    total = int(hist[0].sum()) if total is None else total
    ratio = gw_ratios(gw_means_hist(p, hist, total), with_max)
    return np.array([[gw_entry(v, ratio[c]) for v in range(256)] for c in range(3)], np.uint8)


def gw_literal(img, p, with_max):
    _need3(img)
    ratio = gw_ratios(gw_means_raster(img, p), with_max)
    out = np.empty_like(img)
    for c in range(3):
        with np.errstate(all="ignore"):
            l = img[:, :, c].astype(F64) * ratio[c]
            l = np.where(l < 255.0, l, 255.0)
        out[:, :, c] = l.astype(np.int64).astype(np.uint8)
    return out


def gw_loops(img, p, with_max):
    _need3(img)
    h, w, _ = img.shape
    ml = ma = mb = 0.0
    for i in range(h):
        for j in range(w):
            lc, ac, bc = (pow_libm(int(img[i, j, c]), p) for c in range(3))
            ma += ac
            mb += bc
            ml += lc
    with np.errstate(all="ignore"):
        m = [F64(pow_libm(F64(s) / F64(w * h), F64(1.0) / F64(p))) for s in (ml, ma, mb)]
    ratio = gw_ratios(m, with_max)
    out = np.empty_like(img)
    for i in range(h):
        for j in range(w):
            for c in range(3):
                out[i, j, c] = gw_entry(int(img[i, j, c]), ratio[c])
    return out


def gw_model(img, p, with_max):
    _need3(img)
    return apply_luts(img, gw_luts(p, with_max, histograms(img), img.shape[0] * img.shape[1]))


# ---- cleanBackgroundToWhite ----------------------------------------------------------------------------------------------------

# numaGammaTRC(1.0, 70, 170) [upstream], its 256 values written out (x is a float32: 0.7f and 0.9f lie below 0.7 and 0.9, so
# t[140] = 178 and t[160] = 229, not 179 and 230)
CLEAN_LUT = np.array(
    [0] * 70
    + [0, 3, 5, 8, 10, 13, 15, 18, 20, 23, 26, 28, 31, 33, 36, 38, 41, 43, 46, 48, 51, 54, 56, 59, 61, 64, 66, 69, 71, 74, 77, 79, 82,
       84, 87, 89, 92, 94, 97, 99, 102, 105, 107, 110, 112, 115, 117, 120, 122, 125, 128, 130, 133, 135, 138, 140, 143, 145, 148, 150,
       153, 156, 158, 161, 163, 166, 168, 171, 173, 176, 178, 181, 184, 186, 189, 191, 194, 196, 199, 201, 204, 207, 209, 212, 214, 217,
       219, 222, 224, 227, 229, 232, 235, 237, 240, 242, 245, 247, 250, 252, 255]
    + [255] * 85, np.uint8)


def clean_lut():
    """numaGammaTRC(1.0, 70, 170) computed: x in float32, the product and the add in double, powf(x, 1) taken as x"""
    t = []
    for i in range(256):
        if i < 70:
            t.append(0)
        elif i > 170:
            t.append(255)
        else:
            x = F32(i - 70) / F32(100)
            t.append(min(max(int(255.0 * float(x) + 0.5), 0), 255))
    return np.array(t, np.uint8)


def clean_background(oracle, img):
    """pixBackgroundNormSimple (the oracle's restatement) followed by pixGammaTRC(1.0, 70, 170)"""
    return CLEAN_LUT[oracle.bgnorm(img)]


# ---- inputs ----------------------------------------------------------------------------------------------------------------------

def noise_page(w, h, c, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, c), dtype=np.uint8)


def paper_page(w, h, seed, tint=(228, 236, 243)):
    """tinted paper with a vignette, sensor noise and dark text-like strokes: 3 channels"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    shade = 1.0 - 0.25 * (((xx - w / 2) / max(w, 1)) ** 2 + ((yy - h / 2) / max(h, 1)) ** 2)
    img = np.stack([shade * t for t in tint], axis=2) + rng.normal(0, 3, size=(h, w, 3))
    ink = (rng.random((h, w)) < 0.08) & ((yy // 6) % 3 == 0)
    img[ink] = img[ink] * 0.2 + rng.normal(0, 4, size=(int(ink.sum()), 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def gray3_page(w, h, seed):
    g = paper_page(w, h, seed)[:, :, 1]
    return np.stack([g, g, g], axis=2)


def ramp_page(w, h, c):
    """every value in every channel where w * h >= 256 (each channel starts elsewhere)"""
    i = np.arange(w * h, dtype=np.int64).reshape(h, w)
    return np.stack([((i + 37 * ch) % 256) for ch in range(c)], axis=2).astype(np.uint8)


def checker_page(w, h, c, a=17, b=200):
    i = np.add.outer(np.arange(h), np.arange(w)) % 2
    return np.stack([np.where(i == 0, a + ch, b - ch) for ch in range(c)], axis=2).astype(np.uint8)


def flat_page(w, h, values):
    return np.broadcast_to(np.array(values, np.uint8), (h, w, len(values))).copy()


def colour_families(w, h, seed=1):
    """3-channel pages for the four functions, the degenerate ones included"""
    two = checker_page(w, h, 3, 40, 215)
    zero_ch = noise_page(w, h, 3, seed + 5)
    zero_ch[:, :, 1] = 0
    return [("noise", noise_page(w, h, 3, seed)), ("paper", paper_page(w, h, seed + 1)), ("gray3", gray3_page(w, h, seed + 2)),
            ("ramp", ramp_page(w, h, 3)), ("two_valued", two), ("zero_channel", zero_ch), ("flat255", flat_page(w, h, (255,) * 3)),
            ("flat100", flat_page(w, h, (100,) * 3)), ("flat_each", flat_page(w, h, (0, 100, 255)))]


def hist_families(w, h, c, seed=1):
    """pages for the histogram kernel: what its wavefront-uniform shortcut could get wrong"""
    per = tuple((60 + 70 * ch) % 256 for ch in range(c))
    last = flat_page(w, h, per)
    last[h - 1, w - 1] = [(v + 101) % 256 for v in per]          # one odd pixel in the last column of the last row
    mid = flat_page(w, h, per)
    mid[h // 2, 0] = [(v + 55) % 256 for v in per]                # one in lane 0 of a middle row
    return [("flat0", flat_page(w, h, (0,) * c)), ("flat255", flat_page(w, h, (255,) * c)), ("flat_each", flat_page(w, h, per)),
            ("odd_last", last), ("odd_lane0", mid), ("checker", checker_page(w, h, c)), ("ramp", ramp_page(w, h, c)),
            ("noise", noise_page(w, h, c, seed))]


def emulate_hist(img):
    """k_tone_hist's accounting in numpy: a lane takes 4 pixels of a row, 64 lanes a wavefront (256 pixels from a multiple of 256);
    per channel a wavefront whose lanes all hold four equal pixels of lane 0's value adds 256 once, a lane with four equal pixels
    adds 4, every other lane its n <= 4 pixels one by one"""
    a = img if img.ndim == 3 else img[:, :, None]
    h, w, c = a.shape
    wp = (w + 255) // 256 * 256
    hist = np.zeros((c, 256), np.int64)
    for ch in range(c):
        row = np.full((h, wp), -1, np.int64)
        row[:, :w] = a[:, :, ch]
        px = row.reshape(h, wp // 256, 64, 4)
        n = (px >= 0).sum(axis=3)
        first = np.where(n > 0, px[..., 0], 0)
        flat = (n == 4) & (px == px[..., :1]).all(axis=3)
        uniform = (flat & (first == first[..., :1])).all(axis=2)
        np.add.at(hist[ch], first[..., 0][uniform], 256)
        lanes = flat & ~uniform[..., None]
        np.add.at(hist[ch], first[lanes], 4)
        rest = px[~flat & ~uniform[..., None]]
        np.add.at(hist[ch], rest[rest >= 0], 1)
    return hist


HIST_SIZES = [(1, 1), (3, 1), (5, 7), (64, 1), (257, 3), (1031, 517), (4100, 2)]
SWB_KS = [0.0, 0.01, 0.25, 0.5, -1.0, float("nan")]
GAMMAS = [0.4, 1.0, 2.2]
GAMMA_KS = [1.0, 1.0 + 5e-8, 0.5, 1.7]
GW_PS = [1.0, 2.0, 3.0, 6.0, 0.5, 2.5]
