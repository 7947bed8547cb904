"""prl::binarizeLocalOtsu and what it is built on, restated in numpy / plain Python from the canonical forms of include/prl_hip.h
("the 8-bit cv::GaussianBlur", "binarizeLocalOtsu") - independent of the C++ in prlib_amd/csrc.  Everything is integer, or a fixed
float64 sequence: the tests compare for equality.

    kernel_u8 / blur_u8 / sep_filter_u8   the 8-bit cv::GaussianBlur: 8.8 weights by error diffusion, the separable integer filter
    external_rects                        cv::findContours(RETR_EXTERNAL)'s raster scan and border following; the bounding
                                          rectangles of the contours of at least 3 points
    otsu_threshold / rect_otsu            getThreshVal_Otsu_8u of a rectangle's histogram; the per-rectangle threshold and paint
"""
import math

import numpy as np

MAX_SIDE = 255
TABLES = {1: [1.0], 3: [0.25, 0.5, 0.25], 5: [0.0625, 0.25, 0.375, 0.25, 0.0625],
          7: [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]}


# ---- the 8-bit cv::GaussianBlur -----------------------------------------------------------------------------------------------------

def kernel_f64(n, sigma=0.0):
    if sigma <= 0 and n in TABLES:
        return list(TABLES[n])
    s = sigma if sigma > 0 else ((n - 1) * 0.5 - 1) * 0.3 + 0.8
    k = [math.exp(-0.5 / (s * s) * (i - (n - 1) * 0.5) ** 2) for i in range(n)]
    total = 0.0
    for v in k:
        total += v
    return [v / total for v in k]


def kernel_u8(n, sigma=0.0, with_margin=False):
    """the n 8.8 weights of a side (a list of ints that sums to 256); with_margin: also the smallest distance of an adj from a tie"""
    k = kernel_f64(n, sigma)
    w, err, margin = [0] * n, 0.0, 0.5
    for i in range(n // 2):
        adj = k[i] * 256 + err
        v = round(adj)   # Python rounds ties to even, as cvRound does
        err = adj - v
        margin = min(margin, abs(adj - math.floor(adj) - 0.5))
        w[i] = w[n - 1 - i] = v
    w[n // 2] = 256 - sum(w)
    return (w, margin) if with_margin else w


def reflect101(p, n):
    """cv::borderInterpolate(p, n, BORDER_REFLECT_101), with its loop"""
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * n - 2 - p
    return p


def sep_filter_u8(page, wx, wy):
    """H x W [x C] uint8 -> the same shape: h = sum_i wx[i] p(R(x + i - rx)), dst = (sum_j wy[j] h(R(y + j - ry)) + 32768) >> 16"""
    img = page if page.ndim == 3 else page[:, :, None]
    H, W, _ = img.shape
    rx, ry = len(wx) // 2, len(wy) // 2
    src = img.astype(np.int64)
    h = np.zeros_like(src)
    for i, wt in enumerate(wx):
        cols = [reflect101(x + i - rx, W) for x in range(W)]
        h += int(wt) * src[:, cols]
    assert h.max() <= 0xFFFF
    acc = np.full_like(src, 32768)
    for j, wt in enumerate(wy):
        rows = [reflect101(y + j - ry, H) for y in range(H)]
        acc += int(wt) * h[rows]
    assert acc.max() < 1 << 32
    return (acc >> 16).astype(np.uint8).reshape(page.shape)


def blur_u8(page, ksize, sigma_x=0.0, sigma_y=0.0):
    """cv::GaussianBlur(page, ksize = (width, height), sigma_x, sigma_y) on 8-bit pages"""
    if sigma_y <= 0:
        sigma_y = sigma_x
    return sep_filter_u8(page, kernel_u8(ksize[0], sigma_x), kernel_u8(ksize[1], sigma_y))


def blur_u8_direct(page, ksize, sigma_x=0.0, sigma_y=0.0):
    """the same as one double sum per pixel (gray pages; the self-check of the separable form)"""
    if sigma_y <= 0:
        sigma_y = sigma_x
    wx, wy = kernel_u8(ksize[0], sigma_x), kernel_u8(ksize[1], sigma_y)
    H, W = page.shape
    out = np.zeros_like(page)
    for y in range(H):
        for x in range(W):
            a = 32768
            for j, wj in enumerate(wy):
                for i, wi in enumerate(wx):
                    a += wj * wi * int(page[reflect101(y + j - len(wy) // 2, H), reflect101(x + i - len(wx) // 2, W)])
            out[y, x] = a >> 16
    return out


def noise(h, w, c, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=(h, w, c) if c > 1 else (h, w), dtype=np.uint8)


# ---- the external bounding rectangles ------------------------------------------------------------------------------------------------

def external_contours(edge_map):
    """cv::findContours(map, RETR_EXTERNAL, CHAIN_APPROX_SIMPLE): the point lists in discovery order - OpenCV's retrieval mode 0, the
    raster scan restated literally; borders are followed by contour_ref._trace."""
    import contour_ref as cr

    page = np.asarray(edge_map)
    h, w = page.shape
    img = np.zeros((h + 2, w + 2), np.int8)
    img[1:-1, 1:-1] = page != 0
    out = []
    for y in range(1, h + 1):
        row = img[y]
        prev, lnbd = 0, 0
        for x in range(1, w + 1):
            p = int(row[x])
            if p == prev:
                continue
            start = False
            if prev == 0 and p == 1:
                start = not int(row[lnbd]) > 0
            elif not (p != 0 or prev < 1):
                if prev & -2:          # a hole start: never traced in this mode
                    lnbd = x - 1
            if start:
                out.append(cr._trace(img, x, y, False))
                p = int(row[x])
            prev = p
            if prev & -2:
                lnbd = x
    return out


def rects_of_contours(contours):
    rects = []
    for pts in contours:
        if len(pts) < 3:
            continue
        xs, ys = [p[0] for p in pts], [p[1] for p in pts]
        rects.append((min(xs), min(ys), max(xs) - min(xs) + 1, max(ys) - min(ys) + 1))
    return rects


def external_rects(edge_map):
    """([(x, y, w, h)] of the contours of at least 3 points, the number of contours found)"""
    contours = external_contours(edge_map)
    return rects_of_contours(contours), len(contours)


def component_rects(edge_map):
    """NOT what OpenCV's mode 0 gives: the outer border of EVERY 8-connected component (the non-hole contours of RETR_CCOMP), for
    the test that tells the two apart"""
    import contour_ref as cr

    contours = [pts for pts, hole in cr.find_contours(edge_map) if not hole]
    return rects_of_contours(contours), len(contours)


# ---- the per-rectangle Otsu --------------------------------------------------------------------------------------------------------

FLT_EPSILON = float(np.finfo(np.float32).eps)


def otsu_threshold(hist, pixels):
    """getThreshVal_Otsu_8u on 256 bins of `pixels` pixels: plain float64, in the order OpenCV writes it"""
    scale = 1.0 / float(pixels)
    mu = 0.0
    for i in range(256):
        mu += i * float(hist[i])
    mu *= scale
    mu1 = q1 = max_sigma = 0.0
    max_val = 0
    for i in range(256):
        p_i = float(hist[i]) * scale
        mu1 *= q1
        q1 += p_i
        q2 = 1.0 - q1
        if min(q1, q2) < FLT_EPSILON or max(q1, q2) > 1.0 - FLT_EPSILON:
            continue
        mu1 = (mu1 + i * p_i) / q1
        mu2 = (mu - q1 * mu1) / q2
        sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2)
        if sigma > max_sigma:
            max_sigma, max_val = sigma, i
    return max_val


def otsu_of(plane):
    return otsu_threshold(np.bincount(plane.ravel(), minlength=256), plane.size)


def cv_round(v):
    return int(round(v))   # ties to even


def rect_otsu(gray, rects, max_value=255.0):
    """(the mask, [thr per rectangle]): 255, and 0 inside every rectangle where (p > thr ? imax : 0) ^ 255 != 0"""
    imax = min(max(cv_round(max_value), 0), 255)
    mask = np.full(gray.shape, 255, np.uint8)
    thrs = []
    for (x, y, w, h) in rects:
        roi = gray[y:y + h, x:x + w]
        thr = otsu_of(roi)
        thrs.append(thr)
        v = np.where(roi > thr, imax, 0)
        mask[y:y + h, x:x + w][(v ^ 255) != 0] = 0
    return mask, thrs


# ---- CannyEdgeDetection and the whole call ----------------------------------------------------------------------------------------------

def morph_iterations(plane, iterations):
    """cv::dilate / cv::erode with the 3 x 3 rectangle, |iterations| times each: closing (> 0) or opening (< 0)"""
    import nuil_ref as nr

    n = abs(iterations)
    ops = (nr.dilate, nr.erode) if iterations > 0 else (nr.erode, nr.dilate)
    for op in ops:
        for _ in range(n):
            plane = op(plane, nr.RECT, 3, 3)
    return plane


def canny_pair(t, upper_coeff, lower_coeff):
    """cv::Canny's integer (low, high) for a plane whose Otsu value is t"""
    import edges_ref as er

    upper = upper_coeff * float(t)
    lower = lower_coeff * upper
    return er.canny_thresholds(lower, upper)


def canny_edge_detection(page, size=19, upper_coeff=0.15, lower_coeff=0.01, iterations=1, with_t=False):
    """imageLibCommon.cpp:244-324 on H x W [x C]: the H x W map; with_t: and the Otsu value of every channel"""
    import edges_ref as er

    img = page if page.ndim == 3 else page[:, :, None]
    result = np.zeros(img.shape[:2], np.uint8)
    ts = []
    for c in range(img.shape[2]):
        plane = blur_u8(np.ascontiguousarray(img[:, :, c]), (size, size), 0.0)
        t = otsu_of(plane)
        ts.append(t)
        upper = upper_coeff * float(t)
        lower = lower_coeff * upper
        edges = er.canny(plane, lower, upper)
        if iterations:
            edges = morph_iterations(edges, iterations)
        result |= edges
    return (result, ts) if with_t else result


def rgb2gray(page):
    """cv::cvtColor(COLOR_RGB2GRAY) of H x W x 3 or 4"""
    p = page.astype(np.int64)
    return ((4899 * p[:, :, 0] + 9617 * p[:, :, 1] + 1868 * p[:, :, 2] + 8192) >> 14).astype(np.uint8)


def bgr2gray(page):
    p = page.astype(np.int64)
    return ((1868 * p[:, :, 0] + 9617 * p[:, :, 1] + 4899 * p[:, :, 2] + 8192) >> 14).astype(np.uint8)


def binarize_local_otsu(page, max_value=255.0, clip_limit=0.0, size=19, upper_coeff=0.15, lower_coeff=0.01, iterations=1, stages=False):
    """binarizeLocalOtsu.cpp:37-163: (mask, contours found, rectangles kept); stages: also the intermediate results"""
    import clahe_ref as cl
    import nuil_ref as nr

    gray = rgb2gray(page) if page.ndim == 3 else page
    if clip_limit > 0:
        gray = cl.enhance(gray, clip_limit, True)
    edges = canny_edge_detection(gray, size, upper_coeff, lower_coeff, iterations)
    dilated = edges
    for _ in range(3):
        dilated = nr.dilate(dilated, nr.RECT, 3, 3)
    rects, found = external_rects(dilated)
    mask, thrs = rect_otsu(gray, rects, max_value)
    if stages:
        return mask, found, len(rects), dict(gray=gray, edges=edges, dilated=dilated, rects=rects, thrs=thrs)
    return mask, found, len(rects)
