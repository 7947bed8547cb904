"""prl::binarizeLocalOtsu and what it is built on over the C ABI: the 8-bit cv::GaussianBlur (blur8.hip), CannyEdgeDetection
(edgedet.hip), the external bounding rectangles (contour.h, host code) and the per-rectangle Otsu (localotsu.hip).  The rules are
stated in include/prl_hip.h.

    void prl::binarizeLocalOtsu(cv::Mat&, cv::Mat&, double maxValue = 255.0, double CLAHEClipLimit = 0.0,
                                int GaussianBlurKernelSize = 19, double CannyUpperThresholdCoeff = 0.15,
                                double CannyLowerThresholdCoeff = 0.01, int CannyMorphIters = 1)   (binarizeLocalOtsu.h)

numpy H x W [x C] uint8 goes through the library's host entry; torch CUDA uint8 [N,] H x W [x C] is enqueued on the current stream
(the rule of _pages.py).  Errors are PrlError with the C status.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _capi, _pages

MAX_SIDE = 255
RECT_OTSU_SMALL_AREA = 4096   # PRL_RECT_OTSU_SMALL_AREA: a rectangle of at most this many pixels is one wavefront's


def gaussianKernelU8(n, sigma=0.0):
    """the n 8.8 fixed-point weights the 8-bit cv::GaussianBlur filters a side of n with: uint16 [n], on the host (no device)"""
    w = np.empty(max(int(n), 0), np.uint16)
    _capi.check(_capi.lib().prl_hip_gaussian_kernel_u8(int(n), float(sigma), w.ctypes.data))
    return w


def gaussianBlurU8(pages, ksize, sigmaX=0.0, sigmaY=0.0, out=None):
    """cv::GaussianBlur(pages, ksize = (width, height), sigmaX, sigmaY) on 8-bit pages of 1 to 4 channels, BORDER_REFLECT_101"""
    L = _capi.lib()
    kw, kh, sx, sy = int(ksize[0]), int(ksize[1]), float(sigmaX), float(sigmaY)
    return _pages.run(pages, _pages.same,
                      lambda c, *a: L.prl_hip_gaussian_blur_u8_host(c, kw, kh, sx, sy, *a),
                      lambda n, c, *a: L.prl_hip_gaussian_blur_u8_batch_device(n, c, kw, kh, sx, sy, *a), out)


def sepFilterU8(pages, wx, wy, out=None):
    """the separable filter alone with explicit 8.8 weights (each side sums to at most 256); device tensors only"""
    L = _capi.lib()
    ax, ay = np.ascontiguousarray(wx, np.uint16), np.ascontiguousarray(wy, np.uint16)
    return _pages.run(pages, _pages.same, None,
                      lambda n, c, *a: L.prl_hip_sep_filter_u8_batch_device(n, c, ax.ctypes.data, ax.size, ay.ctypes.data, ay.size, *a), out)


def cannyEdgeDetection(pages, GaussianBlurKernelSize=19, CannyUpperThresholdCoeff=0.15, CannyLowerThresholdCoeff=0.01,
                       CannyMorphIters=1, out=None):
    """CannyEdgeDetection (imageLibCommon.cpp:244-324): [N,] H x W maps of 0 / 255 from pages of 1 to 4 channels"""
    L = _capi.lib()
    k, up, lo, it = int(GaussianBlurKernelSize), float(CannyUpperThresholdCoeff), float(CannyLowerThresholdCoeff), int(CannyMorphIters)
    return _pages.run(pages, _pages.same,
                      lambda c, *a: L.prl_hip_canny_edge_detection_host(c, k, up, lo, it, *a),
                      lambda n, c, *a: L.prl_hip_canny_edge_detection_batch_device(n, c, k, up, lo, it, *a), out, drop_channel=True)


def externalRects(edge_map):
    """(rects K x 4 int32 of x, y, width, height; contours found) of cv::findContours(RETR_EXTERNAL) on a numpy H x W map: the
    bounding rectangles of the contours of at least 3 points; host code"""
    m = np.ascontiguousarray(edge_map, np.uint8)
    if m.ndim != 2:
        raise TypeError("expected an H x W uint8 map")
    h, w = m.shape
    found, kept = ctypes.c_int(0), ctypes.c_int(0)
    L = _capi.lib()
    _capi.check(L.prl_hip_external_rects(m.ctypes.data, max(w, 1), w, h, None, 0, ctypes.byref(found), ctypes.byref(kept)))
    rects = np.zeros((kept.value, 4), np.int32)
    if kept.value:
        _capi.check(L.prl_hip_external_rects(m.ctypes.data, w, w, h, rects.ctypes.data, kept.value, ctypes.byref(found), ctypes.byref(kept)))
    return rects, found.value


def rectOtsu(gray, rects, maxValue=255.0, out=None, with_thresholds=False):
    """The per-rectangle Otsu and the paint on device tensors.  gray: uint8 CUDA [N,] H x W; rects: one array-like K x 4 of
    (x, y, width, height) per page (a single one for a page without the N).  Returns the mask, with_thresholds: and an int32
    tensor of every rectangle's threshold, page after page."""
    import torch

    t4, _chan, batch = _pages.pages4(gray, gray_only=True)
    n, h, w, _ = t4.shape
    lists = [np.asarray(r, np.int32).reshape(-1, 4) for r in (rects if batch else [rects])]
    if len(lists) != n:
        raise ValueError("one list of rectangles per page")
    offsets = np.zeros(n + 1, np.int32)
    offsets[1:] = np.cumsum([len(r) for r in lists])
    flat = np.concatenate(lists) if lists else np.zeros((0, 4), np.int32)
    d_rects = torch.from_numpy(np.ascontiguousarray(flat)).to(gray.device)
    thr = torch.full((max(len(flat), 1),), -1, dtype=torch.int32, device=gray.device)
    res = torch.empty(tuple(gray.shape), dtype=torch.uint8, device=gray.device) if out is None else out
    if not isinstance(res, torch.Tensor) or res.shape != gray.shape or res.dtype != torch.uint8 or res.device != gray.device:
        raise TypeError("out must be a uint8 tensor of the input's shape on the input's device")
    r3 = res if batch else res[None]
    if r3.stride(2) != 1 and w > 1:
        raise TypeError("out must have dense pixels")
    _capi.check(_capi.lib().prl_hip_rect_otsu_batch_device(n, offsets.ctypes.data, d_rects.data_ptr() if len(flat) else None, float(maxValue),
                                                          t4.data_ptr(), t4.stride(0), t4.stride(1), w, h, r3.data_ptr(), r3.stride(0),
                                                          r3.stride(1), thr.data_ptr() if with_thresholds else None,
                                                          _capi.stream_on(gray)))
    return (res, thr[:len(flat)]) if with_thresholds else res


def binarizeLocalOtsu(pages, maxValue=255.0, CLAHEClipLimit=0.0, GaussianBlurKernelSize=19, CannyUpperThresholdCoeff=0.15,
                      CannyLowerThresholdCoeff=0.01, CannyMorphIters=1, out=None, with_counts=False):
    """prl::binarizeLocalOtsu on pages of 1, 3 or 4 channels: [N,] H x W masks.  with_counts: also (contours found, rectangles
    kept) per page, int32 arrays (ints for a single page); a page without contours is all 255 (the C++ function throws there)."""
    L = _capi.lib()
    mv, clip, k = float(maxValue), float(CLAHEClipLimit), int(GaussianBlurKernelSize)
    up, lo, it = float(CannyUpperThresholdCoeff), float(CannyLowerThresholdCoeff), int(CannyMorphIters)
    counts = {}

    def host(c, *a):
        counts["f"], counts["k"] = np.zeros(1, np.int32), np.zeros(1, np.int32)
        return L.prl_hip_binarize_local_otsu_host(c, mv, clip, k, up, lo, it, *a, counts["f"].ctypes.data, counts["k"].ctypes.data)

    def device(n, c, *a):
        counts["f"], counts["k"] = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        return L.prl_hip_binarize_local_otsu_batch_device(n, c, mv, clip, k, up, lo, it, *a[:-1], counts["f"].ctypes.data,
                                                          counts["k"].ctypes.data, a[-1])

    res = _pages.run(pages, _pages.same, host, device, out, drop_channel=True)
    if not with_counts:
        return res
    single = res.ndim == 2
    return res, (int(counts["f"][0]) if single else counts["f"][:res.shape[0]]), (int(counts["k"][0]) if single else counts["k"][:res.shape[0]])
