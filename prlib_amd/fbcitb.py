"""cv::bilateralFilter on 8-bit planes (bilateral.hip) and the parts of prl::binarizeFBCITB that are its own (fbcitb.hip, contour.h)
over the C ABI: the variance mask, the contour tree of cv::findContours(RETR_TREE) with RemoveChildrenContours and the per-contour
decision (host code), and the ordered paint of the rectangles.  The rules are stated in include/prl_hip.h.

numpy H x W [x C] uint8 goes through the library's host entry; torch CUDA uint8 [N,] H x W [x C] is enqueued on the current stream
(the rule of _pages.py).  Errors are PrlError with the C status.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _capi, _pages

BILATERAL_MAX_SIDE = 31
BILATERAL_MAX_TAPS = 708


def bilateralTables(d, sigmaColor, sigmaSpace):
    """(radius, offsets int8 [taps, 2] of (dy, dx) in tap order, space weights float32 [taps], colour weights float32 [256]) of
    cv::bilateralFilter(d, sigmaColor, sigmaSpace) on an 8-bit plane; on the host (no device)"""
    radius, n = ctypes.c_int(0), ctypes.c_int(0)
    dy, dx = np.zeros(BILATERAL_MAX_TAPS, np.int8), np.zeros(BILATERAL_MAX_TAPS, np.int8)
    space, color = np.zeros(BILATERAL_MAX_TAPS, np.float32), np.zeros(256, np.float32)
    _capi.check(_capi.lib().prl_hip_bilateral_tables(int(d), float(sigmaColor), float(sigmaSpace), ctypes.byref(radius), ctypes.byref(n),
                                                     dy.ctypes.data, dx.ctypes.data, space.ctypes.data, color.ctypes.data))
    k = n.value
    return radius.value, np.stack([dy[:k], dx[:k]], axis=1), space[:k].copy(), color


def bilateralFilter(pages, d, sigmaColor, sigmaSpace, out=None):
    """cv::bilateralFilter(pages, d, sigmaColor, sigmaSpace) on 8-bit pages of 1 to 4 channels, every channel filtered as a plane of
    its own, BORDER_REFLECT_101; sides up to 31"""
    L = _capi.lib()
    dd, sc, ss = int(d), float(sigmaColor), float(sigmaSpace)
    return _pages.run(pages, _pages.same,
                      lambda c, *a: L.prl_hip_bilateral_filter_host(c, dd, sc, ss, *a),
                      lambda n, c, *a: L.prl_hip_bilateral_filter_batch_device(n, c, dd, sc, ss, *a), out)


def varianceMask(pages, threshold=200.0, out=None):
    """MatToLocalVarianceMap(page, 3) > threshold on every channel, AND-ed: [N,] H x W maps of 0 / 255 from device pages of 1 or 3
    channels (binarizeFBCITB.cpp:172-183)"""
    L = _capi.lib()
    thr = float(threshold)
    return _pages.run(pages, _pages.same, None, lambda n, c, *a: L.prl_hip_variance_mask_batch_device(n, c, thr, *a), out, drop_channel=True)


def findContoursTree(edge_map):
    """cv::findContours(map, RETR_TREE, CHAIN_APPROX_SIMPLE) on an H x W uint8 numpy map -> ([K x 2 int32 points per border],
    hierarchy M x 4 int32 of (next, previous, first child, parent), holes M bool) in OpenCV's order.  Host code."""
    m = _pages.host_image(edge_map, gray_only=True)
    h, w = m.shape[:2]
    L = _capi.lib()
    npts, ncs = ctypes.c_int(0), ctypes.c_int(0)
    _capi.check(L.prl_hip_find_contours_tree(m.ctypes.data, m.strides[0], w, h, None, 0, None, 0, ctypes.byref(npts), ctypes.byref(ncs)))
    pts = np.zeros((max(npts.value, 1), 2), np.int32)
    cs = np.zeros((max(ncs.value, 1), 6), np.int32)
    _capi.check(L.prl_hip_find_contours_tree(m.ctypes.data, m.strides[0], w, h, pts.ctypes.data, npts.value, cs.ctypes.data, ncs.value,
                                             ctypes.byref(npts), ctypes.byref(ncs)))
    cs = cs[:ncs.value]
    ends = np.cumsum(cs[:, 0]) if len(cs) else np.zeros(0, np.int64)
    contours = [pts[int(e - c):int(e)].copy() for e, c in zip(ends, cs[:, 0])]
    return contours, cs[:, 2:6].copy(), cs[:, 1].astype(bool)


def removeChildrenContours(counts, hierarchy):
    """RemoveChildrenContours on a pre-order hierarchy (M x 4 of next, previous, first child, parent) whose contours have `counts`
    points: a bool array of the contours it keeps.  Host code."""
    hier = np.asarray(hierarchy, np.int32).reshape(-1, 4)
    rec = np.zeros((max(len(hier), 1), 6), np.int32)
    rec[:len(hier), 0] = np.asarray(counts, np.int32)
    rec[:len(hier), 2:] = hier
    ok = np.zeros(max(len(hier), 1), np.uint8)
    _capi.check(_capi.lib().prl_hip_remove_children_contours(rec.ctypes.data, len(hier), ok.ctypes.data))
    return ok[:len(hier)].astype(bool)


def fbcitbContours(contour_map, gray, boundingRectangleMaxArea=0.3):
    """(rects K x 6 int32 of x, y, width, height, cut, below; (found, approved, kept)) of binarizeFBCITB.cpp:196-357 on numpy H x W
    maps: the contour map and the gray plane of the processed page.  Host code."""
    m, g = _pages.host_image(contour_map, gray_only=True), _pages.host_image(gray, gray_only=True)
    if m.shape != g.shape:
        raise ValueError("map and gray plane must have one size")
    h, w = m.shape[:2]
    L = _capi.lib()
    counts = np.zeros(3, np.int32)
    area = float(boundingRectangleMaxArea)
    _capi.check(L.prl_hip_fbcitb_contours(m.ctypes.data, m.strides[0], g.ctypes.data, g.strides[0], w, h, area, None, 0, counts.ctypes.data))
    rects = np.zeros((max(int(counts[2]), 1), 6), np.int32)
    _capi.check(L.prl_hip_fbcitb_contours(m.ctypes.data, m.strides[0], g.ctypes.data, g.strides[0], w, h, area, rects.ctypes.data,
                                          int(counts[2]), counts.ctypes.data))
    return rects[:int(counts[2])], tuple(int(v) for v in counts)


def rectPaint(gray, rects, out=None):
    """The ordered paint on device tensors.  gray: uint8 CUDA [N,] H x W; rects: one array-like K x 6 of (x, y, width, height, cut,
    below) per page (a single one for a page without the N); where rectangles overlap the later one wins."""
    import torch

    t4, _chan, batch = _pages.pages4(gray, gray_only=True)
    n, h, w, _ = t4.shape
    lists = [np.asarray(r, np.int32).reshape(-1, 6) for r in (rects if batch else [rects])]
    if len(lists) != n:
        raise ValueError("one list of rectangles per page")
    offsets = np.zeros(n + 1, np.int32)
    offsets[1:] = np.cumsum([len(r) for r in lists])
    flat = np.concatenate(lists) if lists else np.zeros((0, 6), np.int32)
    d_rects = torch.from_numpy(np.ascontiguousarray(flat)).to(gray.device)
    res = torch.empty(tuple(gray.shape), dtype=torch.uint8, device=gray.device) if out is None else out
    if not isinstance(res, torch.Tensor) or res.shape != gray.shape or res.dtype != torch.uint8 or res.device != gray.device:
        raise TypeError("out must be a uint8 tensor of the input's shape on the input's device")
    r3 = res if batch else res[None]
    if r3.stride(2) != 1 and w > 1:
        raise TypeError("out must have dense pixels")
    _capi.check(_capi.lib().prl_hip_rect_paint_batch_device(n, offsets.ctypes.data, d_rects.data_ptr() if len(flat) else None, t4.data_ptr(),
                                                           t4.stride(0), t4.stride(1), w, h, r3.data_ptr(), r3.stride(0), r3.stride(1),
                                                           _capi.stream_on(gray)))
    return res


def binarizeFBCITB(pages, useCanny=True, useVariancesMap=True, useCLAHE=True, useBilateral=True, useOtherColorspace=False,
                   useMorphology=True, useCannyOnVariances=True, varianceMapThreshold=200.0, CLAHEClipLimit=2.0,
                   gaussianBlurKernelSize=9.0, cannyUpperThresholdCoeff=0.6, cannyLowerThresholdCoeff=0.4, boundingRectangleMaxArea=0.3,
                   bilateralKernelSize=5, bilateralKernelIntensitySigma=150.0, bilateralKernelSpatialSigma=150.0,
                   boundingRectMaxAreaCoeff=0.3, out=None, with_counts=False):
    """prl::binarizeFBCITB on pages of 1 or 3 channels (BGR): [N,] H x W masks.  with_counts: also an int32 array [N, 3] ([3] for a
    single page) of the contours found / approved by RemoveChildrenContours / kept by the rectangle filters."""
    L = _capi.lib()
    p = _capi.FbcitbParams()
    L.prl_hip_default_fbcitb_params(ctypes.byref(p))
    p.use_canny, p.use_variances_map, p.use_clahe, p.use_bilateral = int(bool(useCanny)), int(bool(useVariancesMap)), int(bool(useCLAHE)), int(bool(useBilateral))
    p.use_other_colorspace, p.use_morphology, p.use_canny_on_variances = int(bool(useOtherColorspace)), int(bool(useMorphology)), int(bool(useCannyOnVariances))
    p.bilateral_kernel_size = int(bilateralKernelSize)
    p.variance_map_threshold, p.clahe_clip_limit, p.gaussian_blur_kernel_size = float(varianceMapThreshold), float(CLAHEClipLimit), float(gaussianBlurKernelSize)
    p.canny_upper_threshold_coeff, p.canny_lower_threshold_coeff = float(cannyUpperThresholdCoeff), float(cannyLowerThresholdCoeff)
    p.bounding_rectangle_max_area = float(boundingRectangleMaxArea)
    p.bilateral_kernel_intensity_sigma, p.bilateral_kernel_spatial_sigma = float(bilateralKernelIntensitySigma), float(bilateralKernelSpatialSigma)
    p.bounding_rect_max_area_coeff = float(boundingRectMaxAreaCoeff)
    counts = {}

    def host(c, *a):
        counts["c"] = np.zeros((1, 3), np.int32)
        return L.prl_hip_binarize_fbcitb_host(ctypes.byref(p), c, *a, counts["c"].ctypes.data)

    def device(n, c, *a):
        counts["c"] = np.zeros((max(n, 1), 3), np.int32)
        return L.prl_hip_binarize_fbcitb_batch_device(ctypes.byref(p), n, c, *a[:-1], counts["c"].ctypes.data, a[-1])

    res = _pages.run(pages, _pages.same, host, device, out, drop_channel=True)
    if not with_counts:
        return res
    return res, (counts["c"][0] if res.ndim == 2 else counts["c"][:res.shape[0]])
