"""Grayscale morphology with a flat structuring element, and prl::correctNUIL on top of it (gmorph.hip), over the C ABI.

    void prl::correctNUIL(const cv::Mat& inputImage, cv::Mat& outputImage, int structuringElementSize = 31)
        (src/correctNUIL.h, correctNUIL.cpp:33-90): per channel, x ^ 255 where the channel's mean over the page is below 128,
        then 255 - cv::morphologyEx(channel, MORPH_BLACKHAT, getStructuringElement(MORPH_ELLIPSE, Size(size, size)))

    morphologyEx(pages, op, shape, ksize) = cv::morphologyEx(src, dst, op, cv::getStructuringElement(shape, ksize)), one
        iteration, default anchor and border.

    morphology_ex(pages, op, shape, ksize, anchor=(-1, -1), iterations=1) = cv::morphologyEx(src, dst, op, element, anchor,
        iterations): an anchor of -1 is the centre; a full rectangle runs once, grown over the iterations, cross and ellipse run
        every pass; the composite operators apply `iterations` to each half.

numpy H x W or H x W x C uint8 -> numpy (through the library's host entry); torch CUDA uint8 [N,] H x W [x C] -> torch tensor on
the same device, enqueued on the current stream (a 3-dimensional tensor is H x W x C when its last dimension is at most 4, else
N x H x W).  Pages and rows may be strided; pixels and channels must be dense.  `out` receives the result (out is pages: in
place).  Errors are PrlError with the C status.
"""
from __future__ import annotations

import numpy as np

from . import _capi, _pages

MORPH_ERODE, MORPH_DILATE, MORPH_OPEN, MORPH_CLOSE, MORPH_TOPHAT, MORPH_BLACKHAT = 0, 1, 2, 3, 5, 6
MORPH_RECT, MORPH_CROSS, MORPH_ELLIPSE = 0, 1, 2


def correctNUIL(pages, size: int = 31, out=None):
    """prl::correctNUIL: removes non-uniform illumination; `size` is the ellipse's diameter (1 .. 255)."""
    size, L = int(size), _capi.lib()
    return _pages.run(pages, _pages.same,
                      lambda c, *a: L.prl_hip_correct_nuil_host(c, size, *a),
                      lambda n, c, *a: L.prl_hip_correct_nuil_batch_device(n, c, size, *a), out)


def morphologyEx(pages, op: int, shape: int, ksize, out=None):
    """cv::morphologyEx with cv::getStructuringElement(shape, ksize); ksize is (width, height) or one number for both."""
    kw, kh = (int(ksize), int(ksize)) if np.isscalar(ksize) else (int(ksize[0]), int(ksize[1]))
    op, shape, L = int(op), int(shape), _capi.lib()
    return _pages.run(pages, _pages.same,
                      lambda c, *a: L.prl_hip_morphology_host(c, op, shape, kw, kh, *a),
                      lambda n, c, *a: L.prl_hip_morphology_batch_device(n, c, op, shape, kw, kh, *a), out)


def morphology_ex(pages, op: int, shape: int, ksize, anchor=(-1, -1), iterations: int = 1, out=None):
    """cv::morphologyEx with cv::getStructuringElement(shape, ksize), cv::Point(*anchor) and `iterations` (1 .. 16)."""
    kw, kh = (int(ksize), int(ksize)) if np.isscalar(ksize) else (int(ksize[0]), int(ksize[1]))
    ax, ay, n = int(anchor[0]), int(anchor[1]), int(iterations)
    op, shape, L = int(op), int(shape), _capi.lib()
    return _pages.run(pages, _pages.same,
                      lambda c, *a: L.prl_hip_morphology_ex_host(c, op, shape, kw, kh, ax, ay, n, *a),
                      lambda m, c, *a: L.prl_hip_morphology_ex_batch_device(m, c, op, shape, kw, kh, ax, ay, n, *a), out)
