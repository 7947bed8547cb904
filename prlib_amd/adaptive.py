"""Host-side mirror of the reference's adaptive-threshold binarizers over the C ABI (adaptive.hip):

    cv::adaptiveThreshold(src, dst, maxValue, adaptiveMethod, thresholdType, blockSize, C)
    prl::binarizeNativeAdaptive      (src/binarizations/binarizeNativeAdaptive.h:62-74, .cpp:34-135)
    prl::binarizeAT / binarizeAGT    (binarizeAT.cpp:33-68, binarizeAGT.cpp:33-60)
    prl::binarizePureAdaptiveGaussian (binarizePureAdaptiveGaussian.cpp:32-75)

numpy H x W [x C] uint8 -> numpy H x W (through the library's host entry); torch CUDA uint8 [N,] H x W [x C] -> torch tensor
[N,] H x W on the same device, enqueued on the current stream (a 3-dimensional tensor is H x W x C when its last dimension is at
most 4, else N x H x W; adaptiveThreshold takes gray pages only: 3 dimensions are always N x H x W).  Pages and rows may be
strided; pixels and channels must be dense.  `out` receives the result.  Errors are PrlError with the C status.
"""
from __future__ import annotations

import math

import numpy as np

from . import _capi, _pages

ADAPTIVE_THRESH_MEAN_C, ADAPTIVE_THRESH_GAUSSIAN_C = 0, 1
THRESH_BINARY, THRESH_BINARY_INV = 0, 1


def _params(median, on_color, method, type_, max_value, block, delta, auto_invert):
    p = _capi.AdaptiveParams()
    p.median_ksize, p.median_on_color, p.method, p.type = int(median), int(on_color), int(method), int(type_)
    p.max_value, p.block_size, p.delta, p.auto_invert = float(max_value), int(block), float(delta), int(bool(auto_invert))
    return p


def _run(image, p, out, gray_only=False):
    import ctypes as C

    L = _capi.lib()
    return _pages.run(image, _pages.same,
                      lambda *a: L.prl_hip_binarize_adaptive_host(C.byref(p), *a),
                      lambda n, *a: L.prl_hip_binarize_adaptive_batch_device(C.byref(p), n, *a), out, gray_only=gray_only,
                      drop_channel=True)


def _channels(image):
    if isinstance(image, np.ndarray):
        return image.shape[2] if image.ndim == 3 else 1
    if image.dim() == 4:
        return image.shape[3]
    return image.shape[2] if image.dim() == 3 and image.shape[2] <= 4 else 1


def adaptiveThreshold(src, maxValue, adaptiveMethod, thresholdType, blockSize, C, autoInvert=False, out=None):
    """cv::adaptiveThreshold on gray pages; autoInvert adds binarizeNativeAdaptive's 255 - mask for masks whose mean is below 128."""
    return _run(src, _params(0, 0, adaptiveMethod, thresholdType, maxValue, blockSize, C, autoInvert), out, gray_only=True)


def auto_block_size(rows: int, cols: int) -> int:
    """binarizeNativeAdaptive.cpp:84-91 (may be even: the call then fails as cv::adaptiveThreshold does)."""
    return int(math.sqrt(float(rows * rows + cols * cols)) / 333 + 7)


def binarizeNativeAdaptive(inputImage, isGaussianBlurReqiured=False, medianBlurKernelSize=5, GaussianBlurKernelSize=7,
                           GaussianBlurSigma=150.0, isAdaptiveThresholdCalculatedByGaussian=True, adaptiveThresholdingMaxValue=255.0,
                           adaptiveThresholdingBlockSize=19, adaptiveThresholdingShift=9.0, bilateralFilterBlockSize=0,
                           bilateralFilterColorSigma=150.0, bilateralFilterSpaceSigma=150.0, out=None):
    """The reference's general-purpose binarizer: [BGR -> gray], median, adaptive threshold (BINARY_INV), 255 - mask where the
    mask's mean is below 128.  The 8-bit cv::GaussianBlur variant and the bilateral filter are not provided."""
    if not (adaptiveThresholdingMaxValue >= 0 and adaptiveThresholdingMaxValue <= 255):
        raise _capi.PrlError(_capi.PRL_ERR_BAD_ARG, "Max value must be in range [0; 255]")
    if isGaussianBlurReqiured or bilateralFilterBlockSize >= 3:
        raise NotImplementedError("the Gaussian-blur and bilateral-filter variants are not provided")
    if medianBlurKernelSize < 3:
        raise _capi.PrlError(_capi.PRL_ERR_BAD_WINDOW, "medianBlurKernelSize >= 3")
    bs = adaptiveThresholdingBlockSize
    if bs < 3:
        shape = inputImage.shape
        nd = len(shape)
        hw = shape[:2] if nd == 2 or (nd == 3 and shape[2] <= 4) else shape[1:3]
        bs = auto_block_size(int(hw[0]), int(hw[1]))
    method = ADAPTIVE_THRESH_GAUSSIAN_C if isAdaptiveThresholdCalculatedByGaussian else ADAPTIVE_THRESH_MEAN_C
    return _run(inputImage, _params(medianBlurKernelSize, 0, method, THRESH_BINARY_INV, adaptiveThresholdingMaxValue, bs,
                                    adaptiveThresholdingShift, True), out)


def _colour_only(image, name):
    # the reference hands an empty Mat to cv::adaptiveThreshold for a 1-channel input (binarizeAT.cpp:56-65): an exception there
    if _channels(image) == 1:
        raise _capi.PrlError(_capi.PRL_ERR_BAD_CHANNELS, name + " needs a 3- or 4-channel input (the reference throws for gray)")


def _median_size(k):
    if k < 1 or k % 2 == 0:   # cv::medianBlur: ksize % 2 == 1
        raise _capi.PrlError(_capi.PRL_ERR_BAD_WINDOW, "medianKernelSize must be odd and positive")
    return k


def binarizeAT(inputImage, medianKernelSize, maxValue, blockSize, shift, out=None):
    """median on the colour page, BGR -> gray, ADAPTIVE_THRESH_MEAN_C / THRESH_BINARY with an integer shift."""
    _colour_only(inputImage, "binarizeAT")
    return _run(inputImage, _params(_median_size(medianKernelSize), 1, ADAPTIVE_THRESH_MEAN_C, THRESH_BINARY, maxValue, blockSize, int(shift), False), out)


def binarizeAGT(inputImage, medianKernelSize, maxValue, blockSize, shift, out=None):
    """median on the colour page, BGR -> gray, ADAPTIVE_THRESH_GAUSSIAN_C / THRESH_BINARY with an integer shift."""
    _colour_only(inputImage, "binarizeAGT")
    return _run(inputImage, _params(_median_size(medianKernelSize), 1, ADAPTIVE_THRESH_GAUSSIAN_C, THRESH_BINARY, maxValue, blockSize, int(shift), False), out)


def binarizePureAdaptiveGaussian(inputImage, maxValue, blockSize, shift, out=None):
    """BGR -> gray, ADAPTIVE_THRESH_GAUSSIAN_C / THRESH_BINARY with an integer shift."""
    _colour_only(inputImage, "binarizePureAdaptiveGaussian")
    return _run(inputImage, _params(0, 0, ADAPTIVE_THRESH_GAUSSIAN_C, THRESH_BINARY, maxValue, blockSize, int(shift), False), out)
