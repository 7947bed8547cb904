"""prl::basicDeblur and the float32 cv::GaussianBlur of 8-bit pages it is built on (deblur.hip) over the C ABI; the rules - the
derived kernel size, the weights, the border, the order of the float32 operations - are stated in include/prl_hip.h.

    void prl::basicDeblur(const cv::Mat&, cv::Mat&, size_t gaussianKernelSize = 0, double sigmaX = 9.0, double sigmaY = 0.0,
                          double imageWeight = 0.75)                                          (src/deblur/basicDeblur.h:32-34)

numpy H x W [x C] uint8 goes through the library's host entry; torch CUDA uint8 [N,] H x W [x C] is enqueued on the current
stream (a 3-dimensional tensor is H x W x C when its last dimension is at most 4, else N x H x W: the rule of _pages.py).  1 to 4
channels; pages and rows may be strided, pixels and channels must be dense.  Source and result never share memory.  Errors are
PrlError with the C status.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _capi, _pages

MAX_SIDE = 255


def basicDeblur(pages, gaussianKernelSize=0, sigmaX=9.0, sigmaY=0.0, imageWeight=0.75, out=None):
    """out = saturate_u8(cvRound(x * (float)(2 w) + GaussianBlur_f32(x) * (float)(2 w - 2))) on every channel; the input's shape"""
    L = _capi.lib()
    k, sx, sy, wt = int(gaussianKernelSize), float(sigmaX), float(sigmaY), float(imageWeight)
    return _pages.run(pages, _pages.same,
                      lambda c, *a: L.prl_hip_basic_deblur_host(c, k, sx, sy, wt, *a),
                      lambda n, c, *a: L.prl_hip_basic_deblur_batch_device(n, c, k, sx, sy, wt, *a), out)


def gaussianBlurF32(pages, ksize=(0, 0), sigmaX=9.0, sigmaY=0.0, out=None):
    """cv::GaussianBlur(float(pages), ksize = (width, height), sigmaX, sigmaY) in float32, BORDER_REFLECT_101: a float32 result of
    the input's shape.  `out` (float32, dense rows of W [x C] floats; pages and rows may be strided by multiples of 4 bytes) receives it."""
    L = _capi.lib()
    kw, kh, sx, sy = int(ksize[0]), int(ksize[1]), float(sigmaX), float(sigmaY)
    if isinstance(pages, np.ndarray):
        img = _pages.host_image(pages)
        h, w, c = img.shape
        res = np.empty(pages.shape, np.float32) if out is None else out
        if not isinstance(res, np.ndarray) or res.shape != pages.shape or res.dtype != np.float32 or not res.flags.c_contiguous:
            raise TypeError("out must be a C-contiguous float32 array of the input's shape")
        _capi.check(L.prl_hip_gaussian_blur_f32_host(c, kw, kh, sx, sy, img.ctypes.data, img.strides[0], w, h, res.ctypes.data,
                                                     max(w * c * 4, 4)))
        return res
    import torch

    t4, chan, batch = _pages.pages4(pages)
    n, h, w, c = t4.shape
    oshape = ((n,) if batch else ()) + (h, w) + ((c,) if chan else ())
    res = torch.empty(oshape, dtype=torch.float32, device=pages.device) if out is None else out
    if not isinstance(res, torch.Tensor) or tuple(res.shape) != oshape or res.dtype != torch.float32 or res.device != pages.device:
        raise TypeError("out must be a float32 tensor of the input's shape on the input's device")
    r4 = res if batch else res[None]
    r4 = r4 if chan else r4[:, :, :, None]
    if r4.stride(3) != 1 and c > 1 or r4.stride(2) != c and (chan or w > 1):
        raise TypeError("out must have dense pixels and channels")
    _capi.check(L.prl_hip_gaussian_blur_f32_batch_device(n, c, kw, kh, sx, sy, t4.data_ptr(), t4.stride(0), t4.stride(1), w, h,
                                                         r4.data_ptr(), r4.stride(0) * 4, r4.stride(1) * 4, _capi.stream_on(pages)))
    return res


def gaussianKernelF32(n, sigma=0.0):
    """cv::getGaussianKernel(n, sigma, CV_32F) as cv::GaussianBlur asks for it: float32 [n], on the host (no device)"""
    w = np.empty(max(int(n), 0), np.float32)
    _capi.check(_capi.lib().prl_hip_gaussian_kernel_f32(int(n), float(sigma), w.ctypes.data))
    return w


def gaussianBlurSize(ksize=(0, 0), sigmaX=9.0, sigmaY=0.0):
    """the (width, height) of the kernel cv::GaussianBlur(ksize, sigmaX, sigmaY) filters a float32 image with, on the host"""
    kw, kh = ctypes.c_int(0), ctypes.c_int(0)
    _capi.check(_capi.lib().prl_hip_gaussian_blur_size(int(ksize[0]), int(ksize[1]), float(sigmaX), float(sigmaY), ctypes.byref(kw),
                                                       ctypes.byref(kh)))
    return kw.value, kh.value
