"""Grayscale morphology with a flat structuring element, and prl::correctNUIL on top of it (gmorph.hip), over the C ABI.

    void prl::correctNUIL(const cv::Mat& inputImage, cv::Mat& outputImage, int structuringElementSize = 31)
        (src/correctNUIL.h, correctNUIL.cpp:33-90): per channel, x ^ 255 where the channel's mean over the page is below 128,
        then 255 - cv::morphologyEx(channel, MORPH_BLACKHAT, getStructuringElement(MORPH_ELLIPSE, Size(size, size)))

    morphologyEx(pages, op, shape, ksize) = cv::morphologyEx(src, dst, op, cv::getStructuringElement(shape, ksize)), one
        iteration, default anchor and border.

numpy H x W or H x W x C uint8 -> numpy (through the library's host entry); torch CUDA uint8 [N,] H x W [x C] -> torch tensor on
the same device, enqueued on the current stream (a 3-dimensional tensor is H x W x C when its last dimension is at most 4, else
N x H x W).  Pages and rows may be strided; pixels and channels must be dense.  `out` receives the result (out is pages: in
place).  Errors are PrlError with the C status.
"""
from __future__ import annotations

import numpy as np

from . import _capi

MORPH_ERODE, MORPH_DILATE, MORPH_OPEN, MORPH_CLOSE, MORPH_TOPHAT, MORPH_BLACKHAT = 0, 1, 2, 3, 5, 6
MORPH_RECT, MORPH_CROSS, MORPH_ELLIPSE = 0, 1, 2


def _run(image, out, host, device):
    """host(c, src, src_step, w, h, dst, dst_step) / device(n, c, src, page, step, w, h, dst, page, step, stream) -> status"""
    L = _capi.lib()
    if isinstance(image, np.ndarray):
        if image.dtype != np.uint8 or image.ndim not in (2, 3):
            raise TypeError("expected an H x W [x C] uint8 array")
        img = image if image.ndim == 3 else image[:, :, None]
        if img.strides[2] != 1 or img.strides[1] != img.shape[2] or img.strides[0] < 0:
            img = np.ascontiguousarray(img)
        h, w, c = img.shape
        res = np.empty(image.shape, np.uint8) if out is None else out
        if not isinstance(res, np.ndarray) or res.shape != image.shape or res.dtype != np.uint8 or not res.flags.c_contiguous:
            raise TypeError("out must be a C-contiguous uint8 array of the input's shape")
        _capi.check(host(L, c, img.ctypes.data, img.strides[0], w, h, res.ctypes.data, res.strides[0] if res.ndim else 0))
        return res
    import torch

    t = image
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_cuda or t.dim() not in (2, 3, 4):
        raise TypeError("expected a uint8 CUDA tensor [N,] H x W [x C] or a numpy uint8 array")

    def as4(x):
        if x.dim() == 2:
            return x[None, :, :, None]
        if x.dim() == 3:
            return x[None] if x.shape[-1] <= 4 else x[:, :, :, None]
        return x

    t4 = as4(t)
    n, h, w, c = t4.shape
    if t4.stride(3) != 1 and c > 1 or t4.stride(2) != c:
        t4 = t4.contiguous()
    res = torch.empty(t.shape, dtype=torch.uint8, device=t.device) if out is None else out
    r4 = as4(res)
    if r4.shape != t4.shape or res.dtype != torch.uint8 or res.device != t.device or (r4.stride(3) != 1 and c > 1) or r4.stride(2) != c:
        raise TypeError("out must be a uint8 tensor of the input's shape on its device, pixels and channels dense")
    _capi.check(L.prl_hip_set_device(t.device.index or 0))
    stream = torch.cuda.current_stream(t.device).cuda_stream
    _capi.check(device(L, n, c, t4.data_ptr(), t4.stride(0), t4.stride(1), w, h, r4.data_ptr(), r4.stride(0), r4.stride(1), stream))
    return res


def correctNUIL(pages, size: int = 31, out=None):
    """prl::correctNUIL: removes non-uniform illumination; `size` is the ellipse's diameter (1 .. 255)."""
    size = int(size)
    return _run(pages, out,
                lambda L, c, *a: L.prl_hip_correct_nuil_host(c, size, *a),
                lambda L, n, c, *a: L.prl_hip_correct_nuil_batch_device(n, c, size, *a))


def morphologyEx(pages, op: int, shape: int, ksize, out=None):
    """cv::morphologyEx with cv::getStructuringElement(shape, ksize); ksize is (width, height) or one number for both."""
    kw, kh = (int(ksize), int(ksize)) if np.isscalar(ksize) else (int(ksize[0]), int(ksize[1]))
    op, shape = int(op), int(shape)
    return _run(pages, out,
                lambda L, c, *a: L.prl_hip_morphology_host(c, op, shape, kw, kh, *a),
                lambda L, n, c, *a: L.prl_hip_morphology_batch_device(n, c, op, shape, kw, kh, *a))
