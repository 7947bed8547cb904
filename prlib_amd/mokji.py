"""prl::binarizeMokji (mokji.hip) over the C ABI: one global threshold per page from the co-occurrence matrix of the page and its
square dilation (Mokji & Abu-Bakar 2007), and the co-occurrence primitive itself.

    void prl::binarizeMokji(const cv::Mat& in, cv::Mat& out, size_t maxEdgeWidth = 3, size_t minEdgeMagnitude = 20)
                                                                    (src/binarizations/binarizeMokji.h:46, binarizeMokji.cpp:35-94)
        gray = BGR2GRAY; dil = dilate(gray, RECT (2E + 1)^2); matrix[dil][gray] over the interior [E, rows - E) x [E, cols - E);
        t = (int)(0.5 * sum (m + n) matrix[n][m] / sum matrix[n][m] + 0.5) over n - m >= M; out = gray > t ? 255 : 0.
        No pair (no interior, no edge of M, M >= 256): the page comes out all 255 and t is reported as -1 (include/prl_hip.h).

numpy H x W or H x W x 3 / 4 uint8 -> numpy H x W (through the library's host entry); torch CUDA uint8 [N,] H x W [x 3 / 4] -> torch
tensor without the channel axis on the same device, enqueued on the current stream (a 3-dimensional tensor is H x W x C when its
last dimension is at most 4, else N x H x W: the rule of morphology.py).  Unlike the C++ function the entries here also take gray
pages.  Pages and rows may be strided; pixels and channels must be dense.  `out` receives the result (for 1-channel pages out may
be pages: in place).  Errors are PrlError with the C status.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi


def _pages4(t):
    import torch

    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_cuda or t.dim() not in (2, 3, 4):
        raise TypeError("expected a uint8 CUDA tensor [N,] H x W [x C] or a numpy uint8 array")
    if t.dim() == 2:
        t4, oshape = t[None, :, :, None], tuple(t.shape)
    elif t.dim() == 3 and t.shape[-1] <= 4:
        t4, oshape = t[None], tuple(t.shape[:2])
    elif t.dim() == 3:
        t4, oshape = t[:, :, :, None], tuple(t.shape)
    else:
        t4, oshape = t, tuple(t.shape[:3])
    c = t4.shape[3]
    if t4.stride(3) != 1 and c > 1 or t4.stride(2) != c:
        t4 = t4.contiguous()
    return t4, oshape


def binarizeMokji(pages, maxEdgeWidth=3, minEdgeMagnitude=20, out=None):
    """prl::binarizeMokji: 255 where gray is above the page's co-occurrence threshold, else 0."""
    L = _capi.lib()
    e, m = int(maxEdgeWidth), int(minEdgeMagnitude)
    if isinstance(pages, np.ndarray):
        if pages.dtype != np.uint8 or pages.ndim not in (2, 3):
            raise TypeError("expected an H x W [x C] uint8 array")
        img = pages if pages.ndim == 3 else pages[:, :, None]
        if img.strides[2] != 1 or img.strides[1] != img.shape[2] or img.strides[0] < 0:
            img = np.ascontiguousarray(img)
        h, w, c = img.shape
        res = np.empty((h, w), np.uint8) if out is None else out
        if not isinstance(res, np.ndarray) or res.shape != (h, w) or res.dtype != np.uint8 or not res.flags.c_contiguous:
            raise TypeError("out must be a C-contiguous H x W uint8 array")
        _capi.check(L.prl_hip_binarize_mokji_host(c, e, m, img.ctypes.data, img.strides[0], w, h, res.ctypes.data, res.strides[0]))
        return res
    import torch

    t4, oshape = _pages4(pages)
    n, h, w, c = t4.shape
    res = torch.empty(oshape, dtype=torch.uint8, device=pages.device) if out is None else out
    if not isinstance(res, torch.Tensor) or tuple(res.shape) != oshape or res.dtype != torch.uint8 or res.device != pages.device \
            or res.stride(-1) != 1:
        raise TypeError("out must be a uint8 tensor [N,] H x W on the input's device, pixels dense")
    r3 = res if res.dim() == 3 else res[None]
    _capi.check(L.prl_hip_set_device(pages.device.index or 0))
    stream = torch.cuda.current_stream(pages.device).cuda_stream
    _capi.check(L.prl_hip_binarize_mokji_batch_device(n, c, e, m, t4.data_ptr(), t4.stride(0), t4.stride(1), w, h, r3.data_ptr(),
                                                      r3.stride(0), r3.stride(1), stream))
    return res


def mokjiThresholds(pages, maxEdgeWidth=3, minEdgeMagnitude=20, out=None):
    """The thresholds alone: a torch int32 tensor [N] (or a scalar tensor for one page) on the input's device, -1 where a page has
    no pair; nothing is synchronised.  `out` (int32, contiguous) is overwritten."""
    import torch

    L = _capi.lib()
    t4, oshape = _pages4(pages)
    n, h, w, c = t4.shape
    tshape = oshape[:-2]
    res = torch.empty(tshape, dtype=torch.int32, device=pages.device) if out is None else out
    if not isinstance(res, torch.Tensor) or tuple(res.shape) != tshape or res.dtype != torch.int32 or res.device != pages.device \
            or not res.is_contiguous():
        raise TypeError("out must be a contiguous int32 tensor [N] on the input's device")
    _capi.check(L.prl_hip_set_device(pages.device.index or 0))
    stream = torch.cuda.current_stream(pages.device).cuda_stream
    _capi.check(L.prl_hip_mokji_thresholds_batch_device(n, c, int(maxEdgeWidth), int(minEdgeMagnitude), t4.data_ptr(), t4.stride(0),
                                                        t4.stride(1), w, h, res.data_ptr(), stream))
    return res


def cooccurrence(a, b, border=0, min_diff=0, out=None):
    """out[page][b(y, x)][a(y, x)] = the number of interior pixels (`border` rows and columns dropped all round) with that pair of
    values, for the pairs with b - a >= min_diff: a torch int32 tensor [N,] 256 x 256 holding the uint32 counts, on the input's
    device.  a, b: uint8 CUDA tensors [N,] H x W of the same shape; `out` (int32, contiguous) is overwritten."""
    import torch

    L = _capi.lib()
    for t in (a, b):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_cuda or t.dim() not in (2, 3):
            raise TypeError("expected two uint8 CUDA tensors [N,] H x W")
    if a.shape != b.shape or a.device != b.device:
        raise TypeError("a and b must have the same shape and device")
    a3, b3 = (a, b) if a.dim() == 3 else (a[None], b[None])
    if a3.stride(2) != 1:
        a3 = a3.contiguous()
    if b3.stride(2) != 1:
        b3 = b3.contiguous()
    n, h, w = a3.shape
    oshape = tuple(a.shape[:-2]) + (256, 256)
    res = torch.empty(oshape, dtype=torch.int32, device=a.device) if out is None else out
    if not isinstance(res, torch.Tensor) or tuple(res.shape) != oshape or res.dtype != torch.int32 or res.device != a.device \
            or not res.is_contiguous():
        raise TypeError("out must be a contiguous int32 tensor [N,] 256 x 256 on the input's device")
    _capi.check(L.prl_hip_set_device(a.device.index or 0))
    stream = torch.cuda.current_stream(a.device).cuda_stream
    _capi.check(L.prl_hip_cooccurrence_batch_device(n, int(border), int(min_diff), a3.data_ptr(), a3.stride(0), a3.stride(1),
                                                    b3.data_ptr(), b3.stride(0), b3.stride(1), w, h, res.data_ptr(), stream))
    return res


def mokjiThreshold(cooc, minEdgeMagnitude=20):
    """Step 6 on the host (no device): the threshold of a 256 x 256 matrix of counts [n][m], -1 where no pair has n - m >= M."""
    m = np.ascontiguousarray(cooc, np.uint32)
    if m.shape != (256, 256):
        raise TypeError("expected a 256 x 256 matrix")
    t = C.c_int(0)
    _capi.check(_capi.lib().prl_hip_mokji_threshold(m.ctypes.data, int(minEdgeMagnitude), C.byref(t)))
    return t.value
