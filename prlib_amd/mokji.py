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

from . import _capi, _pages


def binarizeMokji(pages, maxEdgeWidth=3, minEdgeMagnitude=20, out=None):
    """prl::binarizeMokji: 255 where gray is above the page's co-occurrence threshold, else 0."""
    L = _capi.lib()
    e, m = int(maxEdgeWidth), int(minEdgeMagnitude)
    return _pages.run(pages, _pages.same,
                      lambda c, *a: L.prl_hip_binarize_mokji_host(c, e, m, *a),
                      lambda n, c, *a: L.prl_hip_binarize_mokji_batch_device(n, c, e, m, *a), out, drop_channel=True)


def mokjiThresholds(pages, maxEdgeWidth=3, minEdgeMagnitude=20, out=None):
    """The thresholds alone: a torch int32 tensor [N] (or a scalar tensor for one page) on the input's device, -1 where a page has
    no pair; nothing is synchronised.  `out` (int32, contiguous) is overwritten."""
    import torch

    L = _capi.lib()
    t4, _, batch = _pages.pages4(pages)
    n, h, w, c = t4.shape
    tshape = (n,) if batch else ()
    res = torch.empty(tshape, dtype=torch.int32, device=pages.device) if out is None else out
    if not isinstance(res, torch.Tensor) or tuple(res.shape) != tshape or res.dtype != torch.int32 or res.device != pages.device \
            or not res.is_contiguous():
        raise TypeError("out must be a contiguous int32 tensor [N] on the input's device")
    _capi.check(L.prl_hip_mokji_thresholds_batch_device(n, c, int(maxEdgeWidth), int(minEdgeMagnitude), t4.data_ptr(), t4.stride(0),
                                                        t4.stride(1), w, h, res.data_ptr(), _capi.stream_on(pages)))
    return res


def cooccurrence(a, b, border=0, min_diff=0, out=None):
    """out[page][b(y, x)][a(y, x)] = the number of interior pixels (`border` rows and columns dropped all round) with that pair of
    values, for the pairs with b - a >= min_diff: a torch int32 tensor [N,] 256 x 256 holding the uint32 counts, on the input's
    device.  a, b: uint8 CUDA tensors [N,] H x W of the same shape; `out` (int32, contiguous) is overwritten."""
    import torch

    L = _capi.lib()
    a4, b4 = _pages.pages4(a, gray_only=True)[0], _pages.pages4(b, gray_only=True)[0]
    if a.shape != b.shape or a.device != b.device:
        raise TypeError("a and b must have the same shape and device")
    n, h, w, _ = a4.shape
    oshape = tuple(a.shape[:-2]) + (256, 256)
    res = torch.empty(oshape, dtype=torch.int32, device=a.device) if out is None else out
    if not isinstance(res, torch.Tensor) or tuple(res.shape) != oshape or res.dtype != torch.int32 or res.device != a.device \
            or not res.is_contiguous():
        raise TypeError("out must be a contiguous int32 tensor [N,] 256 x 256 on the input's device")
    _capi.check(L.prl_hip_cooccurrence_batch_device(n, int(border), int(min_diff), a4.data_ptr(), a4.stride(0), a4.stride(1),
                                                    b4.data_ptr(), b4.stride(0), b4.stride(1), w, h, res.data_ptr(), _capi.stream_on(a)))
    return res


def mokjiThreshold(cooc, minEdgeMagnitude=20):
    """Step 6 on the host (no device): the threshold of a 256 x 256 matrix of counts [n][m], -1 where no pair has n - m >= M."""
    m = np.ascontiguousarray(cooc, np.uint32)
    if m.shape != (256, 256):
        raise TypeError("expected a 256 x 256 matrix")
    t = C.c_int(0)
    _capi.check(_capi.lib().prl_hip_mokji_threshold(m.ctypes.data, int(minEdgeMagnitude), C.byref(t)))
    return t.value
