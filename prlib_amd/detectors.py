"""The focus measures of blur detection (focus.hip) over the C ABI: LAPM, LAPV, TENG and GLVN of src/detectors/blurDetection.cpp:32-83
from six integer sums per page and channel, taken in one read-only pass (the arithmetic is stated in include/prl_hip.h).

    bool prl::isBlurred(const cv::Mat&)                                        (src/detectors/blurDetection.h:35, .cpp:85-89)
        returns false without looking at the image and calls none of the four measures; they are what this module offers.

numpy H x W [x C] uint8 goes through the library's host entry; torch CUDA uint8 [N,] H x W [x C] is enqueued on the current
stream (a 3-dimensional tensor is H x W x C when its last dimension is at most 4, else N x H x W: the rule of _pages.py).  1, 3 or
4 channels; pages and rows may be strided, pixels and channels must be dense.  The results carry a channel axis exactly when the
input has one.  Errors are PrlError with the C status.
"""
from __future__ import annotations

import numpy as np

from . import _capi, _pages

SUM_P, SUM_P2, SUM_LAP, SUM_LAP2, SUM_LAPM4, SUM_TENG = range(6)
LAPM, LAPV, TENG, GLVN = range(4)


def focusSums(pages, tengKernelSize=3, out=None):
    """The six sums (SUM_P ... SUM_TENG) of every page and channel: a torch int64 tensor [N,] [C x] 6 on the input's device;
    nothing is synchronised.  `out` (int64, contiguous) is overwritten."""
    import torch

    L = _capi.lib()
    t4, chan, batch = _pages.pages4(pages)
    n, h, w, c = t4.shape
    oshape = ((n,) if batch else ()) + ((c,) if chan else ()) + (6,)
    res = torch.empty(oshape, dtype=torch.int64, device=pages.device) if out is None else out
    if not isinstance(res, torch.Tensor) or tuple(res.shape) != oshape or res.dtype != torch.int64 or res.device != pages.device \
            or not res.is_contiguous():
        raise TypeError("out must be a contiguous int64 tensor [N,] [C x] 6 on the input's device")
    _capi.check(L.prl_hip_focus_sums_batch_device(n, c, int(tengKernelSize), t4.data_ptr(), t4.stride(0), t4.stride(1), w, h,
                                                  res.data_ptr(), _capi.stream_on(pages)))
    return res


def focusFromSums(sums, width, height):
    """The four measures (LAPM, LAPV, TENG, GLVN) of every row of six sums, on the host (no device): float64 [...] x 4."""
    s = np.ascontiguousarray(sums, np.int64)
    if s.ndim < 1 or s.shape[-1] != 6:
        raise TypeError("expected int64 sums [...] x 6")
    res = np.empty(s.shape[:-1] + (4,), np.float64)
    L = _capi.lib()
    flat_s, flat_r = s.reshape(-1, 6), res.reshape(-1, 4)
    for i in range(flat_s.shape[0]):
        _capi.check(L.prl_hip_focus_from_sums(flat_s[i].ctypes.data, int(width), int(height), flat_r[i].ctypes.data))
    return res


def focusMeasures(pages, tengKernelSize=3):
    """LAPM, LAPV, TENG, GLVN of every page and channel: a numpy float64 array [N,] [C x] 4.  A numpy image goes through the host
    entry.  For a tensor the sums are taken on the device and copied to the host, which SYNCHRONISES the current stream; the
    measures follow there (prl_hip_focus_from_sums)."""
    if isinstance(pages, np.ndarray):
        img = _pages.host_image(pages)
        h, w, c = img.shape
        res = np.empty((c, 4), np.float64)
        _capi.check(_capi.lib().prl_hip_focus_measures_host(c, int(tengKernelSize), img.ctypes.data, img.strides[0], w, h,
                                                            res.ctypes.data, None))
        return res if pages.ndim == 3 else res[0]
    sums = focusSums(pages, tengKernelSize)
    h, w = _pages.pages4(pages)[0].shape[1:3]
    return focusFromSums(sums.cpu().numpy(), w, h)
