"""prl::removeLines (lines.hip) over the C ABI: strips ruled lines, table grids and form boxes from a page.

    void prl::removeLines(const cv::Mat& inputImage, cv::Mat& outputImage)      (src/removeLines.h:38, removeLines.cpp:30-76)
        gray = BGR2GRAY for 3 channels; bw = threshold(~gray, THRESH_BINARY | THRESH_OTSU); horizontal / vertical = erode then
        dilate of bw with a (cols / 50) x 1 / 1 x (rows / 50) rectangle; out = ~((bw - horizontal) - vertical), one channel

numpy H x W or H x W x 3 uint8 -> numpy H x W (through the library's host entry); torch CUDA uint8 [N,] H x W [x 3] -> torch
tensor without the channel axis on the same device, enqueued on the current stream (a 3-dimensional tensor is H x W x C when its
last dimension is at most 4, else N x H x W: the rule of morphology.py).  Pages and rows may be strided; pixels and channels must
be dense.  `out` receives the result (for 1-channel pages out may be pages: in place).  Errors are PrlError with the C status.
"""
from __future__ import annotations

import numpy as np

from . import _capi


def removeLines(pages, out=None):
    """prl::removeLines: 0 where a pixel is ink (Otsu on the inverted page) outside every long horizontal / vertical run, else 255."""
    L = _capi.lib()
    if isinstance(pages, np.ndarray):
        if pages.dtype != np.uint8 or pages.ndim not in (2, 3):
            raise TypeError("expected an H x W [x 3] uint8 array")
        img = pages if pages.ndim == 3 else pages[:, :, None]
        if img.strides[2] != 1 or img.strides[1] != img.shape[2] or img.strides[0] < 0:
            img = np.ascontiguousarray(img)
        h, w, c = img.shape
        res = np.empty((h, w), np.uint8) if out is None else out
        if not isinstance(res, np.ndarray) or res.shape != (h, w) or res.dtype != np.uint8 or not res.flags.c_contiguous:
            raise TypeError("out must be a C-contiguous H x W uint8 array")
        _capi.check(L.prl_hip_remove_lines_host(c, img.ctypes.data, img.strides[0], w, h, res.ctypes.data, res.strides[0]))
        return res
    import torch

    t = pages
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_cuda or t.dim() not in (2, 3, 4):
        raise TypeError("expected a uint8 CUDA tensor [N,] H x W [x 3] or a numpy uint8 array")
    if t.dim() == 2:
        t4, oshape = t[None, :, :, None], t.shape
    elif t.dim() == 3 and t.shape[-1] <= 4:
        t4, oshape = t[None], t.shape[:2]
    elif t.dim() == 3:
        t4, oshape = t[:, :, :, None], t.shape
    else:
        t4, oshape = t, t.shape[:3]
    n, h, w, c = t4.shape
    if t4.stride(3) != 1 and c > 1 or t4.stride(2) != c:
        t4 = t4.contiguous()
    res = torch.empty(oshape, dtype=torch.uint8, device=t.device) if out is None else out
    if not isinstance(res, torch.Tensor) or tuple(res.shape) != tuple(oshape) or res.dtype != torch.uint8 or res.device != t.device \
            or res.stride(-1) != 1:
        raise TypeError("out must be a uint8 tensor [N,] H x W on the input's device, pixels dense")
    r3 = res if res.dim() == 3 else res[None]
    _capi.check(L.prl_hip_set_device(t.device.index or 0))
    stream = torch.cuda.current_stream(t.device).cuda_stream
    _capi.check(L.prl_hip_remove_lines_batch_device(n, c, t4.data_ptr(), t4.stride(0), t4.stride(1), w, h, r3.data_ptr(), r3.stride(0),
                                                    r3.stride(1), stream))
    return res
