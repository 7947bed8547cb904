"""Host-side mirror of prl::warpCrop (src/warp.cpp:32-102, src/warp.h:49-73) and of the cv::warpPerspective(INTER_LINEAR) it
ends in, over the C ABI (include/prl_hip.h, "perspective crop").

    void prl::warpCrop(const cv::Mat& inputImage, cv::Mat& outputImage, x0, y0, x1, y1, x2, y2, x3, y3,
                       double ratio = -1.0, int borderMode = cv::BORDER_CONSTANT, const cv::Scalar& borderValue = cv::Scalar())

Pages are torch CUDA uint8 tensors N x H x W x C (C in 1..4; a 3-d tensor is N x H x W gray) with dense pixels; rows and pages
may be strided.  Every result has its own size, so the functions return a list of views into one N x maxH x maxW x C buffer.
warp_crop_size and perspective_transform are host code and need no device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi

BORDER_CONSTANT, BORDER_REPLICATE = 0, 1


def warp_crop_size(quad, ratio: float = -1.0):
    """(W, H) of prl::warpCrop's result for the corners x0, y0, ..., x3, y3 (warp.cpp:42-53)."""
    q = np.ascontiguousarray(np.asarray(quad, dtype=np.int32).reshape(8))
    ow, oh = C.c_int(0), C.c_int(0)
    _capi.check(_capi.lib().prl_hip_warp_crop_size(q.ctypes.data, float(ratio), C.byref(ow), C.byref(oh)))
    return ow.value, oh.value


def perspective_transform(src_xy, dst_xy) -> np.ndarray:
    """cv::getPerspectiveTransform(src, dst) for four (x, y) pairs each way -> 3 x 3 float64."""
    s = np.ascontiguousarray(np.asarray(src_xy, dtype=np.float64).reshape(8))
    d = np.ascontiguousarray(np.asarray(dst_xy, dtype=np.float64).reshape(8))
    m = np.zeros(9, dtype=np.float64)
    _capi.check(_capi.lib().prl_hip_perspective_transform(s.ctypes.data, d.ctypes.data, m.ctypes.data))
    return m.reshape(3, 3)


def _pages4(t):
    import torch

    if t.dtype != torch.uint8 or not t.is_cuda or t.dim() not in (3, 4):
        raise TypeError("expected a uint8 CUDA tensor N x H x W [x C]")
    t4 = t if t.dim() == 4 else t[:, :, :, None]
    if t4.shape[3] > 1 and t4.stride(3) != 1 or t4.stride(2) != t4.shape[3]:
        raise TypeError("the pixels of a row must be dense (rows and pages may be strided)")
    return t4


def _border(value):
    v = np.zeros(4, dtype=np.float64)
    a = np.atleast_1d(np.asarray(value, dtype=np.float64))
    v[: min(4, a.size)] = a[:4]
    return v


def _views(buf, sizes, gray):
    outs = [buf[i, :oh, :ow] for i, (ow, oh) in enumerate(sizes)]
    return [o[:, :, 0] for o in outs] if gray else outs


def _destination(t4, sizes, out):
    import torch

    n, c = t4.shape[0], t4.shape[3]
    mw, mh = max(s[0] for s in sizes), max(s[1] for s in sizes)
    if out is None:
        return torch.empty((n, mh, mw, c), dtype=torch.uint8, device=t4.device)
    o4 = _pages4(out)
    if o4.shape[0] != n or o4.shape[3] != c or o4.shape[1] < mh or o4.shape[2] < mw or o4.device != t4.device:
        raise ValueError("`out` needs N pages of the input's channels with room for the largest result")
    return o4


def warp_perspective(pages, matrices, sizes, inverse_map: bool = False, border_mode: int = BORDER_CONSTANT, border_value=0, out=None):
    """cv::warpPerspective(page_i, M_i, Size(*sizes[i]), INTER_LINEAR [| WARP_INVERSE_MAP], border_mode, border_value) ->
    list of tensors (views of one buffer, or of `out`).  matrices: 3 x 3 or N x 3 x 3; sizes: (ow, oh) or N of them."""
    t4 = _pages4(pages)
    n, h, w, c = t4.shape
    m = np.ascontiguousarray(np.broadcast_to(np.asarray(matrices, dtype=np.float64).reshape(-1, 9), (n, 9)))
    wh = np.ascontiguousarray(np.broadcast_to(np.asarray(sizes, dtype=np.int32).reshape(-1, 2), (n, 2)))
    if n == 0:
        return []
    buf = _destination(t4, [(max(1, int(a)), max(1, int(b))) for a, b in wh], out)
    bv = _border(border_value)
    L = _capi.lib()
    stream = _capi.stream_on(t4)
    _capi.check(L.prl_hip_warp_perspective_batch_device(n, c, m.ctypes.data, 1 if inverse_map else 0, t4.data_ptr(), t4.stride(0),
                                                        t4.stride(1), w, h, buf.data_ptr(), buf.stride(0), buf.stride(1),
                                                        wh.ctypes.data, int(border_mode), bv.ctypes.data, stream))
    return _views(buf, [(int(a), int(b)) for a, b in wh], pages.dim() == 3)


def warp_crop(pages, quads, ratio: float = -1.0, border_mode: int = BORDER_CONSTANT, border_value=0, out=None):
    """prl::warpCrop per page -> list of tensors.  quads: 8 ints (x0, y0, ..., x3, y3: top left, top right, bottom right, bottom
    left) or N x 8."""
    t4 = _pages4(pages)
    n, h, w, c = t4.shape
    q = np.ascontiguousarray(np.broadcast_to(np.asarray(quads, dtype=np.int32).reshape(-1, 8), (n, 8)))
    if n == 0:
        return []
    sizes = [warp_crop_size(q[i], ratio) for i in range(n)]
    buf = _destination(t4, sizes, out)
    wh = np.zeros((n, 2), dtype=np.int32)
    bv = _border(border_value)
    L = _capi.lib()
    stream = _capi.stream_on(t4)
    _capi.check(L.prl_hip_warp_crop_batch_device(n, c, q.ctypes.data, float(ratio), t4.data_ptr(), t4.stride(0), t4.stride(1), w, h,
                                                 buf.data_ptr(), buf.stride(0), buf.stride(1), wh.ctypes.data, int(border_mode),
                                                 bv.ctypes.data, stream))
    return _views(buf, [(int(a), int(b)) for a, b in wh], pages.dim() == 3)


def warp_crop_host(image: np.ndarray, quad, ratio: float = -1.0, border_mode: int = BORDER_CONSTANT, border_value=0) -> np.ndarray:
    """prl::warpCrop on one host image (H x W or H x W x C uint8 numpy) through prl_hip_warp_crop_host."""
    img = image if image.ndim == 3 else image[:, :, None]
    if img.dtype != np.uint8 or (img.shape[2] > 1 and img.strides[2] != 1) or img.strides[1] != img.shape[2]:
        raise TypeError("expected a uint8 image with dense pixels")
    h, w, c = img.shape
    q = np.ascontiguousarray(np.asarray(quad, dtype=np.int32).reshape(8))
    ow, oh = warp_crop_size(q, ratio)
    out = np.empty((oh, ow, c), dtype=np.uint8)
    bv = _border(border_value)
    _capi.check(_capi.lib().prl_hip_warp_crop_host(c, q.ctypes.data, float(ratio), img.ctypes.data, img.strides[0], w, h,
                                                   out.ctypes.data, out.strides[0], int(border_mode), bv.ctypes.data))
    return out if image.ndim == 3 else out[:, :, 0]
