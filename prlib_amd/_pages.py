"""The page arguments of the stage modules (denoiseSaltPepper, the adaptive thresholds, morphology, removeLines, the tone
functions, Mokji): one place that turns an image into what the C entries take, and validates or allocates the result.

numpy H x W [x C] uint8 goes through a library's *_host entry:        call(c, src, src_step, w, h, dst, dst_step)
torch CUDA uint8 [N,] H x W [x C] is enqueued on the current stream:  call(n, c, src, src_page_stride, src_step, w, h,
                                                                           dst, dst_page_stride, dst_step, stream)
A 3-dimensional tensor is H x W x C when its last dimension is at most 4, else N x H x W.  Pages and rows may be strided;
pixels and channels must be dense (an input that is not is copied, an `out` that is not is refused).  The result has the
input's shape with oc_of(c) channels; `out` receives it and is returned.

    gray_only      numpy 2-D only, and a 3-dimensional tensor is always N x H x W (cv::adaptiveThreshold)
    drop_channel   the result is [N,] H x W whatever the input's channels (masks: removeLines, Mokji, the adaptive binarizers)
"""
from __future__ import annotations

import numpy as np

from . import _capi


def same(c):
    return c


def host_image(image, gray_only=False):
    """H x W [x C] uint8 numpy -> an H x W x C view (a copy where pixels are not dense or rows run backwards)"""
    if not isinstance(image, np.ndarray) or image.dtype != np.uint8 or image.ndim not in ((2,) if gray_only else (2, 3)):
        raise TypeError("expected an H x W%s uint8 array" % ("" if gray_only else " [x C]"))
    img = image if image.ndim == 3 else image[:, :, None]
    if img.strides[2] != 1 or img.strides[1] != img.shape[2] or img.strides[0] < 0:
        img = np.ascontiguousarray(img)
    return img


def pages4(t, gray_only=False):
    """[N,] H x W [x C] -> (N x H x W x C view with dense pixels, has a channel axis, has a page axis)"""
    import torch

    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_cuda or t.dim() not in ((2, 3) if gray_only else (2, 3, 4)):
        raise TypeError("expected a uint8 CUDA tensor [N,] H x W%s or a numpy uint8 array" % ("" if gray_only else " [x C]"))
    if t.dim() == 2:
        t4, chan, batch = t[None, :, :, None], False, False
    elif t.dim() == 3 and t.shape[-1] <= 4 and not gray_only:
        t4, chan, batch = t[None], True, False
    elif t.dim() == 3:
        t4, chan, batch = t[:, :, :, None], False, True
    else:
        t4, chan, batch = t, True, True
    c = t4.shape[3]
    if t4.stride(3) != 1 and c > 1 or t4.stride(2) != c:
        t4 = t4.contiguous()
    return t4, chan, batch


def _host(image, oc_of, call, out, gray_only, drop_channel):
    img = host_image(image, gray_only)
    h, w, c = img.shape
    oc = 1 if drop_channel else oc_of(c)
    oshape = (h, w) if drop_channel or image.ndim == 2 else (h, w, oc)
    res = np.empty(oshape, np.uint8) if out is None else out
    if not isinstance(res, np.ndarray) or res.shape != oshape or res.dtype != np.uint8 or not res.flags.c_contiguous:
        raise TypeError("out must be a C-contiguous uint8 array of the result's shape")
    _capi.check(call(c, img.ctypes.data, img.strides[0], w, h, res.ctypes.data, max(w * oc, 1)))
    return res


def _device(pages, oc_of, call, out, gray_only, drop_channel):
    import torch

    t4, chan, batch = pages4(pages, gray_only)
    n, h, w, c = t4.shape
    oc = 1 if drop_channel else oc_of(c)
    chan = chan and not drop_channel
    oshape = ((n,) if batch else ()) + (h, w) + ((oc,) if chan else ())
    res = torch.empty(oshape, dtype=torch.uint8, device=pages.device) if out is None else out
    if not isinstance(res, torch.Tensor) or tuple(res.shape) != oshape or res.dtype != torch.uint8 or res.device != pages.device:
        raise TypeError("out must be a uint8 tensor of the result's shape on the input's device")
    r4 = res if batch else res[None]
    r4 = r4 if chan else r4[:, :, :, None]
    if r4.stride(3) != 1 and oc > 1 or r4.stride(2) != oc and (chan or w > 1):
        raise TypeError("out must have dense pixels and channels")
    _capi.check(call(n, c, t4.data_ptr(), t4.stride(0), t4.stride(1), w, h, r4.data_ptr(), r4.stride(0), r4.stride(1),
                     _capi.stream_on(pages)))
    return res


def quad_per_page(pages, host_call, device_call, quad_dtype):
    """A border detector: (quads N x 4 x 2 of quad_dtype, found N bool, a third int32 per page); for one page (a numpy image or a
    tensor without a page axis) the three without the N.  The calls get the source's arguments as above, then the three results."""
    host = isinstance(pages, np.ndarray)
    img, batch = (host_image(pages)[None], False) if host else pages4(pages)[::2]
    n, h, w, c = img.shape
    quads, found, third = np.zeros((max(n, 1), 4, 2), quad_dtype), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    res = (quads.ctypes.data, found.ctypes.data, third.ctypes.data)
    if host:
        _capi.check(host_call(c, img.ctypes.data, img.strides[1], w, h, *res))
    else:
        _capi.check(device_call(n, c, img.data_ptr(), img.stride(0), img.stride(1), w, h, *res, _capi.stream_on(pages)))
    if not batch:
        return quads[0], bool(found[0]), int(third[0])
    return quads[:n], found[:n].astype(bool), third[:n]


def run(pages, oc_of, host_call, device_call, out=None, gray_only=False, drop_channel=False):
    """Dispatch on the kind of `pages`; host_call is None where a function takes device tensors only."""
    if isinstance(pages, np.ndarray) and host_call is not None:
        return _host(pages, oc_of, host_call, out, gray_only, drop_channel)
    return _device(pages, oc_of, device_call, out, gray_only, drop_channel)
