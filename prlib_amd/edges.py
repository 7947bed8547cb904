"""Host-side mirror of cv::pyrDown, cv::Canny, the edge map of prl::documentContour (src/border_detection/autoCrop.cpp:67-101)
and prl::resize (src/resize.cpp:29-62) over the C ABI (include/prl_hip.h, "pyramid, edge map, resize").

Pages are what prlib_amd._pages takes: a numpy H x W [x C] uint8 image goes through the *_host entry, a torch CUDA uint8 tensor
[N,] H x W [x C] is enqueued on the current stream.  cv::Canny and the two stages on their own take gray pages only (a
3-dimensional tensor is N x H x W).  document_edges_geometry, pyr_down_size and resize_pyramid_levels are host code and need no
device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi, _pages


def _three_ints(fn, *args):
    a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
    _capi.check(fn(*args, C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


def pyr_down_size(width: int, height: int, levels: int = 1):
    """(W, H) after `levels` steps of cv::pyrDown."""
    w, h = C.c_int(0), C.c_int(0)
    _capi.check(_capi.lib().prl_hip_pyr_down_size(int(width), int(height), int(levels), C.byref(w), C.byref(h)))
    return w.value, h.value


def document_edges_geometry(width: int, height: int):
    """(levels, W, H): the pyramid levels prl::documentContour takes and the size of its edge map."""
    return _three_ints(_capi.lib().prl_hip_document_edges_geometry, int(width), int(height))


def resize_pyramid_levels(width: int, height: int, max_size: int):
    """(levels, W, H) of prl::resize's pyramid path."""
    return _three_ints(_capi.lib().prl_hip_resize_pyramid_levels, int(width), int(height), int(max_size))


def _resized(pages, oc_of, size_of, host_call, device_call, out, drop_channel=False):
    """A stage whose result is size_of(w, h) = (ow, oh) pixels of oc_of(c) channels ([N,] H x W with drop_channel); the calls get
    the _pages arguments."""
    if isinstance(pages, np.ndarray):
        img = _pages.host_image(pages)
        h, w, c = img.shape
        ow, oh = size_of(w, h)
        oc = oc_of(c)
        oshape = (oh, ow) if pages.ndim == 2 or drop_channel else (oh, ow, oc)
        res = np.empty(oshape, np.uint8) if out is None else out
        if not isinstance(res, np.ndarray) or res.shape != oshape or res.dtype != np.uint8 or not res.flags.c_contiguous:
            raise TypeError("out must be a C-contiguous uint8 array of the result's shape")
        _capi.check(host_call(c, img.ctypes.data, img.strides[0], w, h, res.ctypes.data, max(ow * oc, 1)))
        return res
    import torch

    t4, chan, batch = _pages.pages4(pages)
    n, h, w, c = t4.shape
    ow, oh = size_of(w, h)
    oc = oc_of(c)
    chan = chan and not drop_channel
    oshape = ((n,) if batch else ()) + (oh, ow) + ((oc,) if chan else ())
    res = torch.empty(oshape, dtype=torch.uint8, device=pages.device) if out is None else out
    if not isinstance(res, torch.Tensor) or tuple(res.shape) != oshape or res.dtype != torch.uint8 or res.device != pages.device:
        raise TypeError("out must be a uint8 tensor of the result's shape on the input's device")
    r4 = res if batch else res[None]
    r4 = r4 if chan else r4[:, :, :, None]
    if r4.stride(3) != 1 and oc > 1 or r4.stride(2) != oc and (chan or ow > 1):
        raise TypeError("out must have dense pixels and channels")
    _capi.check(device_call(n, c, t4.data_ptr(), t4.stride(0), t4.stride(1), w, h, r4.data_ptr(), r4.stride(0), r4.stride(1),
                            _capi.stream_on(pages)))
    return res


def pyr_down(pages, levels: int = 1, out=None):
    """cv::pyrDown (BORDER_REFLECT_101) applied `levels` times; 1..4 channels."""
    L = _capi.lib()
    levels = int(levels)
    return _resized(pages, _pages.same, lambda w, h: pyr_down_size(w, h, levels),
                    lambda c, *a: L.prl_hip_pyr_down_host(c, levels, *a), lambda n, c, *a: L.prl_hip_pyr_down_batch_device(n, c, levels, *a), out)


def canny_classes(pages, threshold1: float, threshold2: float, out=None):
    """Stage 1 of cv::Canny: OpenCV's map codes per pixel (2 = edge, 0 = candidate, 1 = neither).  Device tensors only."""
    L = _capi.lib()
    t1, t2 = float(threshold1), float(threshold2)
    return _pages.run(pages, _pages.same, None, lambda n, c, *a: L.prl_hip_canny_classes_batch_device(n, c, t1, t2, *a), out, gray_only=True)


def edge_link(classes, out=None, return_passes: bool = False):
    """Stage 2 of cv::Canny on a byte class map -> 0 / 255 [, the linking passes every page took part in].  Device tensors only."""
    L = _capi.lib()
    passes = []

    def call(n, c, s, sps, ss, w, h, d, dps, ds, stream):
        p = np.zeros(max(n, 1), np.int32)
        passes.append(p[:n])
        return L.prl_hip_edge_link_batch_device(n, s, sps, ss, w, h, d, dps, ds, p.ctypes.data, stream)

    res = _pages.run(classes, _pages.same, None, call, out, gray_only=True)
    return (res, passes[0]) if return_passes else res


def canny(pages, threshold1: float, threshold2: float, out=None):
    """cv::Canny(page, threshold1, threshold2) with apertureSize 3 and the L1 magnitude, gray pages."""
    L = _capi.lib()
    t1, t2 = float(threshold1), float(threshold2)
    return _pages.run(pages, _pages.same, lambda c, *a: L.prl_hip_canny_host(c, t1, t2, *a),
                      lambda n, c, *a: L.prl_hip_canny_batch_device(n, c, t1, t2, *a), out, gray_only=True)


def document_edges(pages, out=None):
    """The edge map prl::documentContour searches, per page: (maps, channels) with the maps [N,] H' x W' at the size of
    document_edges_geometry and `channels` the channel every map was made from (numpy int32; an int for one page)."""
    L = _capi.lib()
    chosen = []

    def host(c, *a):
        ch = np.zeros(1, np.int32)
        chosen.append(ch)
        return L.prl_hip_document_edges_host(c, *a, ch.ctypes.data)

    def device(n, c, *a):
        ch = np.zeros(max(n, 1), np.int32)
        chosen.append(ch[:n])
        return L.prl_hip_document_edges_batch_device(n, c, *a[:-1], ch.ctypes.data, a[-1])

    res = _resized(pages, lambda c: 1, lambda w, h: document_edges_geometry(w, h)[1:], host, device, out, drop_channel=True)
    single = isinstance(pages, np.ndarray) or not _pages.pages4(pages)[2]
    return res, (int(chosen[0][0]) if single else chosen[0])


def resize(pages, scaleX: int, scaleY: int, maxSize: int, out=None):
    """prl::resize(src, dst, scaleX, scaleY, maxSize): cv::resize(INTER_AREA) by the integer factors when both are positive, else
    cv::pyrDown while the long side exceeds maxSize (a copy when it does not)."""
    L = _capi.lib()
    sx, sy = int(scaleX), int(scaleY)
    if sx > 0 and sy > 0:
        return _resized(pages, _pages.same, lambda w, h: (w * sx, h * sy), lambda c, *a: L.prl_hip_resize_replicate_host(c, sx, sy, *a),
                        lambda n, c, *a: L.prl_hip_resize_replicate_batch_device(n, c, sx, sy, *a), out)
    first = pages.shape[:2] if isinstance(pages, np.ndarray) else _pages.pages4(pages)[0].shape[1:3]
    levels = resize_pyramid_levels(int(first[1]), int(first[0]), int(maxSize))[0]
    if levels == 0:   # dst = src.clone()
        return _resized(pages, _pages.same, lambda w, h: (w, h), lambda c, *a: L.prl_hip_resize_replicate_host(c, 1, 1, *a),
                        lambda n, c, *a: L.prl_hip_resize_replicate_batch_device(n, c, 1, 1, *a), out)
    return pyr_down(pages, levels, out)
