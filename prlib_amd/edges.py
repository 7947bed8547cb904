"""Host-side mirror of cv::pyrDown, cv::Canny, the edge map of prl::documentContour (src/border_detection/autoCrop.cpp:67-101)
and prl::resize (src/resize.cpp:29-62) over the C ABI (include/prl_hip.h, "pyramid, edge map, resize").

Pages are what prlib_amd._pages takes: a numpy H x W [x C] uint8 image goes through the *_host entry, a torch CUDA uint8 tensor
[N,] H x W [x C] is enqueued on the current stream.  cv::Canny and the two stages on their own take gray pages only (a
3-dimensional tensor is N x H x W).  document_edges_geometry, pyr_down_size and resize_pyramid_levels are host code and need no
device.

The border detector on top of the edge map ("document contour" in the header): find_contours, approx_poly_closed, document_quad
and document_quad_finish are the host search piece by piece (numpy maps, no device); document_contour is prl::documentContour on
device pages or one host image, auto_crop is prl::autoCrop: the contour, its corners truncated to int, prl::warpCrop.
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


def find_contours(edge_map):
    """cv::findContours(map, RETR_CCOMP, CHAIN_APPROX_SIMPLE) on an H x W uint8 numpy map -> [(K x 2 int32 points, is_hole)] in
    OpenCV's order.  Host code."""
    m = _pages.host_image(edge_map, gray_only=True)
    h, w = m.shape[:2]
    L = _capi.lib()
    npts, ncs = C.c_int(0), C.c_int(0)
    _capi.check(L.prl_hip_find_contours(m.ctypes.data, m.strides[0], w, h, None, 0, None, 0, C.byref(npts), C.byref(ncs)))
    pts = np.zeros((max(npts.value, 1), 2), np.int32)
    cs = np.zeros((max(ncs.value, 1), 2), np.int32)
    _capi.check(L.prl_hip_find_contours(m.ctypes.data, m.strides[0], w, h, pts.ctypes.data, npts.value, cs.ctypes.data, ncs.value,
                                        C.byref(npts), C.byref(ncs)))
    out, at = [], 0
    for k in range(ncs.value):
        out.append((pts[at:at + cs[k, 0]].copy(), bool(cs[k, 1])))
        at += int(cs[k, 0])
    return out


def approx_poly_closed(points, epsilon: float):
    """cv::approxPolyDP(points, epsilon, closed=True) on integer points -> K x 2 int32.  Host code."""
    p = np.ascontiguousarray(np.asarray(points, dtype=np.int32).reshape(-1, 2))
    out = np.zeros((max(len(p), 1), 2), np.int32)
    n = C.c_int(0)
    _capi.check(_capi.lib().prl_hip_approx_poly_closed(p.ctypes.data, len(p), float(epsilon), out.ctypes.data, C.byref(n)))
    return out[:n.value].copy()


def document_quad(edge_map):
    """findDocumentContour on an H x W uint8 numpy map: 4 x 2 int32 corners in the polygon's own order, or None.  Host code."""
    m = _pages.host_image(edge_map, gray_only=True)
    h, w = m.shape[:2]
    quad, found = np.zeros(8, np.int32), C.c_int(0)
    _capi.check(_capi.lib().prl_hip_document_quad(m.ctypes.data, m.strides[0], w, h, quad.ctypes.data, C.byref(found)))
    return quad.reshape(4, 2) if found.value else None


def document_quad_finish(quad, map_size, src_size):
    """scaleContour from map_size = (w, h) to src_size, then cropVerticesOrdering -> 4 x 2 float32.  Host code."""
    q = np.ascontiguousarray(np.asarray(quad, dtype=np.int32).reshape(8))
    out = np.zeros(8, np.float32)
    _capi.check(_capi.lib().prl_hip_document_quad_finish(q.ctypes.data, int(map_size[0]), int(map_size[1]), int(src_size[0]),
                                                         int(src_size[1]), out.ctypes.data))
    return out.reshape(4, 2)


def document_contour(pages):
    """prl::documentContour(page, -1, -1, contour) per page -> (quads N x 4 x 2 float32, found N bool, tries N int32); for one
    page (a numpy image or a tensor without a page axis) the three without the N."""
    L = _capi.lib()
    return _pages.quad_per_page(pages, L.prl_hip_document_contour_host, L.prl_hip_document_contour_batch_device, np.float32)


def auto_crop(pages, return_contour: bool = False):
    """prl::autoCrop per page of an N x H x W [x C] tensor -> list of tensors, None for a page without a quad [, the
    document_contour result].  The corners are truncated to int as the reference does; the destinations are sized with
    warp_crop_size."""
    from . import warp

    t4, chan, batch = _pages.pages4(pages)
    if not batch:
        raise TypeError("expected pages N x H x W [x C]")
    quads, found, tries = document_contour(pages)
    out = [None] * t4.shape[0]
    idx = [i for i in range(t4.shape[0]) if found[i]]
    if idx:
        import torch

        q = quads[idx].astype(np.int32).reshape(-1, 8)   # (int)float: towards zero
        src = pages if len(idx) == t4.shape[0] else pages[torch.as_tensor(idx, device=pages.device)]
        for i, crop in zip(idx, warp.warp_crop(src, q)):
            out[i] = crop
    return (out, (quads, found, tries)) if return_contour else out
