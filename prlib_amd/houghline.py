"""Host-side mirror of cv::HoughLines(rho 1, theta pi / 180) and prl::findHoughLineContour (src/border_detection/houghLine.cpp)
over the C ABI (include/prl_hip.h, "Hough lines").

Maps and pages are what prlib_amd._pages takes: a numpy H x W [x C] uint8 image goes through the *_host entry, a torch CUDA uint8
tensor [N,] H x W [x C] is enqueued on the current stream.  hough_lines and hough_accumulator take 8UC1 maps only (a 3-dimensional
tensor is N x H x W).  hough_lines_geometry and hough_line_quad are host code and need no device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi, _pages


def hough_lines_geometry(width: int, height: int):
    """(numangle, numrho) of cv::HoughLines(rho 1, theta pi / 180) on a width x height map."""
    a, r = C.c_int(0), C.c_int(0)
    _capi.check(_capi.lib().prl_hip_hough_lines_geometry(int(width), int(height), C.byref(a), C.byref(r)))
    return a.value, r.value


def hough_accumulator(maps, out=None):
    """The framed accumulator of the standard transform per map: int32 [N,] (numangle + 2) x (numrho + 2).  Device tensors only;
    `out`: an int32 tensor of that shape whose pages may be strided.  Enqueues only."""
    import torch

    t4, _chan, batch = _pages.pages4(maps, gray_only=True)
    n, h, w, _c = t4.shape
    na, nr = hough_lines_geometry(w, h)
    shape = ((n,) if batch else ()) + (na + 2, nr + 2)
    res = torch.empty(shape, dtype=torch.int32, device=maps.device) if out is None else out
    if not isinstance(res, torch.Tensor) or tuple(res.shape) != shape or res.dtype != torch.int32 or res.device != maps.device:
        raise TypeError("out must be an int32 tensor of the accumulators' shape on the input's device")
    r3 = res if batch else res[None]
    if r3.stride(2) != 1 or r3.stride(1) != nr + 2:
        raise TypeError("out must have dense accumulator pages")
    _capi.check(_capi.lib().prl_hip_hough_accumulator_batch_device(n, t4.data_ptr(), t4.stride(0), t4.stride(1), w, h, r3.data_ptr(),
                                                                   r3.stride(0) * 4, _capi.stream_on(maps)))
    return res


def hough_lines(maps, threshold: int, max_lines=None, return_counts: bool = False):
    """cv::HoughLines(map, 1, pi / 180, threshold) -> per map a K x 2 float32 array of (rho, theta) in OpenCV's order: a list for a
    batch, the array for one map (a numpy image or a tensor without a page axis).  max_lines: room per map; None asks for the
    counts first and then for all lines.  return_counts: also the number of lines found per map (an int for one map), which
    exceeds the rows of an array cut at max_lines."""
    L = _capi.lib()
    thr = int(threshold)
    if isinstance(maps, np.ndarray):
        m = _pages.host_image(maps, gray_only=True)
        h, w = m.shape[:2]
        n, single = 1, True

        def call(buf, cap, cnt):
            return L.prl_hip_hough_lines_host(m.ctypes.data, m.strides[0], w, h, thr, buf, cap, cnt)
    else:
        t4, _chan, batch = _pages.pages4(maps, gray_only=True)
        n, h, w, _c = t4.shape
        single = not batch

        def call(buf, cap, cnt):
            return L.prl_hip_hough_lines_batch_device(n, t4.data_ptr(), t4.stride(0), t4.stride(1), w, h, thr, buf, cap, cnt,
                                                      _capi.stream_on(maps))
    counts = np.zeros(max(n, 1), np.int32)
    if max_lines is None:
        _capi.check(call(None, 0, counts.ctypes.data))
        cap = int(counts[:n].max()) if n else 0
    else:
        cap = int(max_lines)
    lines = np.zeros((max(n, 1), max(cap, 1), 2), np.float32)
    if cap > 0 or max_lines is not None:
        _capi.check(call(lines.ctypes.data if cap > 0 else None, cap, counts.ctypes.data))
    out = [lines[i, :min(int(counts[i]), cap)].copy() for i in range(n)]
    if single:
        return (out[0], int(counts[0])) if return_counts else out[0]
    return (out, counts[:n].copy()) if return_counts else out


def hough_edges(pages, out=None):
    """The edge map of prl::findHoughLineContour: medianBlur(3) x 3, medianBlur(5) x 3, cv::Canny(25, 50) on the page's own 1, 3
    or 4 channels -> 0 / 255 maps [N,] H x W."""
    L = _capi.lib()
    return _pages.run(pages, _pages.same, L.prl_hip_hough_edges_host, L.prl_hip_hough_edges_batch_device, out, drop_channel=True)


def hough_line_quad(lines, width: int, height: int):
    """The line filter and the quad search on K x 2 (rho, theta) lines in cv::HoughLines' order, for a map of width x height:
    4 x 2 int32 corners, or None.  Host code."""
    ln = np.ascontiguousarray(np.asarray(lines, dtype=np.float32).reshape(-1, 2))
    quad, found = np.zeros(8, np.int32), C.c_int(0)
    _capi.check(_capi.lib().prl_hip_hough_line_quad(ln.ctypes.data if len(ln) else None, len(ln), int(width), int(height), quad.ctypes.data,
                                                    C.byref(found)))
    return quad.reshape(4, 2) if found.value else None


def hough_line_contour(pages):
    """prl::findHoughLineContour per page -> (quads N x 4 x 2 int32, found N bool, lines N int32: what cv::HoughLines found); for
    one page (a numpy image or a tensor without a page axis) the three without the N."""
    L = _capi.lib()
    return _pages.quad_per_page(pages, L.prl_hip_hough_line_contour_host, L.prl_hip_hough_line_contour_batch_device, np.int32)
