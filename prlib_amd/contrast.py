"""Contrast enhancement (clahe.hip) over the C ABI: cv::CLAHE::apply and cv::equalizeHist on 8-bit pages, every channel on its own,
and the reference's helper that runs one after the other; the arithmetic is stated in include/prl_hip.h ("contrast").

    void EnhanceLocalContrastByCLAHE(cv::Mat&, cv::Mat&, double CLAHEClipLimit, bool equalizeHistFlag)   (src/imageLibCommon.h:151)

numpy H x W [x C] uint8 goes through the library's host entries (claheLuts takes device tensors only); torch CUDA uint8 [N,] H x W
[x C] is enqueued on the current stream (a 3-dimensional tensor is H x W x C when its last dimension is at most 4, else N x H x W:
the rule of _pages.py).  1 to 4 channels; pages and rows may be strided, pixels and channels must be dense.  The result has the
input's shape; `out` receives it and may be the input.  Errors are PrlError with the C status.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _capi, _pages

MAX_TILES = 64


def clahe(pages, clip_limit=40.0, tiles=(8, 8), out=None):
    """cv::createCLAHE(clip_limit, tiles = (tilesX, tilesY))->apply on every channel; clip_limit <= 0: no clipping"""
    L = _capi.lib()
    cl, tx, ty = float(clip_limit), int(tiles[0]), int(tiles[1])
    return _pages.run(pages, _pages.same,
                      lambda c, *a: L.prl_hip_clahe_host(c, cl, tx, ty, *a),
                      lambda n, c, *a: L.prl_hip_clahe_batch_device(n, c, cl, tx, ty, *a), out)


def claheLuts(pages, clip_limit=40.0, tiles=(8, 8), out=None):
    """The tile tables cv::CLAHE blends: a uint8 tensor [N,] C x tilesY x tilesX x 256 on the input's device; `out` (uint8,
    contiguous) is overwritten."""
    import torch

    t4, _, batch = _pages.pages4(pages)
    n, h, w, c = t4.shape
    tx, ty = int(tiles[0]), int(tiles[1])
    oshape = ((n,) if batch else ()) + (c, max(ty, 0), max(tx, 0), 256)
    res = torch.empty(oshape, dtype=torch.uint8, device=pages.device) if out is None else out
    if not isinstance(res, torch.Tensor) or tuple(res.shape) != oshape or res.dtype != torch.uint8 or res.device != pages.device \
            or not res.is_contiguous():
        raise TypeError("out must be a contiguous uint8 tensor [N,] C x tilesY x tilesX x 256 on the input's device")
    _capi.check(_capi.lib().prl_hip_clahe_luts_batch_device(n, c, float(clip_limit), tx, ty, t4.data_ptr(), t4.stride(0), t4.stride(1),
                                                            w, h, res.data_ptr(), _capi.stream_on(pages)))
    return res


def equalizeHist(pages, out=None):
    """cv::equalizeHist on every channel"""
    L = _capi.lib()
    return _pages.run(pages, _pages.same, L.prl_hip_equalize_hist_host, L.prl_hip_equalize_hist_batch_device, out)


def enhanceLocalContrast(pages, clip_limit, equalize=False, out=None):
    """EnhanceLocalContrastByCLAHE: CLAHE on the 8 x 8 grid on every channel, then, with `equalize`, cv::equalizeHist of the result"""
    L = _capi.lib()
    cl, eq = float(clip_limit), int(bool(equalize))
    return _pages.run(pages, _pages.same,
                      lambda c, *a: L.prl_hip_enhance_local_contrast_host(c, cl, eq, *a),
                      lambda n, c, *a: L.prl_hip_enhance_local_contrast_batch_device(n, c, cl, eq, *a), out)


def claheGeometry(width, height, tiles=(8, 8), clip_limit=40.0):
    """(tile_w, tile_h, ext_w, ext_h, clip) of a width x height page, on the host (no device)"""
    v = [ctypes.c_int(0) for _ in range(5)]
    _capi.check(_capi.lib().prl_hip_clahe_geometry(int(width), int(height), int(tiles[0]), int(tiles[1]), float(clip_limit),
                                                   *[ctypes.byref(x) for x in v]))
    return tuple(x.value for x in v)


def claheTileLut(hist, clip, tile_area=None):
    """one tile's table from its 256 bins, on the host (no device); tile_area: the sum of the bins"""
    h = np.ascontiguousarray(hist, np.uint32)
    if h.shape != (256,):
        raise TypeError("expected 256 bins")
    lut = np.empty(256, np.uint8)
    area = int(h.sum(dtype=np.int64)) if tile_area is None else int(tile_area)
    _capi.check(_capi.lib().prl_hip_clahe_tile_lut(h.ctypes.data, int(clip), area, lut.ctypes.data))
    return lut


def equalizeHistLut(hist):
    """cv::equalizeHist's table from one channel's 256 bins, on the host (no device)"""
    h = np.ascontiguousarray(hist, np.uint32)
    if h.shape != (256,):
        raise TypeError("expected 256 bins")
    lut = np.empty(256, np.uint8)
    _capi.check(_capi.lib().prl_hip_equalize_hist_lut(h.ctypes.data, lut.ctypes.data))
    return lut
