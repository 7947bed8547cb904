"""Tone operations (tone.hip) over the C ABI: point operations whose table depends on page statistics, and their two primitives.

    void prl::gammaCorrection(const cv::Mat&, cv::Mat&, const double k, const double gamma)     (src/balance/gammaCorrection.h:33)
    void prl::simpleWhiteBalance(const cv::Mat&, cv::Mat&, const double k)                      (src/balance/balanceSimpleWhite.h:33)
    void prl::grayWorldWhiteBalance(const cv::Mat&, cv::Mat&, const double pNorm, const bool withMax)
                                                                                                (src/balance/balanceGrayWorldWhite.h:33)
    void prl::cleanBackgroundToWhite(const cv::Mat&, cv::Mat&)                                  (src/cleanBackgroundToWhite.h:40)
    histogram(pages) -> [N,] C x 256 int64 / uint32 counts;  lut(pages, table) = cv::LUT

numpy H x W [x C] uint8 goes through the library's host entries (histogram and lut take device tensors only); torch CUDA uint8
[N,] H x W [x C] is enqueued on the current stream (a 3-dimensional tensor is H x W x C when its last dimension is at most 4, else
N x H x W: the rule of morphology.py).  Pages and rows may be strided; pixels and channels must be dense.  The result has the
input's shape, except that 4 channels come back as 3 from gammaCorrection and cleanBackgroundToWhite, as in the reference.  `out`
receives the result (it may be the input where the channel count stays).  grayWorldWhiteBalance with pNorm != 1 builds its tables
with the host's pow and synchronises the stream.  Errors are PrlError with the C status.
"""
from __future__ import annotations

import numpy as np

from . import _capi


def _host(pages, oc_of, call, out):
    if pages.dtype != np.uint8 or pages.ndim not in (2, 3):
        raise TypeError("expected an H x W [x C] uint8 array")
    img = pages if pages.ndim == 3 else pages[:, :, None]
    if img.strides[2] != 1 or img.strides[1] != img.shape[2] or img.strides[0] < 0:
        img = np.ascontiguousarray(img)
    h, w, c = img.shape
    oc = oc_of(c)
    oshape = (h, w) if pages.ndim == 2 else (h, w, oc)
    res = np.empty(oshape, np.uint8) if out is None else out
    if not isinstance(res, np.ndarray) or res.shape != oshape or res.dtype != np.uint8 or not res.flags.c_contiguous:
        raise TypeError("out must be a C-contiguous uint8 array of the result's shape")
    _capi.check(call(c, img.ctypes.data, img.strides[0], w, h, res.ctypes.data, w * oc))
    return res


def _pages4(t):
    """[N,] H x W [x C] -> (N x H x W x C view with dense pixels, has a channel axis, has a page axis)"""
    import torch

    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_cuda or t.dim() not in (2, 3, 4):
        raise TypeError("expected a uint8 CUDA tensor [N,] H x W [x C] or a numpy uint8 array")
    if t.dim() == 2:
        t4, chan, batch = t[None, :, :, None], False, False
    elif t.dim() == 3 and t.shape[-1] <= 4:
        t4, chan, batch = t[None], True, False
    elif t.dim() == 3:
        t4, chan, batch = t[:, :, :, None], False, True
    else:
        t4, chan, batch = t, True, True
    c = t4.shape[3]
    if t4.stride(3) != 1 and c > 1 or t4.stride(2) != c:
        t4 = t4.contiguous()
    return t4, chan, batch


def _device(pages, oc_of, call, out):
    import torch

    t4, chan, batch = _pages4(pages)
    n, h, w, c = t4.shape
    oc = oc_of(c)
    oshape = ((n,) if batch else ()) + (h, w) + ((oc,) if chan else ())
    res = torch.empty(oshape, dtype=torch.uint8, device=pages.device) if out is None else out
    if not isinstance(res, torch.Tensor) or tuple(res.shape) != oshape or res.dtype != torch.uint8 or res.device != pages.device:
        raise TypeError("out must be a uint8 tensor of the result's shape on the input's device")
    r4 = res if batch else res[None]
    r4 = r4 if chan else r4[:, :, :, None]
    if r4.stride(3) != 1 and oc > 1 or r4.stride(2) != oc:
        raise TypeError("out must have dense pixels and channels")
    L = _capi.lib()
    _capi.check(L.prl_hip_set_device(pages.device.index or 0))
    stream = torch.cuda.current_stream(pages.device).cuda_stream
    _capi.check(call(n, c, t4.data_ptr(), t4.stride(0), t4.stride(1), w, h, r4.data_ptr(), r4.stride(0), r4.stride(1), stream))
    return res


def _same(c):
    return c


def _three(c):
    if c != 3:
        raise _capi.PrlError(_capi.PRL_ERR_BAD_CHANNELS, _capi.lib().prl_hip_strerror(_capi.PRL_ERR_BAD_CHANNELS).decode())
    return 3


def gammaCorrection(pages, k, gamma, out=None):
    """prl::gammaCorrection: sat_u8(pow(v / 255, gamma) * 255), then times k in float32 unless |k - 1| <= 1e-7; 4 channels come back
    as 3 with only the k step applied (the reference's switch has no case for them)."""
    L = _capi.lib()
    k, gamma = float(k), float(gamma)
    oc_of = lambda c: 3 if c == 4 else c  # noqa: E731
    if isinstance(pages, np.ndarray):
        return _host(pages, oc_of, lambda c, *a: L.prl_hip_gamma_correction_host(c, k, gamma, *a), out)
    return _device(pages, oc_of, lambda n, c, *a: L.prl_hip_gamma_correction_batch_device(n, c, k, gamma, *a), out)


def simpleWhiteBalance(pages, k, out=None):
    """prl::simpleWhiteBalance on 3-channel pages: per channel, stretch [vmin, vmax] (the k and 1 - k quantiles) to [0, 255]."""
    L = _capi.lib()
    k = float(k)
    if isinstance(pages, np.ndarray):
        return _host(pages, _three, lambda c, *a: L.prl_hip_simple_white_balance_host(k, *a), out)
    return _device(pages, _three, lambda n, c, *a: L.prl_hip_simple_white_balance_batch_device(n, k, *a), out)


def grayWorldWhiteBalance(pages, pNorm, withMax, out=None):
    """prl::grayWorldWhiteBalance on 3-channel pages: every channel scaled so that its p-norm mean meets the mean (or, withMax, the
    largest) of the three.  pNorm == 1 stays on the device; any other value synchronises the stream."""
    L = _capi.lib()
    p, wm = float(pNorm), int(bool(withMax))
    if isinstance(pages, np.ndarray):
        return _host(pages, _three, lambda c, *a: L.prl_hip_gray_world_host(p, wm, *a), out)
    return _device(pages, _three, lambda n, c, *a: L.prl_hip_gray_world_batch_device(n, p, wm, *a), out)


def cleanBackgroundToWhite(pages, out=None):
    """prl::cleanBackgroundToWhite: backgroundNormalization, then Leptonica's pixGammaTRC(1.0, 70, 170); 4 channels come back as 3."""
    L = _capi.lib()
    oc_of = lambda c: 1 if c == 1 else 3  # noqa: E731
    if isinstance(pages, np.ndarray):
        return _host(pages, oc_of, L.prl_hip_clean_background_host, out)
    return _device(pages, oc_of, L.prl_hip_clean_background_batch_device, out)


def histogram(pages, out=None):
    """Per page and channel, the 256-bin histogram: a torch int32 tensor [N,] C x 256 holding the uint32 counts (a page has at
    most 2^30 pixels), on the input's device; `out` (int32, contiguous) is overwritten."""
    import torch

    t4, _, batch = _pages4(pages)
    n, h, w, c = t4.shape
    oshape = ((n,) if batch else ()) + (c, 256)
    res = torch.empty(oshape, dtype=torch.int32, device=pages.device) if out is None else out
    if not isinstance(res, torch.Tensor) or tuple(res.shape) != oshape or res.dtype != torch.int32 or res.device != pages.device \
            or not res.is_contiguous():
        raise TypeError("out must be a contiguous int32 tensor [N,] C x 256 on the input's device")
    L = _capi.lib()
    _capi.check(L.prl_hip_set_device(pages.device.index or 0))
    stream = torch.cuda.current_stream(pages.device).cuda_stream
    _capi.check(L.prl_hip_histogram_batch_device(n, c, t4.data_ptr(), t4.stride(0), t4.stride(1), w, h, res.data_ptr(), stream))
    return res


def lut(pages, table, out=None):
    """cv::LUT: out(y, x, c) = table[c][pages(y, x, c)].  `table`: a uint8 CUDA tensor C x 256 (or 256 for 1 channel) shared by all
    pages, or N x C x 256 with a set per page."""
    import torch

    t4, _, _ = _pages4(pages)
    n, c = t4.shape[0], t4.shape[3]
    if not isinstance(table, torch.Tensor) or table.dtype != torch.uint8 or table.device != pages.device:
        raise TypeError("table must be a uint8 tensor on the input's device")
    tab = table.contiguous()
    if tuple(tab.shape) in ((c, 256), (256,) if c == 1 else None):
        stride = 0
    elif tuple(tab.shape) in ((n, c, 256), (n, 256) if c == 1 else None):
        stride = c * 256
    else:
        raise TypeError("table must be C x 256 or N x C x 256")
    L = _capi.lib()
    return _device(pages, _same, lambda n_, c_, *a: L.prl_hip_lut_batch_device(n_, c_, tab.data_ptr(), stride, *a), out)
