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

from . import _capi, _pages


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
    return _pages.run(pages, oc_of,
                      lambda c, *a: L.prl_hip_gamma_correction_host(c, k, gamma, *a),
                      lambda n, c, *a: L.prl_hip_gamma_correction_batch_device(n, c, k, gamma, *a), out)


def simpleWhiteBalance(pages, k, out=None):
    """prl::simpleWhiteBalance on 3-channel pages: per channel, stretch [vmin, vmax] (the k and 1 - k quantiles) to [0, 255]."""
    L = _capi.lib()
    k = float(k)
    return _pages.run(pages, _three,
                      lambda c, *a: L.prl_hip_simple_white_balance_host(k, *a),
                      lambda n, c, *a: L.prl_hip_simple_white_balance_batch_device(n, k, *a), out)


def grayWorldWhiteBalance(pages, pNorm, withMax, out=None):
    """prl::grayWorldWhiteBalance on 3-channel pages: every channel scaled so that its p-norm mean meets the mean (or, withMax, the
    largest) of the three.  pNorm == 1 stays on the device; any other value synchronises the stream."""
    L = _capi.lib()
    p, wm = float(pNorm), int(bool(withMax))
    return _pages.run(pages, _three,
                      lambda c, *a: L.prl_hip_gray_world_host(p, wm, *a),
                      lambda n, c, *a: L.prl_hip_gray_world_batch_device(n, p, wm, *a), out)


def cleanBackgroundToWhite(pages, out=None):
    """prl::cleanBackgroundToWhite: backgroundNormalization, then Leptonica's pixGammaTRC(1.0, 70, 170); 4 channels come back as 3."""
    L = _capi.lib()
    oc_of = lambda c: 1 if c == 1 else 3  # noqa: E731
    return _pages.run(pages, oc_of, L.prl_hip_clean_background_host, L.prl_hip_clean_background_batch_device, out)


def histogram(pages, out=None):
    """Per page and channel, the 256-bin histogram: a torch int32 tensor [N,] C x 256 holding the uint32 counts (a page has at
    most 2^30 pixels), on the input's device; `out` (int32, contiguous) is overwritten."""
    import torch

    t4, _, batch = _pages.pages4(pages)
    n, h, w, c = t4.shape
    oshape = ((n,) if batch else ()) + (c, 256)
    res = torch.empty(oshape, dtype=torch.int32, device=pages.device) if out is None else out
    if not isinstance(res, torch.Tensor) or tuple(res.shape) != oshape or res.dtype != torch.int32 or res.device != pages.device \
            or not res.is_contiguous():
        raise TypeError("out must be a contiguous int32 tensor [N,] C x 256 on the input's device")
    _capi.check(_capi.lib().prl_hip_histogram_batch_device(n, c, t4.data_ptr(), t4.stride(0), t4.stride(1), w, h, res.data_ptr(),
                                                           _capi.stream_on(pages)))
    return res


def lut(pages, table, out=None):
    """cv::LUT: out(y, x, c) = table[c][pages(y, x, c)].  `table`: a uint8 CUDA tensor C x 256 (or 256 for 1 channel) shared by all
    pages, or N x C x 256 with a set per page."""
    import torch

    t4, _, _ = _pages.pages4(pages)
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
    return _pages.run(pages, _pages.same, None, lambda n_, c_, *a: L.prl_hip_lut_batch_device(n_, c_, tab.data_ptr(), stride, *a), out)
