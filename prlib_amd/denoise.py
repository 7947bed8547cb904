"""Host-side mirror of prl::denoise (src/denoise/denoiseNLM.h:32, denoiseNLM.cpp:29-32) over the C ABI.

    void prl::denoise(const cv::Mat& inputImage, cv::Mat& outputImage, double strength = 5.5)
      = cv::fastNlMeansDenoisingColored(inputImage, outputImage, strength)     [hColor 3, template 7, search 21]

numpy H x W x {3,4} uint8 -> numpy (staged through the device by the library);
torch CUDA uint8 [N,] H x W x {3,4} -> torch tensor on the same device.  Other channel counts raise, as
the reference's OpenCV call does ("Type of input image should be CV_8UC3 or CV_8UC4!").

denoiseSaltPepper: the other half of the reference's denoise module, `times` passes of cv::medianBlur (median.hip).
"""
from __future__ import annotations

import numpy as np

from . import _capi


def denoise(inputImage, strength: float = 5.5, out=None):
    if isinstance(inputImage, np.ndarray):
        img = np.ascontiguousarray(inputImage)
        if img.ndim != 3 or img.dtype != np.uint8:
            raise TypeError("expected an H x W x C uint8 image")
        h, w, c = img.shape
        res = np.empty_like(img)
        _capi.check(_capi.lib().prl_hip_denoise_host(c, float(strength), img.ctypes.data, img.strides[0], w, h,
                                                     res.ctypes.data, res.strides[0]))
        return res
    import torch

    t = inputImage
    squeeze = t.dim() == 3
    if squeeze:
        t = t.unsqueeze(0)
    if t.dtype != torch.uint8 or not t.is_cuda or t.dim() != 4 or not t.is_contiguous():
        raise TypeError("expected a contiguous uint8 CUDA tensor [N,] H x W x C")
    n, h, w, c = t.shape
    if out is None:
        out = torch.empty_like(t)
    L = _capi.lib()
    _capi.check(L.prl_hip_set_device(t.device.index or 0))
    stream = torch.cuda.current_stream(t.device).cuda_stream
    _capi.check(L.prl_hip_denoise_batch_device(n, c, float(strength), t.data_ptr(), t.stride(0), t.stride(1), w, h,
                                               out.data_ptr(), out.stride(0), out.stride(1), stream))
    return out[0] if squeeze else out


def nlm_planes(planes, h: float, out=None):
    """cv::fastNlMeansDenoising core on 1/2/3 interleaved u8 planes (CUDA tensor [N,] H x W [x C])."""
    import torch

    t = planes
    if t.dim() == 2:
        t4 = t[None, :, :, None]
    elif t.dim() == 3:
        t4 = t[None]
    else:
        t4 = t
    t4 = t4.contiguous()
    n, hh, w, c = t4.shape
    res = torch.empty_like(t4) if out is None else out.view(t4.shape)
    L = _capi.lib()
    _capi.check(L.prl_hip_set_device(t4.device.index or 0))
    stream = torch.cuda.current_stream(t4.device).cuda_stream
    _capi.check(L.prl_hip_nlm_planes_device(n, c, float(h), t4.data_ptr(), t4.stride(0), t4.stride(1), w, hh,
                                            res.data_ptr(), res.stride(0), res.stride(1), stream))
    return res.view(t.shape)


def denoiseSaltPepper(image, kernelSize: int, times: int, out=None):
    """prl::denoiseSaltPepper (src/denoise/denoiseSaltPepper.h:40, .cpp:29-36): `times` passes of cv::medianBlur(out, out,
    kernelSize) over a copy of the input (BORDER_REPLICATE, exact median of every k x k window, channels independent).

    numpy H x W or H x W x C uint8 -> numpy (through the library's host entry); torch CUDA uint8 [N,] H x W [x C] -> torch
    tensor on the same device, enqueued on the current stream (a 3-dimensional tensor is H x W x C when its last dimension is
    at most 4, else N x H x W).  Pages and rows may be strided; pixels and channels must be dense.  `out` receives the
    result (out is image: in place).  Errors are PrlError with the C status."""
    if times < 0:
        raise _capi.PrlError(_capi.PRL_ERR_BAD_ARG, "times must be >= 0")
    L = _capi.lib()
    if isinstance(image, np.ndarray):
        if image.dtype != np.uint8 or image.ndim not in (2, 3):
            raise TypeError("expected an H x W [x C] uint8 array")
        img = image if image.ndim == 3 else image[:, :, None]
        if img.strides[2] != 1 or img.strides[1] != img.shape[2] or img.strides[0] < 0:
            img = np.ascontiguousarray(img)
        h, w, c = img.shape
        res = np.empty(image.shape, np.uint8) if out is None else out
        if not isinstance(res, np.ndarray) or res.shape != image.shape or res.dtype != np.uint8 or not res.flags.c_contiguous:
            raise TypeError("out must be a C-contiguous uint8 array of the input's shape")
        _capi.check(L.prl_hip_median_host(c, int(kernelSize), int(times), img.ctypes.data, img.strides[0], w, h,
                                          res.ctypes.data, res.strides[0] if res.ndim else 0))
        return res
    import torch

    t = image
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_cuda or t.dim() not in (2, 3, 4):
        raise TypeError("expected a uint8 CUDA tensor [N,] H x W [x C] or a numpy uint8 array")

    def as4(x):
        if x.dim() == 2:
            return x[None, :, :, None]
        if x.dim() == 3:
            return x[None] if x.shape[-1] <= 4 else x[:, :, :, None]
        return x

    t4 = as4(t)
    n, h, w, c = t4.shape
    if t4.stride(3) != 1 and c > 1 or t4.stride(2) != c:
        t4 = t4.contiguous()
    res = torch.empty(t.shape, dtype=torch.uint8, device=t.device) if out is None else out
    r4 = as4(res)
    if r4.shape != t4.shape or res.dtype != torch.uint8 or res.device != t.device or (r4.stride(3) != 1 and c > 1) or r4.stride(2) != c:
        raise TypeError("out must be a uint8 tensor of the input's shape on its device, pixels and channels dense")
    _capi.check(L.prl_hip_set_device(t.device.index or 0))
    stream = torch.cuda.current_stream(t.device).cuda_stream
    _capi.check(L.prl_hip_median_batch_device(n, c, int(kernelSize), int(times), t4.data_ptr(), t4.stride(0), t4.stride(1), w, h,
                                              r4.data_ptr(), r4.stride(0), r4.stride(1), stream))
    return res
