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

from . import _capi, _pages


def removeLines(pages, out=None):
    """prl::removeLines: 0 where a pixel is ink (Otsu on the inverted page) outside every long horizontal / vertical run, else 255."""
    L = _capi.lib()
    return _pages.run(pages, _pages.same, L.prl_hip_remove_lines_host, L.prl_hip_remove_lines_batch_device, out, drop_channel=True)
