"""Connected components and rule R's external rectangles on device tensors over the C ABI (components.hip; the rules are stated in
include/prl_hip.h next to prl_hip_external_rects).  Maps are uint8 CUDA tensors [N,] H x W, non-zero = foreground; pages and rows
may be strided, pixels must be dense (the rule of _pages.py).  Errors are PrlError with the C status.  The host scan on numpy
maps stays localotsu.externalRects.
"""
from __future__ import annotations

import numpy as np

from . import _capi, _pages

TILE = 32   # kCcTile: the side of the tile a workgroup labels in LDS


def _maps(maps):
    t4, _chan, batch = _pages.pages4(maps, gray_only=True)
    n, h, w, _ = t4.shape
    return t4, n, h, w, batch


def connectedComponents(maps, connectivity=8, with_stats=False):
    """The foreground components of every map, 8- or 4-connected: (labels, counts[, stats]).  labels: int32 tensor of the maps'
    shape, 0 for the background and 1 .. K per page in increasing order of first pixel (the smallest y * W + x); counts: K per page
    (an int for a single page); stats: one K x 5 int32 tensor per page of left, top, width, height, area in label order (a single
    one for a single page).  with_stats makes a second call once the counts are known, which labels the maps again."""
    import torch

    t4, n, h, w, batch = _maps(maps)
    L = _capi.lib()
    labels = torch.empty((n, h, w), dtype=torch.int32, device=maps.device)
    counts = np.zeros(max(n, 1), np.int32)
    stream = _capi.stream_on(maps)

    def call(lab, stats, room, k):
        _capi.check(L.prl_hip_connected_components_batch_device(n, int(connectivity), t4.data_ptr(), t4.stride(0), t4.stride(1), w, h, lab,
                                                                4 * w * h, 4 * w, k.ctypes.data, stats, room, stream))

    call(labels.data_ptr(), None, 0, counts)
    counts = counts[:n]
    res = (labels if batch else labels[0], counts if batch else int(counts[0]))
    if not with_stats:
        return res
    total = int(counts.sum())
    flat = torch.zeros((max(total, 1), 5), dtype=torch.int32, device=maps.device)
    if total:   # the counts are known now: the statistics get exactly their room
        call(None, flat.data_ptr(), total, np.zeros(max(n, 1), np.int32))
    ends = np.cumsum(counts)
    stats = [flat[int(e) - int(k):int(e)] for k, e in zip(counts, ends)]
    return res + (stats if batch else stats[0],)


def externalRects(maps):
    """Rule R on every map: (rects, found).  rects: one K x 4 int32 numpy array of x, y, width, height per page, the bounding
    rectangles of the kept external components in increasing order of first pixel (a single array for a single page) - what
    cv::findContours(RETR_EXTERNAL) and the drop of the contours of fewer than 3 points leave; found: the external components per
    page."""
    rects, offsets, found, _kept = externalRectsDevice(maps)
    host = rects.cpu().numpy()
    lists = [host[offsets[i]:offsets[i + 1]] for i in range(len(found))]
    return (lists, found) if maps.dim() == 3 else (lists[0], int(found[0]))


def externalRectsDevice(maps, room=None):
    """The same with the rectangles left on the device: (rects int32 tensor total x 4, offsets [N + 1], found [N], kept [N]).  room:
    rectangles the first call has room for (None: a call for the counts, then one with exactly their room); with too little room
    the rectangles are not written and rects is None."""
    import torch

    t4, n, h, w, _batch = _maps(maps)
    L = _capi.lib()
    offsets, found, kept = np.zeros(n + 1, np.int32), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    stream = _capi.stream_on(maps)

    def call(rects, cap):
        _capi.check(L.prl_hip_external_rects_batch_device(n, t4.data_ptr(), t4.stride(0), t4.stride(1), w, h,
                                                          rects.data_ptr() if rects is not None else None, cap, offsets.ctypes.data,
                                                          found.ctypes.data, kept.ctypes.data, stream))

    rects = None
    if room is None:
        call(None, 0)
        room = int(offsets[n])
        if room == 0:
            return torch.zeros((0, 4), dtype=torch.int32, device=maps.device), offsets, found[:n], kept[:n]
    rects = torch.full((max(room, 1), 4), -1, dtype=torch.int32, device=maps.device)
    call(rects, room)
    total = int(offsets[n])
    return (rects[:total] if total <= room else None), offsets, found[:n], kept[:n]
