#!/usr/bin/env python3
"""Generates tests/golden/autocrop/*.npz: the reference's own photographs for the border detector (test_data/auto_crop, sixteen
JPEGs from 447 x 477 to 3264 x 2448), decoded with Pillow.

Run in the BUILD container (it reads /root/reference/test_data/auto_crop; nothing at test time does).  The reference ships the
photographs only, so what a fixture expects comes from the restatement (tests/contour_ref.py on tests/edges_ref.py's map, "parity
unpinned"): whether a quad is found, at which try, and its four corners.  A fixture holds DATA only: the BGR pixels cv::imread
would hand prl::autoCrop and those three results.  A photograph whose compressed fixture would exceed LIMIT bytes is left out; the
census over all sixteen is printed for profiles/r16/INDEX.md.
"""
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import contour_ref as cr  # noqa: E402

REF = "/root/reference/test_data/auto_crop"
OUT = os.path.join(HERE, "autocrop")
LIMIT = 1 << 20   # no committed file above 1 MiB (the largest fixture under tests/golden/scans is larger than that)


def main():
    os.makedirs(OUT, exist_ok=True)
    census = {"first": 0, "closing": 0, "none": 0}
    for k, name in enumerate(sorted(os.listdir(REF))):
        rgb = np.asarray(Image.open(os.path.join(REF, name)).convert("RGB"), dtype=np.uint8)   # cv::imread(IMREAD_COLOR)
        bgr = np.ascontiguousarray(rgb[:, :, ::-1])
        quad, tries = cr.document_contour(bgr)
        census["none" if quad is None else ("first", "closing")[tries]] += 1
        tag = "photo_%02d_%dx%d" % (k, bgr.shape[1], bgr.shape[0])
        path = os.path.join(OUT, tag + ".npz")
        np.savez_compressed(path, bgr=bgr, found=np.int32(quad is not None), tries=np.int32(tries),
                            quad=np.zeros(8, np.float32) if quad is None else quad, source=np.array(name))
        size = os.path.getsize(path)
        kept = size <= LIMIT
        if not kept:
            os.remove(path)
        print(tag, name, "found" if quad is not None else "none", "try", tries, size // 1024, "KiB", "kept" if kept else "left out", flush=True)
    print("census of 16:", census)


if __name__ == "__main__":
    main()
