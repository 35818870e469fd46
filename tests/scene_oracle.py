"""The numpy statement of the cut measure of include/fldr_rate.h (fldr_scene_measure), in integers.

y8(sample): the luma sample reduced to 8 bits — the byte at depth 8, word >> 8 for P010 (nv12 at depth 10), (word & 0x3ff) >> 2 for
yuv420p10le (i420 at depth 10).  Only plane 0 is read.
    sad       = sum |y8(I0) - y8(I1)|
    hist_dist = sum_b |h0[b] - h1[b]|, h the 256-bin histograms of y8
    cut       = sad * 1000 >= sad_permille * 255 * H * W  and  hist_dist * 1000 >= hist_permille * 2 * H * W"""
import os
import re

import numpy as np

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fldr_rate.h")


def defaults():
    """(FLDR_SCENE_SAD_DEFAULT, FLDR_SCENE_HIST_DEFAULT), parsed from the header."""
    text = open(HEADER).read()
    return tuple(int(re.search(r"#define\s+FLDR_SCENE_%s_DEFAULT\s+(\d+)" % n, text).group(1)) for n in ("SAD", "HIST"))


def y8(plane, layout="nv12", depth=8):
    p = np.asarray(plane)
    if depth != 10:
        return p.astype(np.int64)
    return (p.astype(np.int64) >> 8) if layout == "nv12" else ((p.astype(np.int64) & 0x3ff) >> 2)


def measure(planes0, planes1, fmt=("nv12", 8), params=None):
    """planes0 / planes1: the planes of the two frames (only [0], the luma plane, is read); fmt: (layout, depth) or an object with
    .name and .bits (fldr_video.Format); params: (sad_permille, hist_permille), None or zeros = the header's defaults."""
    layout, depth = (fmt.name, fmt.bits) if hasattr(fmt, "bits") else fmt
    a, b = y8(planes0[0], layout, depth), y8(planes1[0], layout, depth)
    H, W = a.shape
    sad = int(np.abs(a - b).sum())
    h0, h1 = np.bincount(a.ravel(), minlength=256), np.bincount(b.ravel(), minlength=256)
    hist_dist = int(np.abs(h0 - h1).sum())
    d = defaults()
    sp, hp = (int(v) or d[i] for i, v in enumerate(params or (0, 0)))
    cut = int(sad * 1000 >= sp * 255 * H * W and hist_dist * 1000 >= hp * 2 * H * W)
    return {"sad": sad, "hist_dist": hist_dist, "cut": cut}


def permille(m, H, W):
    """(sad, hist_dist) of a measure in permille of their maxima (floor)."""
    return m["sad"] * 1000 // (255 * H * W), m["hist_dist"] * 1000 // (2 * H * W)
