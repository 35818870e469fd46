"""Frames for the rate API's tests: tests/content_pairs.py's pairs as YUV 4:2:0 planes in the four containers (NV12, I420, P010,
yuv420p10le), converted by the integer oracles (tests/yuv_oracle.py, tests/yuv_hd_oracle.py).  Ten-bit frames are the 8-bit BGR code
values widened by bit replication ((v << 2) | (v >> 6): 0 -> 0, 255 -> 1023) before the conversion."""
import functools

import numpy as np

import content_pairs as CP
import yuv_hd_oracle as HD
import yuv_oracle as O

CUT_CASES = ("cut", "fade", "fade_in")             # what a maintainer wants repeated, not interpolated
FORMATS = [("nv12", 8), ("i420", 8), ("nv12", 10), ("i420", 10)]


def widen10(u8):
    a = np.asarray(u8).astype(np.uint16)
    return (a << 2) | (a >> 6)


def planes_of_bgr(bgr, layout, depth, mat="bt709", rng="limited", dirt=None):
    """One planar BGR uint8 frame [3,H,W] -> the container's planes (numpy)."""
    if depth == 8:
        return HD.pack_planes(*O.bgr_to_yuv420(np.ascontiguousarray(bgr), mat, rng), layout, 8)
    return HD.pack_planes(*HD.bgr_to_yuv420(widen10(bgr), mat, rng, 10), layout, 10, dirt=dirt)


@functools.lru_cache(maxsize=64)
def content(case, H, W, seed=0, layout="nv12", depth=8, mat="bt709", rng="limited"):
    """(planes of I0, planes of I1) of content_pairs.pair(case, H, W, seed)."""
    u8 = CP.pair(case, H, W, seed).numpy()
    return tuple(planes_of_bgr(u8[i], layout, depth, mat, rng) for i in range(2))
