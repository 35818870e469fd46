"""The numpy statement of include/fldr_scale.h, section "THE RULE": the tables in float64 with exact centres (taps_float), and the integer
arithmetic of a scale on the library's own tables (scale), so that the comparison with the kernel is byte-exact whatever the host's sin
gives.  Frames are tuples of 2-D numpy planes as fldr_video lays them out; sizes are (H, W)."""
import math
from fractions import Fraction

import numpy as np

BILINEAR, BICUBIC, LANCZOS3 = 0, 1, 2
LUMA, CHROMA_H, CHROMA_V = 0, 1, 2
BEFORE, AFTER, AUTO = 0, 1, 2
MAX_SIZE, MAX_TAPS = 16384, 64
RADIUS = {BILINEAR: 1, BICUBIC: 2, LANCZOS3: 3}


def weight(filter, x):
    x = abs(x)
    if filter == BILINEAR:
        return max(0.0, 1.0 - x)
    if filter == BICUBIC:
        if x < 1:
            return 1.5 * x ** 3 - 2.5 * x ** 2 + 1
        return -0.5 * x ** 3 + 2.5 * x ** 2 - 4 * x + 2 if x < 2 else 0.0
    if x >= 3:
        return 0.0
    sinc = lambda v: 1.0 if v == 0 else math.sin(math.pi * v) / (math.pi * v)
    return sinc(x) * sinc(x / 3)


def taps_count(luma_in, luma_out, filter):
    """n = 2 ceil(a max(1, r)), in exact arithmetic."""
    s = max(Fraction(1), Fraction(luma_in, luma_out))
    return 2 * math.ceil(RADIUS[filter] * s)


def outputs(luma_out, kind):
    return luma_out if kind == LUMA else (luma_out + 1) // 2


def centre(luma_in, luma_out, kind, o):
    """The centre of output o on the source axis of its plane, a Fraction."""
    r = Fraction(luma_in, luma_out)
    return o * r + (r - 1) / 4 if kind == CHROMA_H else (o + Fraction(1, 2)) * r - Fraction(1, 2)


def taps_float(luma_in, luma_out, filter, kind):
    """-> (n, left [outputs] of ints, x [outputs, n] float64): x_k = 16384 w_k / sum(w), before any rounding."""
    n = taps_count(luma_in, luma_out, filter)
    s = max(Fraction(1), Fraction(luma_in, luma_out))
    left, rows = [], []
    for o in range(outputs(luma_out, kind)):
        c = centre(luma_in, luma_out, kind, o)
        l = math.floor(c) - n // 2 + 1
        w = np.array([weight(filter, float((l + k - c) / s)) for k in range(n)], np.float64)
        left.append(l)
        rows.append(16384.0 * w / w.sum())
    return n, left, np.array(rows)


def where(where, in_size, out_size):
    if where != AUTO:
        return where
    return BEFORE if out_size[0] * out_size[1] < in_size[0] * in_size[1] else AFTER


def value(plane, layout, depth):
    """The sample values of a plane as int64."""
    p = plane.astype(np.int64)
    return p if depth != 10 else (p >> 6 if layout == "nv12" else p & 0x3ff)


def canonical(vals, layout, depth):
    if depth != 10:
        return vals.astype(np.uint8)
    return (vals << 6 if layout == "nv12" else vals).astype(np.uint16)


def scale_plane(s, tx, ty, depth):
    """One component plane of sample values (int64, rows x cols) through the tables tx, ty = (left, coef) -> the output values."""
    e = 14 - depth
    mx = (1 << depth) - 1
    (lx, qx), (ly, qy) = tx, ty
    lx, ly = np.asarray(lx, np.int64), np.asarray(ly, np.int64)
    qx, qy = np.asarray(qx, np.int64), np.asarray(qy, np.int64)
    rows, cols = s.shape
    ix = np.clip(lx[:, None] + np.arange(qx.shape[1])[None, :], 0, cols - 1)                # [out cols, nx]
    m = ((s[:, ix] * qx[None]).sum(axis=2) + (1 << (13 - e))) >> (14 - e)                   # [rows, out cols]
    assert np.abs(m).max() <= 32767
    iy = np.clip(ly[:, None] + np.arange(qy.shape[1])[None, :], 0, rows - 1)                # [out rows, ny]
    o = ((m[iy] * qy[:, :, None]).sum(axis=1) + (1 << (13 + e))) >> (14 + e)
    return np.clip(o, 0, mx)


def scale(frame, layout, depth, out_size, tables):
    """frame (any size) -> the frame at out_size = (H, W), by the library's tables ({"luma_x", "luma_y", "chroma_x", "chroma_y"} ->
    (left, coef))."""
    oH, oW = out_size
    out = [canonical(scale_plane(value(frame[0], layout, depth), tables["luma_x"], tables["luma_y"], depth), layout, depth)]
    assert out[0].shape == (oH, oW)
    if layout == "nv12":
        uv = value(frame[1], layout, depth)
        comps = [scale_plane(uv[:, c::2], tables["chroma_x"], tables["chroma_y"], depth) for c in range(2)]
        inter = np.empty((comps[0].shape[0], 2 * comps[0].shape[1]), np.int64)
        inter[:, 0::2], inter[:, 1::2] = comps
        out.append(canonical(inter, layout, depth))
    else:
        for p in (1, 2):
            out.append(canonical(scale_plane(value(frame[p], layout, depth), tables["chroma_x"], tables["chroma_y"], depth), layout, depth))
    assert out[1].shape[0] == (oH + 1) // 2
    return tuple(out)


def unclamped_range(plane_vals, tx, ty, depth):
    """(min, max) of the vertical pass's shifted value before the clamp: what the code-range tests assert left the range on both sides."""
    e = 14 - depth
    (lx, qx), (ly, qy) = tx, ty
    qx, qy = np.asarray(qx, np.int64), np.asarray(qy, np.int64)
    rows, cols = plane_vals.shape
    ix = np.clip(np.asarray(lx, np.int64)[:, None] + np.arange(qx.shape[1])[None, :], 0, cols - 1)
    m = ((plane_vals[:, ix] * qx[None]).sum(axis=2) + (1 << (13 - e))) >> (14 - e)
    iy = np.clip(np.asarray(ly, np.int64)[:, None] + np.arange(qy.shape[1])[None, :], 0, rows - 1)
    o = ((m[iy] * qy[:, :, None]).sum(axis=1) + (1 << (13 + e))) >> (14 + e)
    return int(o.min()), int(o.max())


def canonicalised(frame, layout, depth):
    """The frame with every sample in its container's canonical form: what an identity scale returns."""
    return tuple(canonical(value(p, layout, depth), layout, depth) for p in frame)
