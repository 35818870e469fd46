"""The yardstick of the linear-light API's tests (include/fldr_light.h), numpy only: the three transfer curves in float64, the table
rule, accumulate / resolve / mix composed from tests/yuv_hd_oracle.py's two conversions and the header's three lines, and the converter
stated through tests/shutter_oracle.outputs.  Nothing here is derived from the library: the curves are the published formulas
(BT.1886 with zero black, SMPTE ST 2084, BT.2100 HLG), the arithmetic is the header's, in int64."""
import numpy as np

import shutter_oracle as SO
import yuv_hd_oracle as HD

S = (1 << 24) - 1
TRANSFERS = ("gamma24", "pq", "hlg")


# ---- the curves ---------------------------------------------------------------------------------------------------------------------------
def gamma24(v):
    return np.asarray(v, np.float64) ** 2.4


def pq(v):
    """SMPTE ST 2084 EOTF, 10000 cd/m^2 = 1."""
    m1, m2 = 2610.0 / 16384.0, 2523.0 / 4096.0 * 128.0
    c1, c2, c3 = 3424.0 / 4096.0, 2413.0 / 4096.0 * 32.0, 2392.0 / 4096.0 * 32.0
    e = np.asarray(v, np.float64) ** (1.0 / m2)
    return (np.maximum(e - c1, 0.0) / (c2 - c3 * e)) ** (1.0 / m1)


def _hlg(v):
    a = 0.17883277
    b, c = 1.0 - 4.0 * a, 0.5 - a * np.log(4.0 * a)
    v = np.asarray(v, np.float64)
    return np.where(v <= 0.5, v * v / 3.0, (np.exp((v - c) / a) + b) / 12.0)


def hlg(v):
    """BT.2100 HLG inverse OETF (scene light), scaled so that V = 1 gives 1."""
    return _hlg(v) / _hlg(1.0)


CURVES = {"gamma24": gamma24, "pq": pq, "hlg": hlg}


def rounded(transfer, depth):
    """round(f(c / max) * S) for every code, BEFORE the + 1 floor -> int64 [2^depth]."""
    n = 1 << depth
    return np.floor(CURVES[transfer](np.arange(n) / float(n - 1)) * S + 0.5).astype(np.int64)


def table(transfer, depth):
    """lin[0] = 0, lin[c] = max(round(f(V) S), lin[c - 1] + 1)."""
    r = rounded(transfer, depth)
    lin = np.zeros_like(r)
    for c in range(1, len(r)):
        lin[c] = max(r[c], lin[c - 1] + 1)
    return lin


def mid_of(lin):
    """mid[c] = lin[c - 1] + lin[c] for c = 1 .. max -> int64 [max] (index c - 1)."""
    lin = np.asarray(lin).astype(np.int64)
    return lin[:-1] + lin[1:]


# ---- the three lines ----------------------------------------------------------------------------------------------------------------------
def accumulate_codes(codes, weights, lin, acc=None):
    """acc (int64 [3,H,W], None = zero) + sum of w_k lin[codes_k]."""
    lin = np.asarray(lin).astype(np.int64)
    a = np.zeros(codes[0].shape, np.int64) if acc is None else acc.copy()
    for c, w in zip(codes, weights):
        a += int(w) * lin[np.asarray(c).astype(np.int64)]
    assert a.max() < 2 ** 32
    return a


def resolve_codes(acc, total, lin):
    """q = (2 acc + total) // (2 total); code = #{c in 1 .. max : mid[c] <= 2 q}."""
    q = (2 * acc + total) // (2 * total)
    return np.searchsorted(mid_of(lin), 2 * q, "right")


# ---- frames -----------------------------------------------------------------------------------------------------------------------------
def to_codes(frame, layout, depth, mat="bt709", rng="limited"):
    """A frame's container planes -> planar BGR codes [3,H,W] by the video library's rule."""
    return HD.yuv420_to_bgr(*HD.unpack_planes(frame, layout, depth), mat, rng, depth)


def from_codes(codes, layout, depth, mat="bt709", rng="limited"):
    return HD.pack_planes(*HD.bgr_to_yuv420(codes.astype(HD.dtype_of(depth)), mat, rng, depth), layout, depth)


def accumulate(frames, weights, lin, layout, depth, mat="bt709", rng="limited", acc=None):
    return accumulate_codes([to_codes(f, layout, depth, mat, rng) for f in frames], weights, lin, acc)


def resolve(acc, total, lin, layout, depth, mat="bt709", rng="limited"):
    return from_codes(resolve_codes(acc, total, lin), layout, depth, mat, rng)


def mix(frames, weights, lin, layout, depth, mat="bt709", rng="limited"):
    return resolve(accumulate(frames, weights, lin, layout, depth, mat, rng), sum(int(w) for w in weights), lin, layout, depth, mat, rng)


def mix_codes(codes, weights, lin, layout, depth, mat="bt709", rng="limited"):
    """The mix of frames given as planar BGR codes (what fldr_light_forward reads from the video workspace) -> a frame."""
    return from_codes(resolve_codes(accumulate_codes(codes, weights, lin), sum(int(w) for w in weights), lin), layout, depth, mat, rng)


# ---- the converter --------------------------------------------------------------------------------------------------------------------------
def outputs(n_frames, in_rate, out_rate, shutter, sub, cuts=()):
    """shutter_oracle.outputs, with what the linear converter adds: "unchanged" — the output keeps exactly one point and that point
    takes an input frame's samples (k == 0, or a cut pair's source), so it is that frame's bytes and never passes through R'G'B'."""
    res = SO.outputs(n_frames, in_rate, out_rate, shutter, sub, cuts)
    for o in res:
        assert len(o["points"]) <= 255
        (i, k, src), = o["points"] if len(o["points"]) == 1 else ((None, None, None),)
        o["unchanged"] = None if i is None or (k and src is None) else (i if k == 0 else src)
    return res


def output_frame(o, frame_of_point, lin, layout, depth, mat="bt709", rng="limited"):
    """The frame of one entry of outputs(); frame_of_point(i, k, src) -> the container planes of that point."""
    pts = [frame_of_point(i, k, src) for i, k, src in o["points"]]
    if o["unchanged"] is not None:
        return pts[0]
    return mix(pts, [1] * len(pts), lin, layout, depth, mat, rng)
