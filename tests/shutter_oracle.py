"""The yardsticks of the shutter API's tests (include/fldr_shutter.h): a numpy statement of the integer sample rules and a
fractions.Fraction statement of the window rule, the cut rule and the push that returns each output.  Nothing here is derived from
the library: the sample rules are the header's three sentences, the windows are half-open intervals of exact rationals."""
from fractions import Fraction

import numpy as np


def _rate(r):
    return Fraction(*r) if isinstance(r, tuple) else Fraction(r)


# ---- samples ------------------------------------------------------------------------------------------------------------------------------
def value(plane, layout, depth):
    """The value of every sample of a plane: the byte; word >> 6 (P010); word & 0x3ff (yuv420p10le) -> int64."""
    a = np.asarray(plane).astype(np.int64)
    if depth != 10:
        return a
    return a >> 6 if layout == "nv12" else a & 0x3ff


def written(v, layout, depth):
    """The values written back: the byte; v << 6; v."""
    if depth != 10:
        return v.astype(np.uint8)
    return (v << 6).astype(np.uint16) if layout == "nv12" else v.astype(np.uint16)


def accumulate(frames, weights, layout, depth, acc=None):
    """acc (a list of int64 planes, None = zero) + sum of weights[k] * value(frames[k]), plane by plane."""
    out = []
    for p in range(len(frames[0])):
        a = np.zeros(frames[0][p].shape, np.int64) if acc is None else acc[p].copy()
        for f, w in zip(frames, weights):
            a += int(w) * value(f[p], layout, depth)
        out.append(a)
    return out


def resolve(acc, total, layout, depth):
    """(2 acc + total) // (2 total), clamped to the depth's maximum, written in the format."""
    mx = 1023 if depth == 10 else 255
    return tuple(written(np.minimum((2 * a + total) // (2 * total), mx), layout, depth) for a in acc)


def mix(frames, weights, layout, depth):
    return resolve(accumulate(frames, weights, layout, depth), sum(int(w) for w in weights), layout, depth)


# ---- windows ------------------------------------------------------------------------------------------------------------------------------
def window(j, in_rate, out_rate, shutter, sub):
    """(first, last) grid point of output j: the m with j A / B <= m / sub < j A / B + s A / B, in exact rationals."""
    q = _rate(in_rate) / _rate(out_rate)
    s = _rate(shutter)
    start, end = j * q * sub, (j * q + s * q) * sub                # in grid points
    first = -((-start.numerator) // start.denominator)             # ceil
    last = -((-end.numerator) // end.denominator) - 1              # the last m < end
    return first, last


def outputs(n_frames, in_rate, out_rate, shutter, sub, cuts=()):
    """Every output of a stream of n_frames frames, stated point by point: a list of dicts j, points [(i, k, source)], truncated, push.
    cuts: the frames n whose pair (n - 1, n) is a cut.  Point m = i sub + k.  Its scene: the cuts at or before it, the points of a cut
    pair with 2 k >= sub counting as after.  A window keeps the points in the scene of its first point.  On a cut pair a point with
    k > 0 takes frame i when 2 k < sub, else frame i + 1 (source); elsewhere source is None.  push: the push that supplies the last
    kept point, or — the window cut short — the one that supplies the first dropped point, whose measure shows the cut; n_frames
    (the flush) when the stream ends inside the window."""
    cuts = sorted(cuts)
    q = _rate(in_rate) / _rate(out_rate)
    last_m = (n_frames - 1) * sub

    def scene(m):
        i, k = divmod(m, sub)
        before = sum(1 for c in cuts if c <= i)                    # a cut pair (c - 1, c): frame c and everything behind is after it
        return before + (1 if k > 0 and (i + 1) in cuts and 2 * k >= sub else 0)

    def push_of(m):
        return -(-m // sub)                                        # point m needs frame ceil(m / sub)

    res, j = [], 0
    while j * q <= n_frames - 1:
        f, l = window(j, in_rate, out_rate, shutter, sub)
        assert f <= l, "an empty window"
        kept, truncated, push = [], False, None
        for m in range(f, l + 1):
            if m > last_m:
                truncated, push = True, n_frames
                break
            if scene(m) != scene(f):
                truncated, push = True, push_of(m)
                break
            i, k = divmod(m, sub)
            src = None
            if k > 0 and (i + 1) in cuts:
                src = i if 2 * k < sub else i + 1
            kept.append((i, k, src))
        if push is None:
            push = push_of(l)
        res.append({"j": j, "points": kept, "truncated": truncated, "push": push})
        j += 1
    return res
