"""The numpy statement of the interlace API (include/fldr_interlace.h): the weave with its three vertical filters, and the stream's
schedule in exact fractions.  The tests hold libfldr_interlace.so to it byte for byte."""
from fractions import Fraction

import numpy as np

from field_oracle import canonical, mx, value

NONE, LINEAR, COMPLEX = 0, 1, 2


def filter_plane(src, layout, depth, filt):
    """Every row of one progressive plane through the filter: s(k) is the value of row clamp(k, 0, R - 1) in the same column."""
    if filt == NONE:
        return src.copy()
    v = value(src, layout, depth)
    R = v.shape[0]
    s = lambda d: v[np.clip(np.arange(R) + d, 0, R - 1)]
    if filt == LINEAR:
        o = (s(-1) + 2 * s(0) + s(1) + 2) >> 2
    else:
        o = np.clip((-s(-2) + 2 * s(-1) + 6 * s(0) + 2 * s(1) - s(2) + 4) >> 3, 0, mx(depth))      # >> on int64 is arithmetic: floor
    return canonical(o, layout, depth)


def weave(even, odd, layout, depth, filt=NONE, out=None):
    """fldr_interlace_weave: rows y % 2 == 0 of every plane from `even`, rows y % 2 == 1 from `odd` (frames: tuples of numpy planes), each
    through the filter.  A source that is None leaves its rows as they are in `out` (a frame, which is not modified: a copy is returned)."""
    assert even is not None or odd is not None
    ref = even if even is not None else odd
    res = [p.copy() for p in out] if out is not None else [np.zeros_like(p) for p in ref]
    assert out is not None or (even is not None and odd is not None)
    for q, src in ((0, even), (1, odd)):
        if src is None:
            continue
        for p, plane in enumerate(src):
            assert plane.shape[0] % 2 == 0
            res[p][q::2] = filter_plane(plane, layout, depth, filt)[q::2]
    return tuple(res)


# ---- the schedule ---------------------------------------------------------------------------------------------------------------------
def _rate(r):
    return Fraction(*r) if isinstance(r, tuple) else Fraction(r)


def field_step(in_rate, out_rate):
    """Input frames per field: in_rate / (2 out_rate), out_rate in interlaced FRAMES per second."""
    return _rate(in_rate) / (2 * _rate(out_rate))


def plan(k, in_rate, out_rate, tff=True):
    """Output frame k: {"frame", "input": [i0, i1], "r": [r0, r1], "B", "parity": [p0, p1], "push"} — field 2k + f sits at input position
    (2k + f) x step = i + r / B; the push of frame i1 + 1 returns the frame."""
    step = field_step(in_rate, out_rate)
    B = step.denominator
    pos = [(2 * k + f) * step for f in range(2)]
    i = [p.numerator // p.denominator for p in pos]
    r = [int((p - ii) * B) for p, ii in zip(pos, i)]
    first = 0 if tff else 1
    return {"frame": k, "input": i, "r": r, "B": B, "parity": [first, 1 - first], "push": i[1] + 1}


def max_out(in_rate, out_rate):
    """(ceil(B / A) + 1) // 2 with A / B the field step."""
    step = field_step(in_rate, out_rate)
    return (-(-step.denominator // step.numerator) + 1) // 2


def stream_frames(n_frames, in_rate, out_rate):
    """What a stream of n_frames frames returns, by brute force over the fields: a list of n_frames + 1 lists of (k, held) — entry n the
    frames of the push of frame n, the last entry those of the flush.  Field m exists once a frame at or behind its position has been
    pushed (position <= n: the pair (n - 1, n), or frame n - 1 itself at the push of frame n); a frame goes out with its second field.
    At the flush the field on the last frame is made, and a frame left with its first field only is completed from the last frame."""
    step = field_step(in_rate, out_rate)
    pushes = [[] for _ in range(n_frames + 1)]
    if n_frames == 0:
        return pushes
    m = 0
    for n in range(1, n_frames):
        while m * step < n:
            if m & 1:
                pushes[n].append((m >> 1, False))
            m += 1
    if m * step == n_frames - 1:
        if m & 1:
            pushes[n_frames].append((m >> 1, False))
        m += 1
    if m & 1:
        pushes[n_frames].append((m >> 1, True))
    return pushes
