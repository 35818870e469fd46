"""The numpy statement of the field API (include/fldr_field.h): the weave, plane by plane and component by component, and the schedule of
a stream.  A frame is a tuple of 2-D numpy planes (uint8, or uint16 at depth 10) as fldr_video's frames are: NV12 (Y, interleaved UV)
or I420 (Y, U, V).  Everything is an integer statement; tests/test_gpu_field.py holds the kernel to it byte for byte."""
import numpy as np

MOTION, INTRA = 0, 1
STILL_DEFAULT8, SLACK_DEFAULT8 = 2, 16


def mx(depth):
    return 1023 if depth == 10 else 255


def defaults(depth):
    """(still, slack) of a NULL fldr_field_params."""
    up = 2 if depth == 10 else 0
    return STILL_DEFAULT8 << up, SLACK_DEFAULT8 << up


def value(a, layout, depth):
    """v(.): the byte at depth 8, word >> 6 for P010, word & 0x3ff for yuv420p10le."""
    a = a.astype(np.int64)
    if depth != 10:
        return a
    return a >> 6 if layout == "nv12" else a & 0x3ff


def canonical(o, layout, depth):
    if depth != 10:
        return o.astype(np.uint8)
    return (o << 6).astype(np.uint16) if layout == "nv12" else o.astype(np.uint16)


def components(layout, p):
    """Interleaved components of plane p."""
    return 2 if layout == "nv12" and p == 1 else 1


def par(m, tff):
    return (m & 1) ^ (0 if tff else 1)


def weave_plane(cur, prev, nxt, temporal, parity, mode, still, slack, layout, depth, comp):
    R = cur.shape[0]
    assert R % 2 == 0
    out = cur.copy()                                                   # rows y % 2 == parity: the bytes of cur
    top = mx(depth)
    for y in range(R):
        if y % 2 == parity:
            continue
        ya = y - 1 if y > 0 else y + 1
        yb = y + 1 if y < R - 1 else y - 1
        a, b = value(cur[ya], layout, depth), value(cur[yb], layout, depth)
        if mode == INTRA:
            o = (a + b + 1) >> 1
        else:
            o = np.zeros_like(a)
            for c in range(comp):                                      # each component alike: its own columns x = 0 .. C - 1
                p = value(prev[y, c::comp], layout, depth)
                n = value(nxt[y, c::comp], layout, depth)
                t = value(temporal[y >> 1, c::comp], layout, depth)
                ac, bc = a[c::comp], b[c::comp]
                D = np.abs(p - n)
                C = D.shape[0]
                d = np.array([max(D[max(x - 1, 0)], D[x], D[min(x + 1, C - 1)]) for x in range(C)], np.int64)
                lo = np.maximum(np.minimum(ac, bc) - slack, 0)
                hi = np.minimum(np.maximum(ac, bc) + slack, top)
                clamped = np.minimum(np.maximum(t, lo), hi)
                static = (d <= still) if still >= 0 else np.zeros(C, bool)
                o[c::comp] = np.where(static, (p + n + 1) >> 1, clamped)
        out[y] = canonical(o, layout, depth)
    return out


def weave(cur, prev, nxt, temporal, layout, depth, parity, mode=MOTION, still=None, slack=None):
    """The progressive frame of fldr_field_weave.  prev / nxt: the frames holding the fields before / after; temporal: the H/2 x W
    frame; all three may be None in INTRA.  still / slack None: the defaults."""
    ds, dk = defaults(depth)
    still = ds if still is None else still
    slack = dk if slack is None else slack
    out = []
    for p in range(len(cur)):
        src = (None, None, None) if mode == INTRA else (prev[p], nxt[p], temporal[p])
        out.append(weave_plane(cur[p], src[0], src[1], src[2], parity, mode, still, slack, layout, depth, components(layout, p)))
    return tuple(out)


def field_view(frame, parity):
    return tuple(p[parity::2] for p in frame)


# ---- the schedule -----------------------------------------------------------------------------------------------------------------------
def plan(j, tff, rate):
    """Output j: field m = j at rate 2, 2 j at rate 1; frame k holds fields 2k and 2k + 1."""
    m = j if rate == 2 else 2 * j
    holder = lambda f: next(k for k in range(f // 2 + 2) if f in (2 * k, 2 * k + 1))
    return {"field": m, "parity": par(m, tff), "cur": holder(m), "prev": holder(m - 1) if m else -1, "next": holder(m + 1)}


def stream_outputs(n_frames, tff, rate):
    """For a stream of n_frames frames: a list of n_frames + 1 lists of (plan, mode) — entry n what the push of frame n returns, the
    last entry the flush.  A field goes out as soon as the frame of its successor has been pushed; field 0 has no predecessor (INTRA);
    the flush returns, in INTRA, the fields of pushed frames that still wait for a successor."""
    fields = list(range(2 * n_frames)) if rate == 2 else list(range(0, 2 * n_frames, 2))
    out = [[] for _ in range(n_frames + 1)]
    for j, m in enumerate(fields):
        p = plan(j, tff, rate)
        assert p["field"] == m
        if p["next"] < n_frames:
            out[max(p["next"], p["cur"])].append((p, INTRA if m == 0 else MOTION))
        else:
            out[n_frames].append((p, INTRA))
    return out
