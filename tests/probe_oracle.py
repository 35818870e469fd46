"""The numpy statement of include/fldr_probe.h: the probe measure (fldr_probe_measure) and the classifier (fldr_probe_frame_class,
fldr_probe_classify), in integers.  Written from the header, not from the C.

y8(sample) is tests/scene_oracle.py's.  The luma plane is cut into tiles of 32 x 32 samples, partial at the right and bottom edges;
tiles_x = ceil(W / 32), tile index = ty * tiles_x + tx.  S_k: C = 0 cur, P = 1 the previous frame, N = 2 the next.
    comb[q][k], max_tile_comb[q][k], max_tile[q][k]: the combed samples of candidate k on the rows y % 2 != q, 1 <= y <= H - 2:
        (a - m) * (b - m) > comb_thresh^2, a = y8(cur[y-1]), b = y8(cur[y+1]), m = y8(S_k[y])  — tests/pulldown_oracle.py's comb_map
    field_*[p]: |y8(cur) - y8(prev)| over the rows y % 2 == p, per tile; field_moving_tiles[p] = tiles with a sum >= tile_sad_min
    frame_moving_tiles = tiles whose two field sums together are >= frame_tile_sad_min; repeat = prev given and none such
    lap[k][p] = sum of |a + b - 2 m| over the rows y % 2 == p, 1 <= y <= H - 2; tff_sum = lap[P][1] + lap[N][0], bff_sum = lap[P][0] + lap[N][1]
A frame that is None is not measured: its words are 0, and tff_sum / bff_sum are 0 unless both are given."""
import os
import re

import numpy as np

import cadence_oracle as CO
import pulldown_oracle as PO
import scene_oracle as S

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fldr_probe.h")
TILE = 32
assert CO.TILE == PO.TILE == TILE                # one tiling for the repeat, pulldown and probe measures
C, P, N = 0, 1, 2
UNKNOWN, PROGRESSIVE, FILM, INTERLACED, MIXED = range(5)
STILL, F_PROG, F_FILM, F_VIDEO = range(4)
MAX_CYCLE = 16
KEYS = ("comb", "max_tile_comb", "max_tile", "field_sad", "field_max_tile_sad", "field_max_tile", "field_moving_tiles", "frame_moving_tiles",
        "repeat", "lap", "tff_sum", "bff_sum")
VERDICT_KEYS = ("kind", "tff", "mixed", "cycle", "drop", "anchor", "irregular", "confirmed", "n_frames", "n_moved", "n_still", "n_prog",
                "n_film", "n_video", "votes_tff", "votes_bff")


def defaults():
    """{comb_thresh, comb_tile_min, tile_sad_min, frame_tile_sad_min, min_moved}, parsed from the header."""
    text = open(HEADER).read()
    names = {"comb_thresh": "COMB_THRESH", "comb_tile_min": "COMB_TILE", "tile_sad_min": "TILE_SAD", "frame_tile_sad_min": "FRAME_TILE_SAD",
             "min_moved": "MIN_MOVED"}
    return {k: int(re.search(r"#define\s+FLDR_PROBE_%s_DEFAULT\s+(\d+)" % n, text).group(1)) for k, n in names.items()}


def _params(kw):
    p = dict(defaults(), max_outliers=0, anchor=0)
    for k, v in kw.items():
        assert k in p, k
        if v or k in ("max_outliers", "anchor"):
            p[k] = int(v)
    return p


def lap_map(cur, src, fmt=("nv12", 8)):
    """|a + b - 2 m| of every sample, an int64 array [H, W] (0 on rows 0 and H - 1)."""
    layout, depth = PO._fmt(fmt)
    c, s = S.y8(cur[0], layout, depth).astype(np.int64), S.y8(src[0], layout, depth).astype(np.int64)
    out = np.zeros(c.shape, np.int64)
    out[1:-1] = np.abs(c[:-2] + c[2:] - 2 * s[1:-1])
    return out


def measure(cur, prev, nxt, fmt=("nv12", 8), **params):
    """cur / prev / nxt: the planes of the three frames (only [0] is read; prev / nxt may be None); parameters not given or 0 = the
    header's defaults."""
    layout, depth = PO._fmt(fmt)
    p = _params(params)
    out = {"comb": [[0] * 3, [0] * 3], "max_tile_comb": [[0] * 3, [0] * 3], "max_tile": [[0] * 3, [0] * 3], "field_sad": [0, 0],
           "field_max_tile_sad": [0, 0], "field_max_tile": [0, 0], "field_moving_tiles": [0, 0], "frame_moving_tiles": 0, "repeat": 0,
           "lap": [[0, 0] for _ in range(3)], "tff_sum": 0, "bff_sum": 0}
    for k, src in enumerate((cur, prev, nxt)):
        if src is None:
            continue
        for q in (0, 1):
            t = PO._tiles(PO.comb_map(cur, src, q, p["comb_thresh"], (layout, depth))).ravel()
            out["comb"][q][k], out["max_tile_comb"][q][k], out["max_tile"][q][k] = int(t.sum()), int(t.max()), int(t.argmax())
        full = lap_map(cur, src, (layout, depth))
        out["lap"][k] = [int(full[0::2].sum()), int(full[1::2].sum())]
    if prev is not None:
        diff = np.abs(S.y8(cur[0], layout, depth).astype(np.int64) - S.y8(prev[0], layout, depth).astype(np.int64))
        fields = []
        for par in (0, 1):
            d = diff.copy()
            d[1 - par::2] = 0
            t = PO._tiles(d).ravel()
            fields.append(t)
            out["field_sad"][par], out["field_max_tile_sad"][par], out["field_max_tile"][par] = int(t.sum()), int(t.max()), int(t.argmax())
            out["field_moving_tiles"][par] = int((t >= p["tile_sad_min"]).sum())
        out["frame_moving_tiles"] = int((fields[0] + fields[1] >= p["frame_tile_sad_min"]).sum())
        out["repeat"] = int(out["frame_moving_tiles"] == 0)
    if prev is not None and nxt is not None:
        out["tff_sum"] = out["lap"][P][1] + out["lap"][N][0]
        out["bff_sum"] = out["lap"][P][0] + out["lap"][N][1]
    return out


def measure_stream(frames, fmt=("nv12", 8), **params):
    """The results of frames 1 .. len - 2, each against both neighbours: what a probe stream pushed all of `frames` holds (window
    permitting)."""
    return [measure(frames[n], frames[n - 1], frames[n + 1], fmt, **params) for n in range(1, len(frames) - 1)]


# ---- the classifier ------------------------------------------------------------------------------------------------------------------------
def frame_class(r, **params):
    p = _params(params)
    if r["frame_moving_tiles"] == 0:
        return STILL
    m = r["max_tile_comb"]
    if m[0][C] < p["comb_tile_min"] and m[1][C] < p["comb_tile_min"]:
        return F_PROG
    if all(min(m[q]) < p["comb_tile_min"] for q in (0, 1)):
        return F_FILM
    return F_VIDEO


def classify(results, **params):
    p = _params(params)
    M = len(results)
    classes = [frame_class(r, **params) for r in results]
    v = {k: 0 for k in VERDICT_KEYS}
    v.update(kind=UNKNOWN, tff=-1, cycle=1, anchor=p["anchor"], n_frames=M, n_still=classes.count(STILL), n_prog=classes.count(F_PROG),
             n_film=classes.count(F_FILM), n_video=classes.count(F_VIDEO))
    video = [r for r, c in zip(results, classes) if c == F_VIDEO]
    v["votes_tff"] = sum(1 for r in video if r["tff_sum"] < r["bff_sum"])
    v["votes_bff"] = sum(1 for r in video if r["tff_sum"] > r["bff_sum"])
    v["n_moved"] = M - v["n_still"]
    if v["n_moved"] < p["min_moved"]:
        return v
    n_prog, n_film, n_video = (n if n > p["max_outliers"] else 0 for n in (v["n_prog"], v["n_film"], v["n_video"]))
    if n_video == 0 and n_film == 0:
        v["kind"] = PROGRESSIVE
    elif n_video == 0:
        v["kind"] = FILM
    elif n_film == 0:
        v["kind"] = INTERLACED
        v["tff"] = 1 if v["votes_tff"] > v["votes_bff"] else 0 if v["votes_tff"] < v["votes_bff"] else -1
        v["mixed"] = int(n_prog > 0)
    else:
        v["kind"] = MIXED
    if v["kind"] == PROGRESSIVE:
        r = [int(c == STILL) for c in classes]
    elif v["kind"] == FILM:
        r = [int(x["field_moving_tiles"][p["anchor"]] == 0) for x in results]
    else:
        return v
    if not any(r):
        return v
    cycles = [c for c in range(1, MAX_CYCLE + 1) if c < M and all(r[n] == r[n + c] for n in range(M - c))]
    if not cycles:
        v["irregular"] = 1
        return v
    c = cycles[0]
    v.update(cycle=c, drop=sum(r[:c]), confirmed=sum(1 for n in range(M - c) if r[n] and r[n + c]))
    return v
