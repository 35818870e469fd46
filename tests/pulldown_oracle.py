"""The numpy statement of include/fldr_pulldown.h: the field-matching measure and its decision (fldr_pulldown_measure), the assembly of
the matched frame (fldr_pulldown_assemble) and the schedule of a pulldown stream (match, drop, survivors, inner rate), in integers.
Written from the header, not from the kernels.

y8(sample) is tests/scene_oracle.py's.  The anchor parity q names the rows y % 2 == q of cur that every candidate keeps; candidate k
takes the other rows from S_k: C = 0 cur, P = 1 the previous frame, N = 2 the next.  The luma plane is cut into tiles of 32 x 32
samples, partial at the right and bottom edges; tiles_x = ceil(W / 32), tile index = ty * tiles_x + tx.
    combed sample (rows y % 2 != q, 1 <= y <= H - 2): (a - m) * (b - m) > comb_thresh^2, a = y8(cur[y-1]), b = y8(cur[y+1]), m = y8(S_k[y])
    comb[k] = their number, max_tile_comb[k] = the largest per tile, max_tile[k] = the lowest index that attains it
    dup_*: the sum of |y8(cur) - y8(prev)| over the rows y % 2 == q, per tile; dup_moving_tiles = tiles with a sum >= tile_sad_min
    match = the allowed candidate with the smallest (max_tile_comb, comb), ties to C, P, N in that order
    combed = max_tile_comb[match] >= comb_tile_min
A candidate without a frame is not measured (zeros); all dup_* are 0 without prev."""
import os
import re
from fractions import Fraction

import numpy as np

import scene_oracle as S

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fldr_pulldown.h")
TILE = 32
C, P, N = 0, 1, 2
KEEP, AVERAGE = 0, 1
KEYS = ("match", "combed", "comb", "max_tile_comb", "max_tile", "dup_sad", "dup_max_tile_sad", "dup_max_tile", "dup_moving_tiles")


def defaults():
    """(comb_thresh, comb_tile_min, tile_sad_min), parsed from the header."""
    text = open(HEADER).read()
    return tuple(int(re.search(r"#define\s+FLDR_PULLDOWN_%s_DEFAULT\s+(\d+)" % n, text).group(1)) for n in ("COMB_THRESH", "COMB_TILE", "TILE_SAD"))


def _fmt(fmt):
    return (fmt.name, fmt.bits) if hasattr(fmt, "bits") else fmt


def _tiles(full):
    """Per-tile sums of an [H, W] integer array -> [tiles_y, tiles_x]."""
    H, W = full.shape
    ty, tx = -(-H // TILE), -(-W // TILE)
    pad = np.zeros((ty * TILE, tx * TILE), np.int64)
    pad[:H, :W] = full
    return pad.reshape(ty, TILE, tx, TILE).sum(axis=(1, 3))


def comb_map(cur, src, q, comb_thresh, fmt=("nv12", 8)):
    """1 where a sample of candidate `src` is combed, an int64 array [H, W] (0 on the anchor rows and on rows 0 and H - 1)."""
    layout, depth = _fmt(fmt)
    c, s = S.y8(cur[0], layout, depth), S.y8(src[0], layout, depth)
    H, W = c.shape
    out = np.zeros((H, W), np.int64)
    y = np.array([r for r in range(1, H - 1) if r % 2 != q], np.int64)
    out[y] = (c[y - 1] - s[y]) * (c[y + 1] - s[y]) > comb_thresh * comb_thresh
    return out


def measure(cur, prev, nxt, fmt=("nv12", 8), q=0, comb_thresh=0, comb_tile_min=0, tile_sad_min=0, allowed=0):
    """cur / prev / nxt: the planes of the three frames (only [0] is read; prev / nxt may be None); zeros = the header's defaults."""
    layout, depth = _fmt(fmt)
    d = defaults()
    comb_thresh, comb_tile_min, tile_sad_min, allowed = comb_thresh or d[0], comb_tile_min or d[1], tile_sad_min or d[2], allowed or 7
    comb, max_tile_comb, max_tile = [0, 0, 0], [0, 0, 0], [0, 0, 0]
    for k, src in enumerate((cur, prev, nxt)):
        if src is None:
            assert not allowed >> k & 1, "candidate %d is allowed but has no frame" % k
            continue
        t = _tiles(comb_map(cur, src, q, comb_thresh, (layout, depth))).ravel()
        comb[k], max_tile_comb[k], max_tile[k] = int(t.sum()), int(t.max()), int(t.argmax())     # argmax: the first of equal maxima
    out = {"comb": comb, "max_tile_comb": max_tile_comb, "max_tile": max_tile,
           "dup_sad": 0, "dup_max_tile_sad": 0, "dup_max_tile": 0, "dup_moving_tiles": 0}
    if prev is not None:
        diff = np.abs(S.y8(cur[0], layout, depth) - S.y8(prev[0], layout, depth))
        diff[1 - q::2] = 0
        t = _tiles(diff).ravel()
        out.update(dup_sad=int(t.sum()), dup_max_tile_sad=int(t.max()), dup_max_tile=int(t.argmax()), dup_moving_tiles=int((t >= tile_sad_min).sum()))
    out["match"] = min((k for k in range(3) if allowed >> k & 1), key=lambda k: (max_tile_comb[k], comb[k], k))
    out["combed"] = int(max_tile_comb[out["match"]] >= comb_tile_min)
    return out


def _value(p, layout, depth):
    p = p.astype(np.int64)
    return p if depth != 10 else (p >> 6 if layout == "nv12" else p & 0x3ff)


def assemble(cur, prev, nxt, fmt=("nv12", 8), q=0, match=0, combed=0, post=KEEP):
    """The matched frame, every plane: rows y % 2 == q from cur, the others from S_match as they are — or, with post = AVERAGE and
    combed, the line average of cur's rows y - 1 and y + 1 (the one neighbour twice at the plane's first and last row)."""
    layout, depth = _fmt(fmt)
    src = (cur, prev, nxt)[match]
    out = []
    for p in range(len(cur)):
        o = cur[p].copy()
        rows = o.shape[0]
        if post == AVERAGE and combed:
            v = _value(cur[p], layout, depth)
            for y in range(1 - q, rows, 2):
                a = v[1] if y == 0 else v[y - 1]
                b = v[y - 1] if y == rows - 1 else v[y + 1]
                avg = (a + b + 1) >> 1
                o[y] = (avg << 6 if (depth == 10 and layout == "nv12") else avg).astype(o.dtype)
        else:
            o[1 - q::2] = src[p][1 - q::2]
        out.append(o)
    return tuple(out)


# ---- the schedule ------------------------------------------------------------------------------------------------------------------------
def inner_rate(in_rate, cycle, drop):
    q = Fraction(*in_rate) if isinstance(in_rate, tuple) else Fraction(in_rate)
    return q * (cycle - drop) / cycle


def match_stream(frames, fmt=("nv12", 8), q=0, post=KEEP, **params):
    """Every frame of a stream that is pushed whole and then flushed, matched: frame n against prev = n - 1 and next = n + 1; frame 0
    with allowed = C | N, the last with C | P (each intersected with params' allowed; C alone where that leaves nothing).
    -> (results, matched frames)."""
    allowed = params.pop("allowed", 0) or 7
    results, matched = [], []
    for n, cur in enumerate(frames):
        prev = frames[n - 1] if n else None
        nxt = frames[n + 1] if n + 1 < len(frames) else None
        a = allowed & (1 | (2 if prev is not None else 0) | (4 if nxt is not None else 0)) or 1
        r = measure(cur, prev, nxt, fmt, q, allowed=a, **params)
        results.append(r)
        matched.append(assemble(cur, prev, nxt, fmt, q, r["match"], r["combed"], post))
    return results, matched


def drops(results, n_drop):
    """The positions, within one cycle, of the n_drop frames to drop.  results: the cycle's result dicts, None for a frame without a
    key (frame 0 of the stream)."""
    order = sorted((r["dup_max_tile_sad"], r["dup_sad"], k) for k, r in enumerate(results) if r is not None)
    return sorted(k for _, _, k in order[:n_drop])


def survivors(results, cycle, drop):
    """results[n]: the measure of stream frame n.  -> (kept frame numbers, reports): one report per cycle, the partial last one
    included, as fldr_pulldown_report without its cut_mask."""
    Nf = len(results)
    kept, reports = [], []
    for first in range(0, Nf, cycle):
        rs = results[first:first + cycle]
        keyed = [None if first + k == 0 else r for k, r in enumerate(rs)]
        m = len(rs)
        gone = drops(keyed, drop if m == cycle else m * drop // cycle)
        kept += [first + k for k in range(m) if k not in gone]
        reports.append({"first_frame": first, "n_frames": m, "dropped_mask": sum(1 << k for k in gone),
                        "combed_mask": sum(r["combed"] << k for k, r in enumerate(rs)),
                        "moving_dropped": sum(1 for k in gone if rs[k]["dup_moving_tiles"]),
                        "still_kept": sum(1 for k in range(m) if k not in gone and keyed[k] is not None and not rs[k]["dup_moving_tiles"]),
                        "match": [r["match"] for r in rs],
                        "measure": [{k: r[k] for k in KEYS} for r in rs]})
    return kept, reports
