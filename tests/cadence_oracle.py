"""The numpy statement of include/fldr_cadence.h: the repeat measure (fldr_repeat_measure) and the choice of the frames a cadence
stream drops, in integers.

y8(sample) is tests/scene_oracle.py's.  The luma plane is cut into tiles of 32 x 32 samples, partial at the right and bottom edges;
tiles_x = ceil(W / 32), tile index = ty * tiles_x + tx.
    tile_sad(i)  = sum over tile i of |y8(I0) - y8(I1)|
    sad          = sum of all tile_sad;  max_tile_sad = the largest, max_tile = the lowest index that attains it
    moving_tiles = number of tiles with tile_sad >= tile_sad_min;  repeat = moving_tiles == 0
Frame n of a stream belongs to cycle n // cycle; its key is (max_tile_sad, sad) of the pair (n - 1, n); frame 0 has none and is never
dropped.  Of every complete cycle the `drop` frames with the smallest keys go, the lower frame first among equals; of a partial last
cycle of m frames, floor(m * drop / cycle)."""
import os
import re

import numpy as np

import scene_oracle as S

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fldr_cadence.h")
TILE = 32
KEYS = ("sad", "max_tile_sad", "max_tile", "moving_tiles", "repeat")


def default():
    """FLDR_REPEAT_TILE_SAD_DEFAULT, parsed from the header."""
    return int(re.search(r"#define\s+FLDR_REPEAT_TILE_SAD_DEFAULT\s+(\d+)", open(HEADER).read()).group(1))


def tile_sads(planes0, planes1, fmt=("nv12", 8)):
    """tile_sad of every tile, an int64 array [tiles_y, tiles_x]."""
    layout, depth = (fmt.name, fmt.bits) if hasattr(fmt, "bits") else fmt
    d = np.abs(S.y8(planes0[0], layout, depth) - S.y8(planes1[0], layout, depth))
    H, W = d.shape
    ty, tx = -(-H // TILE), -(-W // TILE)
    full = np.zeros((ty * TILE, tx * TILE), np.int64)
    full[:H, :W] = d
    return full.reshape(ty, TILE, tx, TILE).sum(axis=(1, 3))


def measure(planes0, planes1, fmt=("nv12", 8), tile_sad_min=0):
    """planes0 / planes1: the planes of the two frames (only [0] is read); tile_sad_min: 0 or None = the header's default."""
    t = tile_sads(planes0, planes1, fmt).ravel()
    moving = int((t >= (int(tile_sad_min or 0) or default())).sum())
    return {"sad": int(t.sum()), "max_tile_sad": int(t.max()), "max_tile": int(t.argmax()),       # argmax: the first of equal maxima
            "moving_tiles": moving, "repeat": int(moving == 0)}


ZERO = {k: 0 for k in KEYS}


def drops(measures, n_drop):
    """The positions, within one cycle, of the n_drop frames to drop.  measures: the cycle's result dicts, None for a frame without a
    key (frame 0 of the stream)."""
    order = sorted((m["max_tile_sad"], m["sad"], k) for k, m in enumerate(measures) if m is not None)
    return sorted(k for _, _, k in order[:n_drop])


def survivors(measures, cycle, drop):
    """measures[n]: the result dict of the pair (n - 1, n) for n >= 1 (measures[0] is ignored) of a stream that is pushed whole and then
    flushed.  -> (kept frame numbers, reports): one report per cycle, the partial last one included, as fldr_cadence_report without
    its cut_mask."""
    N = len(measures)
    kept, reports = [], []
    for first in range(0, N, cycle):
        ms = [None if n == 0 else measures[n] for n in range(first, min(first + cycle, N))]
        m = len(ms)
        gone = drops(ms, drop if m == cycle else m * drop // cycle)
        kept += [first + k for k in range(m) if k not in gone]
        reports.append({"first_frame": first, "n_frames": m, "dropped_mask": sum(1 << k for k in gone),
                        "moving_dropped": sum(1 for k in gone if not ms[k]["repeat"]),
                        "still_kept": sum(1 for k in range(m) if k not in gone and ms[k] is not None and ms[k]["repeat"]),
                        "measure": [dict(ZERO) if x is None else {k: x[k] for k in KEYS} for x in ms]})
    return kept, reports
