#!/usr/bin/env python3
"""The probe measure (libfldr_probe.so) at 1920x1080 NV12 and 3840x2160 P010 (BT.709 limited), on a moving texture
(fldr_harness.synthetic_pair, as tools/bench_pulldown.py's clip) telecined 3:2 top field first, in one process:

  * µs per fldr_probe_measure (cur, prev and next all given: 3 luma planes, each byte loaded once) beside µs for the TWO
    fldr_pulldown_measure calls (anchor 0 and anchor 1: 5 luma planes) that give the same comb and field words without the order sums,
    and beside a device copy of the three luma planes (3 read, 3 written); each call's launches back to back on one stream —
    --measures calls captured into one graph, the graph replayed --replays times between two device events, so that the host's cost of
    a call stays out —, the three alternated --alternations times; with the bytes each moves, GB/s and the ratios.

    python tools/bench_probe.py [--alternations 3] [--measures 100] [--replays 10] [--out profiles/probe.json]

Before any timing the probe measure is compared with its oracle (tests/probe_oracle.py) and with the two pulldown measures."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fldr-vfi_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import fldr_probe  # noqa: E402
import fldr_pulldown  # noqa: E402
import fldr_video  # noqa: E402
import probe_oracle as O  # noqa: E402
import pulldown_frames as PF  # noqa: E402
from bench_pulldown import MAT, RNG, fmt_name, make_clip, timed, to_dev  # noqa: E402

CASES = [(1080, 1920, 8), (2160, 3840, 10)]


def measure_case(a, dev, frames, depth, H, W, res):
    """frames: three consecutive container frames (host)."""
    fmt = fldr_video.Format("nv12", MAT, RNG, depth)
    b = 1 if depth == 8 else 2
    prev, cur, nxt = frames
    d = [to_dev(f, dev) for f in (cur, prev, nxt)]
    st = fldr_probe.measure_state(dev)
    ps = [fldr_pulldown.measure_state(dev) for _ in range(2)]
    got = fldr_probe.measure(d[0], d[1], d[2], fmt, state=st)
    if got != dict(O.measure(cur, prev, nxt, ("nv12", depth)), reserved=[0] * 12):
        raise SystemExit("the probe measure differs from the oracle's: %r" % (got,))
    for q in (0, 1):
        p = fldr_pulldown.measure(d[0], d[1], d[2], fmt, q, state=ps[q])
        if (got["comb"][q], got["max_tile_comb"][q], got["field_sad"][q], got["field_moving_tiles"][q]) != \
           (p["comb"], p["max_tile_comb"], p["dup_sad"], p["dup_moving_tiles"]):
            raise SystemExit("the probe measure differs from the pulldown measure at anchor %d" % q)
    lumas = [f[0] for f in d]
    outs = [torch.empty_like(y) for y in lumas]

    def two_pulldown():
        for q in (0, 1):
            fldr_pulldown.measure(d[0], d[1], d[2], fmt, q, state=ps[q], read=False)

    def copy():
        for o, y in zip(outs, lumas):
            o.copy_(y)
    m = timed({"probe_measure": lambda: fldr_probe.measure(d[0], d[1], d[2], fmt, state=st, read=False),
               "two_pulldown_measures": two_pulldown, "copy_three_luma_planes": copy}, a, a.measures)
    med = {k: statistics.median(v) for k, v in m.items()}
    luma = H * W * b
    moved = {"probe_measure": 3 * luma, "two_pulldown_measures": 5 * luma, "copy_three_luma_planes": 6 * luma}
    res["measure"]["%dx%d_%s" % (W, H, fmt_name(depth))] = {
        "us_per_call": med, "runs": m, "bytes_moved": moved, "gb_per_s": {k: moved[k] / med[k] * 1e-3 for k in med},
        "probe_over_two_pulldown_measures": med["probe_measure"] / med["two_pulldown_measures"],
        "probe_over_copy": med["probe_measure"] / med["copy_three_luma_planes"], "result": got}
    print("%dx%d %s: probe measure %.1f us, two pulldown measures %.1f us, copy of three luma planes %.1f us" % (
        W, H, fmt_name(depth), med["probe_measure"], med["two_pulldown_measures"], med["copy_three_luma_planes"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--measures", type=int, default=100, help="calls captured into one graph")
    ap.add_argument("--replays", type=int, default=10, help="replays of the graph per timed loop")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "alternations": a.alternations, "calls_per_graph": a.measures, "replays_per_loop": a.replays,
           "measure": {}}
    for H, W, depth in CASES:
        frames, _ = PF.telecine32(make_clip(4, depth, H, W), 0)
        measure_case(a, dev, frames[1:4], depth, H, W, res)              # frame 2 (B top, C bottom) between its neighbours
        if a.out:                                                        # written after every format: a cut-off run keeps what it measured
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: v for k, v in res.items() if k != "measure"}))


if __name__ == "__main__":
    main()
