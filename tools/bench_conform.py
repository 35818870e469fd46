#!/usr/bin/env python3
"""The conform kernel (libfldr_conform.so) on a moving texture (fldr_harness.synthetic_pair, as tools/bench_pulldown.py's clip), in one
process and ONE run: µs per fldr_conform_frame of a whole frame at 1920x1080 and 3840x2160 for

  * an equal-matrix conversion, NV12 -> P010 (BT.709 limited on both sides): the luma pass reads no chroma;
  * a matrix-changing one, NV12 BT.601 -> P010 BT.709: every luma run reads two chroma rows as well;
  * a 10 -> 8 one with the ordered dither, P010 -> NV12;
  * and once, at its own size, a 720x576 -> 1024x576 pillarbox (NV12 BT.601 -> P010 BT.709, the picture at x = 152),

each beside a device-to-device copy of the bytes the kernel moves at least once (the source read plus the canvas written) and beside the
video library's two converters of the same run — fldr_video_debug_to_planar on the source format (it converts a PAIR: its figure is
halved) plus fldr_video_debug_from_planar on the output format, which together are the only way to change a format without this library.
The two converters are timed as kernels only: the planar buffer the second reads is not the first's output where the depths differ, and
nothing pads the picture for them.  --calls calls are captured back to back into one graph on one stream, the graph is replayed --replays
times between two device events, so that the host's cost of a call stays out; the candidates are alternated --alternations times.

    python tools/bench_conform.py [--alternations 3] [--calls 20] [--replays 5] [--out profiles/conform.json]

Before any timing every conform is compared with its oracle (tests/conform_oracle.py), byte for byte."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fldr-vfi_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import conform_oracle as CO  # noqa: E402
import fldr_conform  # noqa: E402
import fldr_video  # noqa: E402
import rate_frames as RF  # noqa: E402
from bench_pulldown import timed, to_dev, to_host  # noqa: E402
import fldr_harness as Hn  # noqa: E402

SIZES = [(1080, 1920), (2160, 3840)]
# name -> (source format, output format, dither)
CASES = {
    "equal_matrix_nv12_to_p010": (("nv12", "bt709", "limited", 8), ("nv12", "bt709", "limited", 10), False),
    "matrix_601_nv12_to_709_p010": (("nv12", "bt601", "limited", 8), ("nv12", "bt709", "limited", 10), False),
    "dithered_p010_to_nv12": (("nv12", "bt709", "limited", 10), ("nv12", "bt709", "limited", 8), True),
}
PILLARBOX = ((576, 720), (576, 1024), (152, 0), ("nv12", "bt601", "limited", 8), ("nv12", "bt709", "limited", 10))


def frame_bytes(size, depth):
    return size[0] * size[1] * (1 if depth == 8 else 2) * 3 // 2


def source(fmt, H, W):
    u8 = Hn.synthetic_pair(H, W, seed=7).numpy()[0]                        # [3, H, W]
    return RF.planes_of_bgr(np.ascontiguousarray(u8), fmt[0], fmt[3], fmt[1], fmt[2])


def one(a, dev, name, in_size, out_size, at, src, dst, dither, res):
    fi, fo = fldr_video.Format(*src), fldr_video.Format(*dst)
    host = source(src, in_size[0], in_size[1])
    ins = to_dev(host, dev)
    out = fldr_video.empty_frame(fo, out_size[0], out_size[1], dev)
    fldr_conform.frame(ins, fi, out, fo, at, dither)
    torch.cuda.synchronize()
    want = CO.conform(host, src, dst, out_size, at, int(dither))
    if not all(np.array_equal(x, y) for x, y in zip(to_host(out), want)):
        raise SystemExit("the conform %s at %r differs from the oracle's" % (name, in_size))
    moved = frame_bytes(in_size, src[3]) + frame_bytes(out_size, dst[3])
    a_buf = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
    b_buf = torch.empty_like(a_buf)
    # the route through planar BGR: a pair in, in the source format; one frame out, from a planar buffer of the output's depth and size
    pair_in = torch.empty(2, 3, in_size[0], in_size[1], dtype=fldr_video.plane_dtype(fi), device=dev)
    planar_out = torch.zeros(3, out_size[0], out_size[1], dtype=fldr_video.plane_dtype(fo), device=dev)
    calls = {"conform": lambda: fldr_conform.frame(ins, fi, out, fo, at, dither),
             "copy_same_bytes": lambda: b_buf.copy_(a_buf),
             "to_planar_of_a_pair": lambda: fldr_video.debug_to_planar((ins, ins), fi, pair_in),
             "from_planar": lambda: fldr_video.debug_from_planar(planar_out, fo, out)}
    runs = timed(calls, a, a.calls)
    med = {k: statistics.median(v) for k, v in runs.items()}
    through_bgr = med["to_planar_of_a_pair"] / 2 + med["from_planar"]
    # with different matrices every luma row loads two chroma rows as well: 2 rows x W / 2 columns x 2 components per luma row
    read = frame_bytes(in_size, src[3]) + (2 * in_size[0] * in_size[1] * (1 if src[3] == 8 else 2) if src[1] != dst[1] else 0)
    entry = {"in_size": in_size, "out_size": out_size, "at": at, "source": "-".join(map(str, src)), "output": "-".join(map(str, dst)), "dither": bool(dither),
             "us_per_call": med, "runs": runs, "bytes_moved_at_least": moved, "bytes_loaded_and_stored_by_the_lanes": read + frame_bytes(out_size, dst[3]),
             "through_planar_bgr_us": through_bgr, "over_copy": med["conform"] / med["copy_same_bytes"], "over_planar_bgr": med["conform"] / through_bgr,
             "gb_per_s_of_bytes_moved": moved / med["conform"] / 1e3}
    res["kernels"]["%s_%dx%d" % (name, in_size[1], in_size[0])] = entry
    print("%s %dx%d: conform %.1f us, copy of the same bytes %.1f us (x %.2f), through planar BGR %.1f us (x %.2f)" % (
        name, in_size[1], in_size[0], med["conform"], med["copy_same_bytes"], entry["over_copy"], through_bgr, entry["over_planar_bgr"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20, help="calls captured into one graph")
    ap.add_argument("--replays", type=int, default=5, help="replays of the graph per timed loop")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "alternations": a.alternations, "calls_per_graph": a.calls, "replays_per_loop": a.replays,
           "run_bytes": fldr_conform.RUN_BYTES, "threads": fldr_conform.THREADS, "kernels": {}}

    def save():
        if a.out:                                                            # written after every part: a cut-off run keeps what it measured
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
    for size in SIZES:
        for name, (src, dst, dither) in CASES.items():
            one(a, dev, name, size, size, (0, 0), src, dst, dither, res)
            save()
    in_size, out_size, at, src, dst = PILLARBOX
    one(a, dev, "pillarbox_601_nv12_to_709_p010", in_size, out_size, at, src, dst, False, res)
    save()
    print(json.dumps({k: v for k, v in res.items() if k != "kernels"}))


if __name__ == "__main__":
    main()
