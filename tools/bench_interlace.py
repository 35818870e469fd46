#!/usr/bin/env python3
"""The interlace API (libfldr_interlace.so) at 1920x1080 NV12 and 3840x2160 P010 (BT.709 limited), on a moving texture
(fldr_harness.synthetic_pair, as tools/bench_pulldown.py's clip), in one process:

  * µs per fldr_interlace_weave of a whole frame (both sources given) under each of the three filters, beside its two yardsticks of the
    same run: a device-to-device copy of the bytes the kernel reads once plus writes — two half frames in and one frame out under NONE
    (a copy of one frame), two frames in and one out under the filters (a copy of a frame and a half) —, and fldr_pulldown_assemble, which
    under NONE moves the same bytes.  --calls calls are captured back to back into one graph on one stream, the graph is replayed
    --replays times between two device events, so that the host's cost of a call stays out; the candidates are alternated
    --alternations times;
  * ms per PUSHED frame of an interlace stream, 24 -> 30i (four fields in five interpolated) and 50 -> 25i (no forward at all), beside
    fldr_rate 24 -> 60 and 50 -> 50 pushed the same frames — the same fields, returned as whole frames —, alternated the same way, the C
    entry points called directly (host frames in and out: includes PCIe and host copies).

    python tools/bench_interlace.py [--frames 6] [--alternations 3] [--calls 100] [--replays 10] [--out profiles/interlace.json]

Before any timing every weave is compared with its oracle (tests/interlace_oracle.py) and the 24 -> 30i stream's frames with the oracle's
weave of the converter's, byte for byte."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fldr-vfi_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import fldr_harness as Hn  # noqa: E402
import fldr_interlace  # noqa: E402
import fldr_model  # noqa: E402
import fldr_pulldown  # noqa: E402
import fldr_rate  # noqa: E402
import fldr_video  # noqa: E402
import interlace_oracle as IO  # noqa: E402
from bench_pulldown import MAT, RNG, fmt_name, make_clip, timed, to_dev, to_host  # noqa: E402

CASES = [(1080, 1920, 8), (2160, 3840, 10)]
FILTERS = {"none": fldr_interlace.NONE, "linear": fldr_interlace.LINEAR, "complex": fldr_interlace.COMPLEX}


def kernels_alone(a, dev, clip, depth, H, W, res):
    fmt = fldr_video.Format("nv12", MAT, RNG, depth)
    b = 1 if depth == 8 else 2
    even, odd = to_dev(clip[0], dev), to_dev(clip[1], dev)
    out = tuple(torch.empty_like(p) for p in even)
    for name, filt in FILTERS.items():
        fldr_interlace.weave(even, odd, out, fmt, filt)
        torch.cuda.synchronize()
        if not all(np.array_equal(x, y) for x, y in zip(to_host(out), IO.weave(clip[0], clip[1], "nv12", depth, filt))):
            raise SystemExit("the %s weave differs from the oracle's" % name)
    frame_bytes = H * W * b * 3 // 2
    one, half_more = (torch.empty(frame_bytes * k // 2, dtype=torch.uint8, device=dev) for k in (2, 3))
    one_dst, half_more_dst = torch.empty_like(one), torch.empty_like(half_more)
    calls = {"weave_" + name: (lambda f=filt: fldr_interlace.weave(even, odd, out, fmt, f)) for name, filt in FILTERS.items()}
    calls["copy_1_frame"] = lambda: one_dst.copy_(one)
    calls["copy_1.5_frames"] = lambda: half_more_dst.copy_(half_more)
    calls["pulldown_assemble"] = lambda: fldr_pulldown.assemble(even, odd, None, out, fmt, 0, 1, 0, None, fldr_pulldown.POST_KEEP)
    runs = timed(calls, a, a.calls)
    med = {k: statistics.median(v) for k, v in runs.items()}
    moved = {"weave_none": 2 * frame_bytes, "weave_linear": 3 * frame_bytes, "weave_complex": 3 * frame_bytes, "copy_1_frame": 2 * frame_bytes,
             "copy_1.5_frames": 3 * frame_bytes, "pulldown_assemble": 2 * frame_bytes}
    entry = {"us_per_call": med, "runs": runs, "bytes_moved": moved, "gb_per_s": {k: moved[k] / med[k] * 1e-3 for k in med},
             "none_over_copy": med["weave_none"] / med["copy_1_frame"], "none_over_pulldown_assemble": med["weave_none"] / med["pulldown_assemble"],
             "linear_over_copy": med["weave_linear"] / med["copy_1.5_frames"], "complex_over_copy": med["weave_complex"] / med["copy_1.5_frames"],
             "linear_over_none": med["weave_linear"] / med["weave_none"], "complex_over_none": med["weave_complex"] / med["weave_none"]}
    res["kernels_alone"]["%dx%d_%s" % (W, H, fmt_name(depth))] = entry
    print("%dx%d %s: weave none %.1f us (copy %.1f, pulldown assemble %.1f), linear %.1f, complex %.1f (copy of 1.5 frames %.1f)" % (
        W, H, fmt_name(depth), med["weave_none"], med["copy_1_frame"], med["pulldown_assemble"], med["weave_linear"], med["weave_complex"],
        med["copy_1.5_frames"]), flush=True)


def end_to_end(a, nm, clip, depth, H, W, res):
    fmt = fldr_video.Format("nv12", MAT, RNG, depth)
    structs = [fldr_video.frame_struct(f) for f in clip]
    LI, LR = fldr_interlace.lib(), fldr_rate.lib()
    n = ctypes.c_int(0)
    entry = {}
    for name, in_rate, out_rate, model in (("24_to_30i", 24, 30, nm), ("50_to_25i", 50, 25, None)):
        il = fldr_interlace.Interlacer(model, H, W, fmt, in_rate, out_rate, True, fldr_interlace.LINEAR)
        conv = fldr_rate.Converter(nm, H, W, fmt, in_rate, 2 * out_rate, scene=True)
        if model is not None:                                           # the contract, once, before any timing
            got = [o for f in clip for o in il.push(f)]
            fields = [o for f in clip for o in conv.push(f)]
            want = [IO.weave(fields[2 * k], fields[2 * k + 1], "nv12", depth, IO.LINEAR) for k in range(len(got))]
            if not got or not all(np.array_equal(x, y) for fa, fb in zip(got, want) for x, y in zip(fa, fb)):
                raise SystemExit("the stream's frames differ from the woven outputs of the converter")
        il_outs, conv_outs = il._out_structs(), conv._out_structs()

        def run_interlace():
            LI.fldr_interlace_reset(il._h)
            total = 0
            t0 = time.perf_counter()
            for fr in structs:
                rc = LI.fldr_interlace_push(il._h, ctypes.byref(fr), il_outs, ctypes.byref(n), None)
                if rc:
                    raise SystemExit("fldr_interlace_push: %d" % rc)
                total += n.value
            return time.perf_counter() - t0, total

        def run_rate():
            LR.fldr_rate_reset(conv._h)
            total = 0
            t0 = time.perf_counter()
            for fr in structs:
                rc = LR.fldr_rate_push(conv._h, ctypes.byref(fr), conv_outs, ctypes.byref(n), None)
                if rc:
                    raise SystemExit("fldr_rate_push: %d" % rc)
                total += n.value
            return time.perf_counter() - t0, total
        runs = {"interlace": [], "rate": []}
        for alt in range(a.alternations + 1):                            # pass 0 warms both objects
            for who, run in (("interlace", run_interlace), ("rate", run_rate)):
                dt, n_out = run()
                if alt:
                    runs[who].append({"ms_per_pushed_frame": dt * 1e3 / len(structs), "outputs": n_out})
        il.close()
        conv.close()
        med = {k: statistics.median(r["ms_per_pushed_frame"] for r in v) for k, v in runs.items()}
        entry[name] = {"pushed_frames": len(structs), "rate_conversion": "%d -> %d" % (in_rate, 2 * out_rate), "ms_per_pushed_frame": med,
                       "interlace_over_rate": med["interlace"] / med["rate"], "runs": runs}
        print("%dx%d %s %s: interlace %.2f ms per pushed frame, fldr_rate %d -> %d %.2f" % (
            W, H, fmt_name(depth), name, med["interlace"], in_rate, 2 * out_rate, med["rate"]), flush=True)
    res["end_to_end"]["%dx%d_%s" % (W, H, fmt_name(depth))] = entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=6, help="frames of the clip pushed in one timed run")
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--calls", type=int, default=100, help="calls captured into one graph")
    ap.add_argument("--replays", type=int, default=10, help="replays of the graph per timed loop")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    nm = fldr_model.NativeModel.from_npz(Hn.DEFAULT_WEIGHTS, device=0)
    res = {"device": torch.cuda.get_device_name(0), "alternations": a.alternations, "calls_per_graph": a.calls, "replays_per_loop": a.replays,
           "filter_of_the_streams": "linear", "kernels_alone": {}, "end_to_end": {}}
    for H, W, depth in CASES:
        clip = make_clip(a.frames, depth, H, W)
        kernels_alone(a, dev, clip, depth, H, W, res)
        end_to_end(a, nm, clip, depth, H, W, res)
        if a.out:                                                        # written after every size: a cut-off run keeps what it measured
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: v for k, v in res.items() if k not in ("kernels_alone", "end_to_end")}))
    nm.close()


if __name__ == "__main__":
    main()
