#!/usr/bin/env python3
"""The scale API (libfldr_scale.so) on a moving texture (fldr_harness.synthetic_pair, as tools/bench_pulldown.py's clip), NV12 and P010
(BT.709 limited), in one process:

  * µs per fldr_scale_frame of a whole frame at 1920x1080 -> 3840x2160, 3840x2160 -> 1920x1080 and 3840x2160 -> 1280x720 under each of
    the three filters and both reads of the horizontal pass (direct from global memory, staged through LDS), beside a device-to-device copy of the bytes the kernel moves at least once (the input read plus the output
    written) in the same run.  --calls calls are captured back to back into one graph on one stream, the graph is replayed --replays
    times between two device events, so that the host's cost of a call stays out; the candidates are alternated --alternations times;
  * ms per PUSHED frame of a 24 -> 60 scale stream with the placement AUTO picks — 1080p -> 2160p scaled AFTER the forward, 2160p ->
    1080p scaled BEFORE it — beside what a user does without this library: fldr_rate_push 24 -> 60 at 2160 on frames a host scaler made
    (up) or whose outputs a host scaler would still have to shrink (down); the host scaler's own time is not counted, so the comparison
    favours the converter.  The forced opposite placement is timed too.  The C entry points are called directly (host frames in and
    out: includes PCIe and host copies).

    python tools/bench_scale.py [--frames 5] [--alternations 3] [--calls 20] [--replays 5] [--out profiles/scale.json]

Before any timing every scale is compared with its oracle (tests/scale_oracle.py on the library's tables), byte for byte."""
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
import fldr_model  # noqa: E402
import fldr_rate  # noqa: E402
import fldr_scale  # noqa: E402
import fldr_video  # noqa: E402
import scale_oracle as SO  # noqa: E402
from bench_pulldown import MAT, RNG, fmt_name, make_clip, timed, to_dev, to_host  # noqa: E402

SCALES = [((1080, 1920), (2160, 3840)), ((2160, 3840), (1080, 1920)), ((2160, 3840), (720, 1280))]
FILTERS = {"bilinear": fldr_scale.BILINEAR, "bicubic": fldr_scale.BICUBIC, "lanczos": fldr_scale.LANCZOS3}
READS = {"direct": fldr_scale.READ_DIRECT, "staged": fldr_scale.READ_STAGED}          # how the horizontal pass reads its source


def frame_bytes(size, depth):
    return size[0] * size[1] * (1 if depth == 8 else 2) * 3 // 2


def kernels_alone(a, dev, depth, res):
    fmt = fldr_video.Format("nv12", MAT, RNG, depth)
    clips = {}
    for in_size, out_size in SCALES:
        if in_size not in clips:
            clips[in_size] = make_clip(1, depth, in_size[0], in_size[1])[0]
        host = clips[in_size]
        src = to_dev(host, dev)
        out = fldr_video.empty_frame(fmt, out_size[0], out_size[1], dev)
        maps = {(name, rname): fldr_scale.Map(in_size, out_size, fmt, filt, read=read) for name, filt in FILTERS.items() for rname, read in READS.items()}
        picked = fldr_scale.Map(in_size, out_size, fmt, fldr_scale.LANCZOS3)
        auto = [r for r, v in READS.items() if v == picked.read][0]
        picked.close()
        for (name, rname), m in maps.items():
            m.frame(src, out)
            torch.cuda.synchronize()
            want = SO.scale(host, "nv12", depth, out_size, fldr_scale.tables(in_size, out_size, FILTERS[name]))
            if not all(np.array_equal(x, y) for x, y in zip(to_host(out), want)):
                raise SystemExit("the %s %s scale %r -> %r differs from the oracle's" % (name, rname, in_size, out_size))
        moved = frame_bytes(in_size, depth) + frame_bytes(out_size, depth)
        a_buf = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        b_buf = torch.empty_like(a_buf)
        calls = {"scale_%s_%s" % k: (lambda m=m: m.frame(src, out)) for k, m in maps.items()}
        calls["copy_same_bytes"] = lambda: b_buf.copy_(a_buf)
        runs = timed(calls, a, a.calls)
        med = {k: statistics.median(v) for k, v in runs.items()}
        luma_macs = {name: in_size[0] * out_size[1] * maps[(name, "direct")].taps[0] + out_size[0] * out_size[1] * maps[(name, "direct")].taps[1]
                     for name in FILTERS}
        entry = {"us_per_call": med, "runs": runs, "bytes_moved": moved, "auto_reads": auto, "taps": {name: maps[(name, "direct")].taps for name in FILTERS},
                 "tile_rows_by_samples": {"%s_%s" % k: m.tile for k, m in maps.items()}, "lds_bytes": {"%s_%s" % k: m.lds_bytes for k, m in maps.items()},
                 "luma_macs_without_tile_overlap": luma_macs,
                 "over_copy": {"%s_%s" % k: med["scale_%s_%s" % k] / med["copy_same_bytes"] for k in maps},
                 "staged_over_direct": {name: med["scale_%s_staged" % name] / med["scale_%s_direct" % name] for name in FILTERS}}
        key = "%dx%d_to_%dx%d_%s" % (in_size[1], in_size[0], out_size[1], out_size[0], fmt_name(depth))
        res["kernels_alone"][key] = entry
        print("%s (direct / staged; auto reads %s): %s; copy of the same bytes %.1f us" % (
            key, auto, ", ".join("%s %.1f / %.1f us" % (n, med["scale_%s_direct" % n], med["scale_%s_staged" % n]) for n in FILTERS), med["copy_same_bytes"]),
            flush=True)
        for m in maps.values():
            m.close()


def end_to_end(a, nm, depth, res):
    fmt = fldr_video.Format("nv12", MAT, RNG, depth)
    small, big = (1080, 1920), (2160, 3840)
    clip = {small: make_clip(a.frames, depth, small[0], small[1]), big: make_clip(a.frames, depth, big[0], big[1])}
    LS, LR = fldr_scale.lib(), fldr_rate.lib()
    n = ctypes.c_int(0)
    entry = {}

    def run(push, reset, h, structs, outs):
        reset(h)
        total = 0
        t0 = time.perf_counter()
        for fr in structs:
            rc = push(h, ctypes.byref(fr), outs, ctypes.byref(n), None)
            if rc:
                raise SystemExit("push: %d" % rc)
            total += n.value
        return time.perf_counter() - t0, total
    conv = fldr_rate.Converter(nm, big[0], big[1], fmt, 24, 60, scene=True)
    for name, in_size, out_size in (("1080p24_to_2160p60", small, big), ("2160p24_to_1080p60", big, small)):
        objs = {w: fldr_scale.Scaler(nm, in_size, out_size, fmt, 24, 60, fldr_scale.LANCZOS3, w, True) for w in (fldr_scale.AUTO, fldr_scale.BEFORE, fldr_scale.AFTER)}
        auto = objs.pop(fldr_scale.AUTO)
        picked = auto.where
        auto.close()
        structs = [fldr_video.frame_struct(f) for f in clip[in_size]]
        big_structs = [fldr_video.frame_struct(f) for f in clip[big]]      # what the converter at 2160 is pushed
        cands = {("scale_before" if w == fldr_scale.BEFORE else "scale_after"): (LS.fldr_scale_push, LS.fldr_scale_reset, o._h, structs, o._out_structs())
                 for w, o in objs.items()}
        cands["rate_at_2160"] = (LR.fldr_rate_push, LR.fldr_rate_reset, conv._h, big_structs, conv._out_structs())
        runs = {k: [] for k in cands}
        for alt in range(a.alternations + 1):                               # pass 0 warms every object
            for who, args in cands.items():
                dt, n_out = run(*args)
                if alt:
                    runs[who].append({"ms_per_pushed_frame": dt * 1e3 / len(structs), "outputs": n_out})
        for o in objs.values():
            o.close()
        med = {k: statistics.median(r["ms_per_pushed_frame"] for r in v) for k, v in runs.items()}
        auto_name = "scale_before" if picked == fldr_scale.BEFORE else "scale_after"
        entry[name] = {"pushed_frames": len(structs), "auto_picks": auto_name, "ms_per_pushed_frame": med,
                       "auto_over_rate_at_2160": med[auto_name] / med["rate_at_2160"],
                       "auto_over_the_other_placement": med[auto_name] / med["scale_after" if auto_name == "scale_before" else "scale_before"], "runs": runs}
        print("%s %s: auto = %s %.2f ms per pushed frame, the other placement %.2f, fldr_rate at 2160 %.2f" % (
            name, fmt_name(depth), auto_name, med[auto_name], med["scale_after" if auto_name == "scale_before" else "scale_before"], med["rate_at_2160"]),
            flush=True)
    conv.close()
    res["end_to_end"][fmt_name(depth)] = entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=5, help="frames of the clip pushed in one timed run")
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20, help="calls captured into one graph")
    ap.add_argument("--replays", type=int, default=5, help="replays of the graph per timed loop")
    ap.add_argument("--depths", default="8,10", help="8: NV12, 10: P010")
    ap.add_argument("--skip-streams", action="store_true", help="kernels only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "alternations": a.alternations, "calls_per_graph": a.calls, "replays_per_loop": a.replays,
           "filter_of_the_streams": "lanczos", "kernels_alone": {}, "end_to_end": {}}

    def save():
        if a.out:                                                            # written after every part: a cut-off run keeps what it measured
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
    for depth in [int(v) for v in a.depths.split(",")]:
        kernels_alone(a, dev, depth, res)
        save()
    if not a.skip_streams:
        nm = fldr_model.NativeModel.from_npz(Hn.DEFAULT_WEIGHTS, device=0)
        for depth in [int(v) for v in a.depths.split(",")]:
            end_to_end(a, nm, depth, res)
            save()
        nm.close()
    print(json.dumps({k: v for k, v in res.items() if k not in ("kernels_alone", "end_to_end")}))


if __name__ == "__main__":
    main()
