#!/usr/bin/env python3
"""The pulldown API (libfldr_pulldown.so) at 1920x1080 and 3840x2160, NV12 and P010 (BT.709 limited), on a moving texture
(fldr_harness.synthetic_pair, as tools/bench_cadence.py's clip) telecined 3:2 top field first, in one process:

  * µs per fldr_pulldown_measure (cur, prev and next all given: 2.5 luma planes) beside µs per fldr_repeat_measure of two of the same
    frames (2 luma planes), each measure's three launches back to back on one stream — --measures calls captured into one graph, the graph
    replayed --replays times between two device events, so that the host's cost of a call stays out —, the two alternated
    --alternations times; with the bytes each moves, GB/s and the ratio of the two times;
  * µs per fldr_pulldown_assemble (match read on the device; one frame read, one written) beside a device copy of the same frame
    (torch's copy of every plane), alternated the same way;
  * ms per CONTAINER frame of a pulldown stream at 3840x2160, 3:2 film in 60i (30 frames per second, cycle 5, drop 1) -> 60p, beside
    fldr_rate 24 -> 60 pushed the film frames alone — the floor: the difference is the upload, measure, assembly and download of every
    container frame —, alternated --alternations times, the C entry points called directly (host frames in and out: includes PCIe and
    host copies).  Both times are divided by the number of container frames.

    python tools/bench_pulldown.py [--film 8] [--cycles 2] [--alternations 3] [--measures 100] [--replays 10] [--out profiles/pulldown.json]

Before any timing every measure and assembly is compared with its oracle (tests/pulldown_oracle.py, tests/cadence_oracle.py) and the
stream's frames with the converter's on the matched survivors, byte for byte."""
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

import cadence_oracle as C  # noqa: E402
import fldr_cadence  # noqa: E402
import fldr_harness as Hn  # noqa: E402
import fldr_model  # noqa: E402
import fldr_pulldown  # noqa: E402
import fldr_rate  # noqa: E402
import fldr_video  # noqa: E402
import pulldown_frames as PF  # noqa: E402
import pulldown_oracle as P  # noqa: E402
import yuv_hd_oracle as HD  # noqa: E402
import yuv_oracle as O  # noqa: E402

MAT, RNG = "bt709", "limited"
SIZES = [(1080, 1920), (2160, 3840)]
CYCLE, DROP = 5, 1


def fmt_name(depth):
    return "nv12" if depth == 8 else "p010"


def make_clip(n, depth, H, W):
    u8 = Hn.synthetic_pair(H + 4 * n, W + 6 * n, seed=7).numpy()[0]
    out = []
    for k in range(n):
        f = np.ascontiguousarray(u8[:, 4 * k:4 * k + H, 6 * k:6 * k + W])
        if depth == 8:
            out.append(O.pack_nv12(*O.bgr_to_yuv420(f, MAT, RNG)))
        else:
            w16 = (f.astype(np.uint16) << 2) | (f >> 6)
            out.append(HD.pack_planes(*HD.bgr_to_yuv420(w16, MAT, RNG, 10), "nv12", 10))
    return out


def to_dev(planes, dev):
    return tuple(torch.from_numpy(np.ascontiguousarray(p).view(np.int16) if p.dtype == np.uint16 else np.ascontiguousarray(p)).to(dev).view(
        torch.uint16 if p.dtype == np.uint16 else torch.uint8) for p in planes)


def to_host(planes):
    return tuple((p.view(torch.int16).cpu().numpy().view(np.uint16) if p.dtype == torch.uint16 else p.cpu().numpy()) for p in planes)


def timed(calls, a, count):
    """µs per call of each of `calls`, alternated: {name: [one figure per alternation]}.  `count` calls are captured back to back into
    one graph on one stream (a chain, no parallel branches) and the graph is replayed: the host's cost of a call — several times the
    device's at these sizes — stays out of the figure."""
    side = torch.cuda.Stream()
    graphs = {}
    for name, call in calls.items():
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                call()
        side.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name], stream=side):
            for _ in range(count):
                call()
    runs = {k: [] for k in calls}
    for _ in range(a.alternations):
        for name, g in graphs.items():
            g.replay()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.replays):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            runs[name].append(e0.elapsed_time(e1) * 1e3 / (count * a.replays))
    return runs


def kernels_alone(a, dev, frames, depth, H, W, res):
    """frames: three consecutive container frames (host), the middle one matched through P."""
    fmt = fldr_video.Format("nv12", MAT, RNG, depth)
    b = 1 if depth == 8 else 2
    prev, cur, nxt = frames
    d = [to_dev(f, dev) for f in (cur, prev, nxt)]
    out = tuple(torch.empty_like(p) for p in d[0])
    st, rs = fldr_pulldown.measure_state(dev), fldr_cadence.repeat_state(dev)
    got = fldr_pulldown.measure(d[0], d[1], d[2], fmt, 0, state=st)
    want = P.measure(cur, prev, nxt, ("nv12", depth), 0)
    if got != dict(want, reserved=[0] * 5):
        raise SystemExit("the pulldown measure differs from the oracle's: %r" % (got,))
    if fldr_cadence.repeat_measure((d[1], d[0]), fmt, state=rs) != dict(C.measure(prev, cur, ("nv12", depth)), reserved=[0, 0]):
        raise SystemExit("the repeat measure differs from the oracle's")
    fldr_pulldown.assemble(d[0], d[1], d[2], out, fmt, 0, -1, 0, st, fldr_pulldown.POST_KEEP)
    torch.cuda.synchronize()
    frame = P.assemble(cur, prev, nxt, ("nv12", depth), 0, want["match"], want["combed"], P.KEEP)
    if not all(np.array_equal(x, y) for x, y in zip(to_host(out), frame)):
        raise SystemExit("the assembled frame differs from the oracle's")
    luma = H * W * b
    frame_bytes = luma * 3 // 2
    m = timed({"pulldown_measure": lambda: fldr_pulldown.measure(d[0], d[1], d[2], fmt, 0, state=st, read=False),
               "repeat_measure": lambda: fldr_cadence.repeat_measure((d[1], d[0]), fmt, state=rs, read=False)}, a, a.measures)

    def copy():
        for o, p in zip(out, d[0]):
            o.copy_(p)
    c = timed({"pulldown_assemble": lambda: fldr_pulldown.assemble(d[0], d[1], d[2], out, fmt, 0, -1, 0, st, fldr_pulldown.POST_KEEP),
               "device_copy": copy}, a, a.measures)
    med = {k: statistics.median(v) for k, v in list(m.items()) + list(c.items())}
    moved = {"pulldown_measure": luma * 5 // 2, "repeat_measure": 2 * luma, "pulldown_assemble": 2 * frame_bytes, "device_copy": 2 * frame_bytes}
    entry = {"us_per_call": med, "runs": dict(m, **c), "bytes_moved": moved,
             "gb_per_s": {k: moved[k] / med[k] * 1e-3 for k in med},
             "measure_over_repeat_measure": med["pulldown_measure"] / med["repeat_measure"],
             "assemble_over_device_copy": med["pulldown_assemble"] / med["device_copy"], "result": got}
    res["kernels_alone"]["%dx%d_%s" % (W, H, fmt_name(depth))] = entry
    print("%dx%d %s: measure %.1f us (repeat measure %.1f), assemble %.1f us (device copy %.1f)" % (
        W, H, fmt_name(depth), med["pulldown_measure"], med["repeat_measure"], med["pulldown_assemble"], med["device_copy"]), flush=True)


def end_to_end(a, nm, film, depth, H, W, res):
    fmt = fldr_video.Format("nv12", MAT, RNG, depth)
    frames, _ = PF.telecine32(film, 0)
    frames = frames[:len(frames) // CYCLE * CYCLE]
    results, matched = P.match_stream(frames, ("nv12", depth), 0)
    kept, _ = P.survivors(results, CYCLE, DROP)
    n_film = len(frames) // CYCLE * (CYCLE - DROP)
    if len(kept) != n_film or not all(np.array_equal(x, y) for k, f in zip(kept, film) for x, y in zip(matched[k], f)):
        raise SystemExit("the oracle's survivors are not the film frames: kept %r" % (kept,))
    pd = fldr_pulldown.Pulldown(nm, H, W, fmt, 30, 60, CYCLE, DROP, 0)
    conv = fldr_rate.Converter(nm, H, W, fmt, 24, 60, scene=True)
    got = [o for f in frames for o in pd.push(f)] + pd.flush()
    want = [o for f in film[:n_film] for o in conv.push(f)] + conv.flush()
    if len(got) != len(want) or not all(np.array_equal(x, y) for fa, fb in zip(got, want) for x, y in zip(fa, fb)):
        raise SystemExit("the stream's frames differ from the converter's on the film frames")
    structs = [fldr_video.frame_struct(f) for f in frames]
    film_structs = [fldr_video.frame_struct(f) for f in film[:n_film]]
    pd_outs, conv_outs = pd._out_structs(), conv._out_structs()
    LP, LR = fldr_pulldown.lib(), fldr_rate.lib()
    n = ctypes.c_int(0)

    def run_pulldown():
        LP.fldr_pulldown_reset(pd._h)
        total = 0
        t0 = time.perf_counter()
        for _ in range(a.cycles):
            for fr in structs:
                rc = LP.fldr_pulldown_push(pd._h, ctypes.byref(fr), pd_outs, ctypes.byref(n), None)
                if rc:
                    raise SystemExit("fldr_pulldown_push: %d" % rc)
                total += n.value
        rc = LP.fldr_pulldown_flush(pd._h, pd_outs, ctypes.byref(n), None)     # the last cycle is completed by the flush
        if rc:
            raise SystemExit("fldr_pulldown_flush: %d" % rc)
        return time.perf_counter() - t0, total + n.value

    def run_floor():
        LR.fldr_rate_reset(conv._h)
        total = 0
        t0 = time.perf_counter()
        for _ in range(a.cycles):
            for fr in film_structs:
                rc = LR.fldr_rate_push(conv._h, ctypes.byref(fr), conv_outs, ctypes.byref(n), None)
                if rc:
                    raise SystemExit("fldr_rate_push: %d" % rc)
                total += n.value
        rc = LR.fldr_rate_flush(conv._h, conv_outs, ctypes.byref(n))
        if rc:
            raise SystemExit("fldr_rate_flush: %d" % rc)
        return time.perf_counter() - t0, total + n.value
    container = len(structs) * a.cycles
    runs = {"pulldown": [], "rate_on_film": []}
    for alt in range(a.alternations + 1):                                # pass 0 warms both objects
        for name, run in (("pulldown", run_pulldown), ("rate_on_film", run_floor)):
            dt, n_out = run()
            if alt:
                runs[name].append({"ms_per_container_frame": dt * 1e3 / container, "output_frames_per_s": n_out / dt, "outputs": n_out})
    pd.close()
    conv.close()
    med = {k: statistics.median(r["ms_per_container_frame"] for r in v) for k, v in runs.items()}
    res["end_to_end"]["%dx%d_%s" % (W, H, fmt_name(depth))] = {
        "container_frames": container, "film_frames": n_film * a.cycles, "ms_per_container_frame": med,
        "cost_ms_per_container_frame": med["pulldown"] - med["rate_on_film"], "pulldown_over_floor": med["pulldown"] / med["rate_on_film"], "runs": runs}
    print("%dx%d %s 60i (5, 1) -> 60p: pulldown %.2f ms per container frame, fldr_rate 24 -> 60 on the film frames %.2f" % (
        W, H, fmt_name(depth), med["pulldown"], med["rate_on_film"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--film", type=int, default=8, help="film frames of the clip (3:2: five container frames per four)")
    ap.add_argument("--cycles", type=int, default=2, help="times the container clip is pushed in one timed run")
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--measures", type=int, default=100, help="calls captured into one graph")
    ap.add_argument("--replays", type=int, default=10, help="replays of the graph per timed loop")
    ap.add_argument("--depths", default="8,10", help="8: NV12, 10: P010")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    nm = fldr_model.NativeModel.from_npz(Hn.DEFAULT_WEIGHTS, device=0)
    res = {"device": torch.cuda.get_device_name(0), "cycle": CYCLE, "drop": DROP, "alternations": a.alternations, "calls_per_graph": a.measures, "replays_per_loop": a.replays,
           "kernels_alone": {}, "end_to_end": {}}
    for H, W in SIZES:
        for depth in [int(v) for v in a.depths.split(",")]:
            film = make_clip(a.film, depth, H, W)
            frames, _ = PF.telecine32(film, 0)
            kernels_alone(a, dev, frames[1:4], depth, H, W, res)         # frame 2 (B top, C bottom): matched through the previous frame
            if (H, W) == SIZES[-1]:
                end_to_end(a, nm, film, depth, H, W, res)
            if a.out:                                                    # written after every format: a cut-off run keeps what it measured
                with open(a.out, "w") as f:
                    f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: v for k, v in res.items() if k not in ("kernels_alone", "end_to_end")}))
    nm.close()


if __name__ == "__main__":
    main()
