#!/usr/bin/env python3
"""The pipe API (libfldr_pipe.so) beside the synchronous converter it is built on (fldr_rate_push), host frames in and host frames out,
in one process: at 1920x1080 and 3840x2160, NV12 and P010 (BT.709 limited), for 24 -> 60, 1 -> 2 and 1 -> 8, on a moving texture
(fldr_harness.synthetic_pair, as tools/bench_rate.py's sessions).

  * ms per pushed frame and output frames/s of fldr_rate_push and of the pipe at depth 1 .. 4, with the copying calls
    (fldr_pipe_submit(frame) / fldr_pipe_receive: the host copies the converter makes) and with the in-place calls
    (fldr_pipe_submit(NULL) / fldr_pipe_receive_view: no host copy).  The converter and the pipe modes alternate --alternations times;
    the median is reported, every run is kept.  The C entry points are called directly (no fresh numpy copies of the outputs, which
    fldr_rate.Converter.push and fldr_pipe.Pipe.receive add).  The pipe is driven the way examples/fldr_fps_async.c drives it: receive
    the oldest job when `depth` are outstanding, then submit.  The in-place mode times no producer and no consumer: the pinned input
    frames hold clip frames written before the clock starts, and the views are not read.
  * a breakdown per configuration, each stage alone, in a separate timed pass: the host copy of one frame into and out of pinned memory
    by the host clock; the upload of one frame, the download of one frame and the forward of one pair (fldr_rate_forward with the n_t
    the schedule gives) by device events.  From them the floor per pushed frame — the largest of the compute time, the upload plus
    download time of the bytes a push moves, and the host copy time of the mode — and how close each mode comes to it.
  * before any timing the pipe's jobs are compared with the converter's on the same clip, byte for byte.

    python tools/bench_pipe.py [--frames 12] [--cycles 3] [--alternations 3] [--sizes 1080,2160] [--out profiles/pipe_push.json]

A timed run pushes the clip of --frames frames --cycles times over (the jump from the last frame back to the first is one more pair,
a cut or not: the forward runs either way), so that a run lasts a good fraction of a second.
"""
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
import fldr_pipe  # noqa: E402
import fldr_rate  # noqa: E402
import fldr_video  # noqa: E402
import yuv_hd_oracle as HD  # noqa: E402
import yuv_oracle as O  # noqa: E402

MAT, RNG = "bt709", "limited"
SPREAD = 0.10                     # run-to-run spread of the push figures
RATIOS = [(24, 60), (1, 2), (1, 8)]
DEPTHS = [1, 2, 3, 4]


def make_clip(h, w, n, depth):
    u8 = Hn.synthetic_pair(h + 4 * n, w + 6 * n, seed=7).numpy()[0]
    out = []
    for k in range(n):
        f = np.ascontiguousarray(u8[:, 4 * k:4 * k + h, 6 * k:6 * k + w])
        if depth == 8:
            out.append(O.pack_nv12(*O.bgr_to_yuv420(f, MAT, RNG)))
        else:
            w16 = (f.astype(np.uint16) << 2) | (f >> 6)
            out.append(HD.pack_planes(*HD.bgr_to_yuv420(w16, MAT, RNG, 10), "nv12", 10))
    return out


# ---- the drivers: raw library calls ---------------------------------------------------------------------------------------------------
def run_converter(c, structs, outs_struct):
    """Push every frame -> (seconds, output frames)."""
    L = fldr_rate.lib()
    n, total = ctypes.c_int(0), 0
    res = fldr_rate.SceneResult()
    t0 = time.perf_counter()
    for fr in structs:
        rc = L.fldr_rate_push(c._h, ctypes.byref(fr), outs_struct, ctypes.byref(n), ctypes.byref(res))
        if rc:
            raise SystemExit("fldr_rate_push: %d" % rc)
        total += n.value
    return time.perf_counter() - t0, total


def run_pipe(p, structs, views):
    """views False: submit(frame) / receive into the staged host frames; True: submit(NULL) / receive_view.  -> (seconds, outputs)."""
    L = fldr_pipe.lib()
    n, total = ctypes.c_int(0), 0
    res = fldr_rate.SceneResult()
    h, depth = p._h, p.depth

    def receive():
        if views:
            rc = L.fldr_pipe_receive_view(h, p._views, ctypes.byref(n), ctypes.byref(res))
        else:
            rc = L.fldr_pipe_receive(h, p._out_structs, ctypes.byref(n), ctypes.byref(res))
        if rc:
            raise SystemExit("fldr_pipe_receive: %d" % rc)
        return n.value
    t0 = time.perf_counter()
    for fr in structs:
        if L.fldr_pipe_pending(h) == depth:
            total += receive()
        rc = L.fldr_pipe_submit(h, None if views else ctypes.byref(fr))
        if rc:
            raise SystemExit("fldr_pipe_submit: %d" % rc)
    while L.fldr_pipe_pending(h):
        total += receive()
    return time.perf_counter() - t0, total


def check_equal(nm, h, w, fmt, clip, in_rate, out_rate):
    """The pipe's jobs (depth 3, in-place input, views) against Converter.push, frame by frame."""
    c = fldr_rate.Converter(nm, h, w, fmt, in_rate, out_rate, scene=True)
    p = fldr_pipe.Pipe(nm, h, w, fmt, in_rate, out_rate, depth=3, scene=True)
    want = [(c.push(f), c.last_scene) for f in clip[:6]]
    got = []
    for f in clip[:6]:
        if p.pending == 3:
            got.append(p.receive())
        for dst, src in zip(p.input_planes(), f):
            dst[...] = src
        p.submit()
    while p.pending:
        got.append(p.receive())
    c.close()
    p.close()
    for k, ((a, sa), (b, sb)) in enumerate(zip(got, want)):
        if sa != sb or len(a) != len(b) or not all(np.array_equal(x, y) for fa, fb in zip(a, b) for x, y in zip(fa, fb)):
            raise SystemExit("%dx%d %d -> %d: job %d of the pipe differs from the converter's push" % (w, h, in_rate, out_rate, k))


# ---- the stages alone -------------------------------------------------------------------------------------------------------------------
def breakdown(nm, nr, dev, h, w, fmt, clip, in_rate, out_rate, reps):
    sched = fldr_rate.schedule(1000, in_rate, out_rate)[1:1000]
    outs_per_push = sum(len(s) for s in sched) / len(sched)
    inter_per_push = sum(1 for s in sched for o in s if o[2]) / len(sched)
    n_t = max(sum(1 for o in s if o[2]) for s in sched)
    frame_bytes = sum(p.nbytes for p in clip[0])
    # host copies: one frame into the pipe's pinned input frame, one frame out of it (numpy, whole planes)
    p = fldr_pipe.Pipe(nm, h, w, fmt, in_rate, out_rate, depth=1, scene=True)
    pinned = p.input_planes()
    mine = tuple(np.empty_like(a) for a in clip[0])
    t_in, t_out = [], []
    for k in range(reps):
        src = clip[k % len(clip)]
        t0 = time.perf_counter()
        for d, s in zip(pinned, src):
            np.copyto(d, s)
        t1 = time.perf_counter()
        for d, s in zip(mine, pinned):
            np.copyto(d, s)
        t2 = time.perf_counter()
        t_in.append((t1 - t0) * 1e3)
        t_out.append((t2 - t1) * 1e3)
    p.close()
    # copies by device events: one frame up, one frame down, pinned memory
    host = torch.empty(frame_bytes, dtype=torch.uint8).pin_memory()
    devb = torch.empty(frame_bytes, dtype=torch.uint8, device=dev)

    def by_events(fn, n):
        for _ in range(2):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n
    up = by_events(lambda: devb.copy_(host, non_blocking=True), reps)
    down = by_events(lambda: host.copy_(devb, non_blocking=True), reps)
    # the forward of one pair with the schedule's n_t, frames resident
    pair = [tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in f) for f in clip[:2]]
    t = torch.tensor([(k + 1) / (n_t + 1) for k in range(n_t)], device=dev, dtype=torch.float32)
    ws = nr.workspace(h, w, n_t)
    outs = [fldr_video.empty_frame(fmt, h, w, dev) for _ in range(n_t)]
    comp = by_events(lambda: nr.forward(pair, t, fmt, outs=outs, ws=ws, read=False), reps)
    del ws, outs, pair
    pack, unpack = statistics.median(t_in), statistics.median(t_out) * outs_per_push
    copies = up + down * inter_per_push
    return {"frame_bytes": frame_bytes, "outputs_per_push": outs_per_push, "interpolated_per_push": inter_per_push, "n_t": n_t,
            "host_pack_ms": pack, "host_unpack_ms": unpack, "upload_ms": up, "download_ms": down * inter_per_push,
            "upload_GBps": frame_bytes / up / 1e6, "download_GBps": frame_bytes / down / 1e6, "compute_ms": comp,
            "floor_ms": {"copy": max(comp, copies, pack + unpack), "inplace": max(comp, copies)},
            "floor_stage": {"copy": max((comp, "compute"), (copies, "pcie"), (pack + unpack, "host copies"))[1],
                            "inplace": max((comp, "compute"), (copies, "pcie"))[1]}}


def one_config(a, nm, nr, dev, h, w, depth_bits, clip, in_rate, out_rate):
    fmt = fldr_video.Format("nv12", MAT, RNG, depth_bits)
    check_equal(nm, h, w, fmt, clip, in_rate, out_rate)
    structs = [fldr_video.frame_struct(f) for f in clip] * a.cycles
    c = fldr_rate.Converter(nm, h, w, fmt, in_rate, out_rate, scene=True)
    outs_struct = c._out_structs()
    pipes = {d: fldr_pipe.Pipe(nm, h, w, fmt, in_rate, out_rate, depth=d, scene=True) for d in DEPTHS}
    runs = {"converter": []}
    for d in DEPTHS:
        runs["pipe_copy_d%d" % d] = []
        runs["pipe_inplace_d%d" % d] = []
    outputs = None

    def record(name, dt, n_out):
        runs[name].append({"ms_per_push": dt * 1e3 / len(structs), "output_frames_per_s": n_out / dt})
    for alt in range(a.alternations + 1):                            # pass 0 warms every object (and fills the pinned input rings)
        fldr_rate.lib().fldr_rate_reset(c._h)
        dt, n_out = run_converter(c, structs, outs_struct)
        outputs = n_out
        if alt:
            record("converter", dt, n_out)
        for d in DEPTHS:
            p = pipes[d]
            for views in (False, True):
                p.reset()
                dt, n_out = run_pipe(p, structs, views)
                if n_out != outputs:
                    raise SystemExit("the pipe returned %d frames, the converter %d" % (n_out, outputs))
                if alt:
                    record("pipe_%s_d%d" % ("inplace" if views else "copy", d), dt, n_out)
    c.close()
    for p in pipes.values():
        p.close()
    med = {k: {f: statistics.median(r[f] for r in v) for f in ("ms_per_push", "output_frames_per_s")} for k, v in runs.items()}
    br = breakdown(nm, nr, dev, h, w, fmt, clip, in_rate, out_rate, a.reps)
    conv = med["converter"]["ms_per_push"]
    verdict = {}
    for mode in ("copy", "inplace"):
        best = min((med["pipe_%s_d%d" % (mode, d)]["ms_per_push"], d) for d in DEPTHS if d >= 2)
        verdict[mode] = {"best_depth": best[1], "ms_per_push": best[0], "converter_over_pipe": conv / best[0],
                         "faster_than_the_spread": bool(conv / best[0] > 1 + SPREAD), "floor_ms": br["floor_ms"][mode],
                         "floor_stage": br["floor_stage"][mode], "pipe_over_floor": best[0] / br["floor_ms"][mode]}
    return {"size": [h, w], "format": "nv12" if depth_bits == 8 else "p010", "in_rate": in_rate, "out_rate": out_rate,
            "pushes": len(structs), "outputs": outputs, "median": med, "runs": runs, "breakdown": br,
            "converter_over_floor": conv / br["floor_ms"]["copy"], "verdict": verdict}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12, help="frames of the clip")
    ap.add_argument("--cycles", type=int, default=3, help="times the clip is pushed in one timed run")
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10, help="repetitions of each stage in the breakdown")
    ap.add_argument("--sizes", default="1080,2160", help="heights: 1080 (1920x1080), 2160 (3840x2160)")
    ap.add_argument("--depths", default="8,10", help="8: NV12, 10: P010")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    nm = fldr_model.NativeModel.from_npz(Hn.DEFAULT_WEIGHTS, device=0)
    nr = fldr_rate.NativeRate(nm)
    res = {"device": torch.cuda.get_device_name(0), "pushes": a.frames * a.cycles, "alternations": a.alternations, "spread": SPREAD, "configs": []}
    for hh in [int(v) for v in a.sizes.split(",")]:
        h, w = hh, {1080: 1920, 2160: 3840}.get(hh, hh * 16 // 9)
        for bits in [int(v) for v in a.depths.split(",")]:
            clip = make_clip(h, w, a.frames, bits)
            for in_rate, out_rate in RATIOS:
                t0 = time.perf_counter()
                r = one_config(a, nm, nr, dev, h, w, bits, clip, in_rate, out_rate)
                res["configs"].append(r)
                v = r["verdict"]
                print("%dx%d %s %d->%d: converter %.2f ms/push; pipe copy d%d %.2f (x%.2f), in-place d%d %.2f (x%.2f); floor %.2f / %.2f ms (%s / %s)  [%.0f s]" % (
                    w, h, r["format"], in_rate, out_rate, r["median"]["converter"]["ms_per_push"], v["copy"]["best_depth"], v["copy"]["ms_per_push"],
                    v["copy"]["converter_over_pipe"], v["inplace"]["best_depth"], v["inplace"]["ms_per_push"], v["inplace"]["converter_over_pipe"],
                    v["copy"]["floor_ms"], v["inplace"]["floor_ms"], v["copy"]["floor_stage"], v["inplace"]["floor_stage"], time.perf_counter() - t0),
                    flush=True)
                if a.out:                                            # written after every configuration: a cut-off run keeps what it measured
                    with open(a.out, "w") as f:
                        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: v for k, v in res.items() if k != "configs"}))
    nm.close()


if __name__ == "__main__":
    main()
