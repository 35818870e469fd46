#!/usr/bin/env python3
"""The field API (libfldr_field.so) on one MI355X, NV12 and P010 (BT.709 limited), on a moving texture (fldr_harness.synthetic_pair),
in one process:

  * µs per fldr_field_weave at 1920x1080 and 3840x2160 — MOTION on moving content, MOTION on still content, INTRA — by device events
    around the replay of a captured graph of --reps calls (a loop of calls would time the host's enqueue rate), with the bytes the
    rule needs (every source byte once plus every output byte: 3 frames in MOTION, 1.5 in INTRA) and, beside each, a device-to-device copy that reads and writes the same total in the same run, the two alternated --alternations times.  Both walk
    --sets buffer sets in turn so that a launch does not find its predecessor's lines in the caches.
  * ms per fldr_field_forward on 1080i and 2160i beside fldr_video_forward on the same field pair (H/2 x W views, n_t = 1), the cut
    measure alone and the weave alone, alternated.
  * output frames per second of a stream at 1080i, rate 2, beside fldr_rate_push 25 -> 50 at the same size (host frames in and out:
    includes PCIe and host copies), alternated.

    python tools/bench_field.py [--alternations 3] [--out profiles/field.json]

Before any timing the weave at 1920x1080 is compared with its oracle (tests/field_oracle.py) byte for byte, and the forward's output
with the oracle's weave of its temporal frame."""
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

import field_oracle as F  # noqa: E402
import fldr_field as K  # noqa: E402
import fldr_harness as Hn  # noqa: E402
import fldr_model  # noqa: E402
import fldr_rate  # noqa: E402
import fldr_video  # noqa: E402
import rate_frames as RF  # noqa: E402

MAT, RNG = "bt709", "limited"
SIZES = {"1080": (1080, 1920), "2160": (2160, 3840)}


def fmt_name(depth):
    return "nv12" if depth == 8 else "p010"


def pictures(H, W, depth, n=2):
    """n pictures of one moving scene in the container (numpy planes)."""
    u8 = Hn.synthetic_pair(H + 4 * n, W + 6 * n, seed=7).numpy()[0]
    return [RF.planes_of_bgr(np.ascontiguousarray(u8[:, 4 * k:4 * k + H, 6 * k:6 * k + W]), "nv12", depth, MAT, RNG) for k in range(n)]


def weave_frames(a, b):
    """The woven frame with the top field of picture a and the bottom field of picture b."""
    out = []
    for p, q in zip(a, b):
        r = p.copy()
        r[1::2] = q[1::2]
        out.append(r)
    return tuple(out)


def to_dev(planes, dev):
    return tuple(torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in planes)


def frame_bytes(H, W, depth):
    return (H * W + 2 * ((W + 1) // 2) * (H // 2)) * (2 if depth == 10 else 1)


def timed(calls, reps, alternations, graph=False):
    """{name: median µs per call}, {name: runs}: each call warmed, then `reps` of it between two device events, the calls alternated.
    graph: the `reps` calls are captured once, on one stream, and the replay is timed — the device's time, not the host's enqueue rate,
    which is what a loop of calls of a few µs each would measure."""
    runs = {k: [] for k in calls}
    graphs = {}
    if graph:
        s = torch.cuda.Stream()
        for name, call in calls.items():
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for i in range(5):
                    call(i)
            s.synchronize()
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name], stream=s):
                for i in range(reps):
                    call(i)
    for _ in range(alternations):
        for name, call in calls.items():
            if graph:
                graphs[name].replay()
            else:
                for i in range(5):
                    call(i)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if graph:
                graphs[name].replay()
            else:
                for i in range(reps):
                    call(i)
            e1.record()
            torch.cuda.synchronize()
            runs[name].append(e0.elapsed_time(e1) * 1e3 / reps)
    return {k: statistics.median(v) for k, v in runs.items()}, runs


def same(got, want):
    return all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))


def weave_alone(a, dev, size, depth, res):
    H, W = SIZES[size]
    fmt = fldr_video.Format("nv12", MAT, RNG, depth)
    pa, pb = pictures(H, W, depth)
    temporal_host = tuple(np.ascontiguousarray(p[1::2]) if k == 0 else np.ascontiguousarray(p[:H // 4]) for k, p in enumerate(pb))
    content = {"motion_moving": (weave_frames(pa, pb), weave_frames(pa, pa), weave_frames(pb, pb), K.MOTION),
               "motion_still": (weave_frames(pa, pa), weave_frames(pa, pa), weave_frames(pa, pa), K.MOTION),
               "intra": (weave_frames(pa, pb), None, None, K.INTRA)}
    fb = frame_bytes(H, W, depth)
    out = {}
    for kind, (cur, prev, nxt, mode) in content.items():
        sets = []
        for _ in range(a.sets):
            d = [None if f is None else to_dev(f, dev) for f in (cur, prev, nxt, temporal_host if mode == K.MOTION else None)]
            sets.append((d, fldr_video.empty_frame(fmt, H, W, dev)))
        if size == "1080":                                                # the oracle's per-sample statement takes seconds at this size
            d, o = sets[0]
            K.weave(d[0], d[1], d[2], d[3], fmt, 0, mode, out=o)
            torch.cuda.synchronize()
            if not same(o, F.weave(cur, prev, nxt, temporal_host, "nv12", depth, 0, mode)):
                raise SystemExit("the %s weave differs from the oracle's" % kind)
        total = fb * 3 if mode == K.MOTION else fb * 3 // 2              # bytes read once + bytes written
        src = [torch.empty(total // 2, dtype=torch.uint8, device=dev).fill_(k) for k in range(a.sets)]
        dst = [torch.empty(total // 2, dtype=torch.uint8, device=dev) for _ in range(a.sets)]

        def run_weave(i):
            d, o = sets[i % a.sets]
            K.weave(d[0], d[1], d[2], d[3], fmt, 0, mode, out=o)

        def run_copy(i):
            dst[i % a.sets].copy_(src[i % a.sets])
        med, runs = timed({"weave": run_weave, "copy": run_copy}, a.reps, a.alternations, graph=True)
        rate = {k: total / (v * 1e-6) / 1e12 for k, v in med.items()}
        out[kind] = {"bytes_read_plus_written": total, "us": med, "tb_per_s": rate, "weave_over_copy_rate": rate["weave"] / rate["copy"], "runs": runs}
        print("%s %s %s: weave %.1f us (%.2f TB/s), copy of the same bytes %.1f us (%.2f TB/s)" % (
            size, fmt_name(depth), kind, med["weave"], rate["weave"], med["copy"], rate["copy"]), flush=True)
        del sets, src, dst
    res["weave"].setdefault(size, {})[fmt_name(depth)] = out


def forward_parts(a, nf, dev, size, depth, res):
    H, W = SIZES[size]
    fmt = fldr_video.Format("nv12", MAT, RNG, depth)
    pa, pb = pictures(H, W, depth)
    cur, prev, nxt = weave_frames(pa, pa), weave_frames(pa, pb), weave_frames(pb, pa)      # parity 0: the fields before / after are pb's and pa's odd rows
    d = [to_dev(f, dev) for f in (cur, prev, nxt)]
    ws = nf.workspace(H, W)
    out = fldr_video.empty_frame(fmt, H, W, dev)
    nf.forward(d[0], d[1], d[2], fmt, 0, scene=True, out=out, ws=ws)
    torch.cuda.synchronize()
    temporal = nf.temporal(ws, H, W, fmt)
    if size == "1080" and not same(out, F.weave(cur, prev, nxt, tuple(p.cpu().numpy() for p in temporal), "nv12", depth, 0, F.MOTION)):
        raise SystemExit("the forward's output differs from the oracle's weave of its temporal frame")
    views = (K.field_view(d[1], 1), K.field_view(d[2], 1))
    nv = fldr_video.NativeVideo(nf.model)
    vws = nv.workspace(H // 2, W, 1)
    vout = [fldr_video.empty_frame(fmt, H // 2, W, dev)]
    t = torch.tensor([0.5], dtype=torch.float32, device=dev)
    st = fldr_rate.scene_state(dev)
    calls = {"field_forward": lambda i: nf.forward(d[0], d[1], d[2], fmt, 0, scene=True, out=out, ws=ws),
             "video_forward": lambda i: nv.forward(views, t, fmt, fmt, outs=vout, ws=vws),
             "scene_measure": lambda i: fldr_rate.scene_measure(views, fmt, state=st, read=False),
             "weave": lambda i: K.weave(d[0], d[1], d[2], temporal, fmt, 0, K.MOTION, out=out)}
    med, runs = timed(calls, a.forwards, a.alternations)
    ms = {k: v / 1e3 for k, v in med.items()}
    res["forward"].setdefault(size, {})[fmt_name(depth)] = {
        "ms": ms, "field_minus_video_ms": ms["field_forward"] - ms["video_forward"], "measure_plus_weave_ms": ms["scene_measure"] + ms["weave"],
        "runs_us": runs}
    print("%si %s: field forward %.3f ms, video forward on the field pair %.3f ms, cut measure %.3f ms, weave %.3f ms" % (
        size, fmt_name(depth), ms["field_forward"], ms["video_forward"], ms["scene_measure"], ms["weave"]), flush=True)


def stream_throughput(a, nm, depth, res):
    H, W = SIZES["1080"]
    fmt = fldr_video.Format("nv12", MAT, RNG, depth)
    pics = pictures(H, W, depth, a.frames + 1)
    frames = [weave_frames(pics[k], pics[k + 1]) for k in range(a.frames)]
    structs = [fldr_video.frame_struct(f) for f in frames]
    stream = K.Stream(nm, H, W, fmt, tff=True, rate=2, scene=True)
    conv = fldr_rate.Converter(nm, H, W, fmt, 25, 50, scene=True)
    s_outs, c_outs = stream._out_structs(), conv._out_structs()
    LF, LR = K.lib(), fldr_rate.lib()
    n = ctypes.c_int(0)

    def run_field():
        LF.fldr_field_reset(stream._h)
        total = 0
        t0 = time.perf_counter()
        for fr in structs:
            rc = LF.fldr_field_push(stream._h, ctypes.byref(fr), s_outs, ctypes.byref(n), None)
            if rc:
                raise SystemExit("fldr_field_push: %d" % rc)
            total += n.value
        return time.perf_counter() - t0, total

    def run_rate():
        LR.fldr_rate_reset(conv._h)
        total = 0
        t0 = time.perf_counter()
        for fr in structs:
            rc = LR.fldr_rate_push(conv._h, ctypes.byref(fr), c_outs, ctypes.byref(n), None)
            if rc:
                raise SystemExit("fldr_rate_push: %d" % rc)
            total += n.value
        return time.perf_counter() - t0, total
    runs = {"field_rate2": [], "rate_25_to_50": []}
    for alt in range(a.alternations + 1):                                # pass 0 warms both objects
        for name, run in (("field_rate2", run_field), ("rate_25_to_50", run_rate)):
            dt, n_out = run()
            if alt:
                runs[name].append({"output_frames_per_s": n_out / dt, "ms_per_pushed_frame": dt * 1e3 / len(structs), "outputs": n_out})
    stream.close()
    conv.close()
    med = {k: statistics.median(r["output_frames_per_s"] for r in v) for k, v in runs.items()}
    res["stream_1080i"][fmt_name(depth)] = {"pushed_frames": len(structs), "output_frames_per_s": med, "runs": runs}
    print("1080i %s: stream rate 2 %.1f output frames/s, fldr_rate 25 -> 50 %.1f output frames/s" % (fmt_name(depth), med["field_rate2"], med["rate_25_to_50"]),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200, help="weaves / copies per timed loop")
    ap.add_argument("--forwards", type=int, default=20, help="forwards per timed loop")
    ap.add_argument("--frames", type=int, default=12, help="frames of the stream clip")
    ap.add_argument("--sets", type=int, default=4, help="buffer sets the weave and the copy walk")
    ap.add_argument("--depths", default="8,10", help="8: NV12, 10: P010")
    ap.add_argument("--sizes", default="1080,2160")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    nm = fldr_model.NativeModel.from_npz(Hn.DEFAULT_WEIGHTS, device=0)
    nf = K.NativeField(nm)
    res = {"device": torch.cuda.get_device_name(0), "alternations": a.alternations, "reps": a.reps, "forwards": a.forwards, "sets": a.sets,
           "weave": {}, "forward": {}, "stream_1080i": {}}

    def save():
        if a.out:                                                        # written after every part: a cut-off run keeps what it measured
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
    for depth in [int(v) for v in a.depths.split(",")]:
        for size in a.sizes.split(","):
            weave_alone(a, dev, size, depth, res)
            save()
            forward_parts(a, nf, dev, size, depth, res)
            save()
        stream_throughput(a, nm, depth, res)
        save()
    print(json.dumps({k: v for k, v in res.items() if k not in ("weave", "forward", "stream_1080i")}))
    nm.close()


if __name__ == "__main__":
    main()
