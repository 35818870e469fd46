#!/usr/bin/env python3
"""The linear-light API (libfldr_light.so) on random NV12 and P010 frames at 3840x2160, beside fldr_shutter_mix on the same frames in
the same run, and its converter beside the shutter converter on a moving texture:

  * µs and bytes per µs of the three kernels light_accumulate_kernel (two frames onto an accumulator), light_resolve_kernel and
    light_mix_kernel (two frames).  The API reaches them only with the video library's converters on either side, so the tool times
    the calls (fldr_light_accumulate / resolve / mix) and the two converters alone (through libfldr_video_test.so), by device events
    over back-to-back launches on one stream, and reports call minus converters as the kernel's time; the --trace table separates
    them exactly.  fldr_shutter_mix of the same two frames is the yardstick.  Bytes: a planar frame is 3 H W samples (P), the
    accumulator 12 H W bytes (A), a 4:2:0 frame 1.5 H W samples (F).
  * Converter.push ms for 120 -> 24 (sub = 1), 180 degrees, at 1920x1080 and 3840x2160, fldr_light beside fldr_shutter.

    python tools/bench_light.py [--steps 50] [--alternations 3] [--out profiles/light_forward.json]

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_light.py --trace [--depth 8|10]
        a short loop of the calls for the kernel trace (no counters in that run): the three light kernels beside the converters and
        shutter_mix_kernel in one table.  The JSON line it prints carries the bytes each kernel moves per launch.

Every result is checked against tests/light_oracle.py before timing."""
import argparse
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
import fldr_light as L  # noqa: E402
import fldr_model  # noqa: E402
import fldr_shutter as T  # noqa: E402
import fldr_video  # noqa: E402
import light_oracle as LO  # noqa: E402
import yuv_oracle as O  # noqa: E402

MAT, RNG = "bt709", "limited"
H4, W4 = 2160, 3840


def fmt_name(depth):
    return "nv12" if depth == 8 else "p010"


def kernel_bytes(depth):
    """Bytes per launch of each kernel on two 4K frames."""
    b = 2 if depth == 10 else 1
    P, A, F = 3 * H4 * W4 * b, 12 * H4 * W4, H4 * W4 * 3 // 2 * b
    return {"light_accumulate_kernel": 2 * P + 2 * A, "light_resolve_kernel": A + P, "light_mix_kernel": 3 * P, "shutter_mix_kernel": 3 * F,
            "yuv420_to_planar_pair": 2 * F + 2 * P, "planar_to_yuv420": P + F}


def calls_of(dev, depth):
    """[(name, callable)] on two random 4K frames, checked against the oracle."""
    fmt = fldr_video.Format("nv12", MAT, RNG, depth)
    curve = L.Curve("gamma24" if depth == 8 else "pq", depth)
    g = np.random.default_rng(depth)
    dt, top = (np.uint8, 256) if depth == 8 else (np.uint16, 65536)
    host = [tuple(g.integers(0, top, s).astype(dt) for s in fldr_video.plane_shapes(fmt, H4, W4)) for _ in range(2)]
    d = [tuple(torch.from_numpy(p).to(dev) for p in f) for f in host]
    w = [1, 2]
    out = fldr_video.empty_frame(fmt, H4, W4, dev)
    scratch = torch.empty(L.scratch_bytes(H4, W4, fmt), dtype=torch.uint8, device=dev)
    acc = L.accumulate(curve, d, w, fmt, scratch=scratch)
    L.resolve(curve, acc, 3, H4, W4, fmt, out=out, scratch=scratch)
    want = LO.mix(host, w, curve.lin, "nv12", depth)
    if not all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(out, want)):
        raise SystemExit("accumulate + resolve differ from the oracle")
    sout = fldr_video.empty_frame(fmt, H4, W4, dev)
    L.mix(curve, d, w, fmt, out=out, scratch=scratch)
    if not all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(out, want)):
        raise SystemExit("mix differs from the oracle")
    pair = fldr_video.debug_to_planar(d, fmt)
    calls = [("to_planar", lambda: fldr_video.debug_to_planar(d, fmt, pair=pair)),
             ("from_planar", lambda: fldr_video.debug_from_planar(pair[0], fmt, out=sout)),
             ("light_accumulate", lambda: L.accumulate(curve, d, w, fmt, acc=acc, first=True, scratch=scratch)),
             ("light_resolve", lambda: L.resolve(curve, acc, 3, H4, W4, fmt, out=out, scratch=scratch)),
             ("light_mix", lambda: L.mix(curve, d, w, fmt, out=out, scratch=scratch)),
             ("shutter_mix", lambda: T.mix(d, w, fmt, out=sout))]
    return calls, curve


def kernels(a, dev, res):
    for depth in (8, 10):
        calls, curve = calls_of(dev, depth)
        kb = kernel_bytes(depth)
        moved = {"light_accumulate": kb["yuv420_to_planar_pair"] + kb["light_accumulate_kernel"],
                 "light_resolve": kb["light_resolve_kernel"] + kb["planar_to_yuv420"],
                 "light_mix": kb["yuv420_to_planar_pair"] + kb["light_mix_kernel"] + kb["planar_to_yuv420"],
                 "shutter_mix": kb["shutter_mix_kernel"], "to_planar": kb["yuv420_to_planar_pair"], "from_planar": kb["planar_to_yuv420"]}
        row = {}
        for name, call in calls:
            per = []
            for _ in range(a.alternations):
                for _ in range(5):
                    call()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    call()
                e1.record()
                torch.cuda.synchronize()
                per.append(e0.elapsed_time(e1) * 1e3 / a.steps)
            us = statistics.median(per)
            row[name] = {"us": us, "runs": per, "bytes": moved[name], "bytes_per_us": moved[name] / us}
        est = {"light_accumulate_kernel": row["light_accumulate"]["us"] - row["to_planar"]["us"],
               "light_resolve_kernel": row["light_resolve"]["us"] - row["from_planar"]["us"],
               "light_mix_kernel": row["light_mix"]["us"] - row["to_planar"]["us"] - row["from_planar"]["us"]}
        row["kernels"] = {k: {"us": v, "bytes": kb[k], "bytes_per_us": kb[k] / v if v > 0 else None} for k, v in est.items()}
        row["light_mix_kernel_over_shutter_mix"] = {"time": est["light_mix_kernel"] / row["shutter_mix"]["us"],
                                                    "bytes": kb["light_mix_kernel"] / kb["shutter_mix_kernel"]}
        row["light_mix_over_shutter_mix"] = {"time": row["light_mix"]["us"] / row["shutter_mix"]["us"],
                                             "bytes": moved["light_mix"] / moved["shutter_mix"]}
        res["calls_us"][fmt_name(depth)] = row
        res["kernel_bytes_per_launch"][fmt_name(depth)] = kb
        curve.close()


def trace(a, dev):
    calls, curve = calls_of(dev, a.depth)
    for _ in range(a.steps):
        for _, call in calls:
            call()
    torch.cuda.synchronize()
    print(json.dumps({"trace": fmt_name(a.depth), "loops": a.steps, "bytes_per_launch": kernel_bytes(a.depth)}))
    curve.close()


def pushes(a, dev, nm, res):
    fmt = fldr_video.Format("nv12", MAT, RNG)
    curve = L.Curve("gamma24", 8)
    out = {}
    for (h, w) in ((1080, 1920), (2160, 3840)):
        n = a.session_pushes
        u8 = Hn.synthetic_pair(h + 4 * n, w + 6 * n, seed=7).numpy()[0]
        clip = [O.pack_nv12(*O.bgr_to_yuv420(np.ascontiguousarray(u8[:, 4 * k:4 * k + h, 6 * k:6 * k + w]), MAT, RNG)) for k in range(n)]
        row = {}
        for name, make in (("light_120_to_24_sub1", lambda: L.Converter(nm, curve, h, w, fmt, 120, 24, (1, 2), 1, scene=True)),
                           ("shutter_120_to_24_sub1", lambda: T.Converter(nm, h, w, fmt, 120, 24, (1, 2), 1, scene=True))):
            s = make()
            s.push(clip[0])
            s.push(clip[1])                                               # warm
            t0 = time.perf_counter()
            n_out = 0
            for k in range(2, n):
                n_out += len(s.push(clip[k]))
            dt = time.perf_counter() - t0
            s.close()
            row[name] = {"ms_per_push": dt * 1e3 / (n - 2), "outputs": n_out}
        out["%dx%d" % (w, h)] = row
    res["push"] = out
    curve.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--session-pushes", type=int, default=12)
    ap.add_argument("--no-pushes", action="store_true", help="skip the push measurement")
    ap.add_argument("--trace", action="store_true", help="only a short loop of the calls, for a kernel trace")
    ap.add_argument("--depth", type=int, default=8, choices=[8, 10], help="with --trace: the depth of the frames")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.trace:
        a.steps = min(a.steps, 10)
        trace(a, dev)
        return
    nm = fldr_model.NativeModel.from_npz(Hn.DEFAULT_WEIGHTS, device=0)
    res = {"size": [H4, W4], "steps": a.steps, "device": torch.cuda.get_device_name(0), "calls_us": {}, "kernel_bytes_per_launch": {}}
    with torch.no_grad():
        kernels(a, dev, res)
        if not a.no_pushes:
            pushes(a, dev, nm, res)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    nm.close()


if __name__ == "__main__":
    main()
