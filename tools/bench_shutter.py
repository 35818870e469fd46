#!/usr/bin/env python3
"""The shutter API (libfldr_shutter.so) on random NV12 and P010 frames at 3840x2160, and its converter on a moving texture:

  * µs per fldr_shutter_accumulate (n = 1, 4, 8 frames onto a held accumulator), fldr_shutter_resolve and fldr_shutter_mix (n = 8), by
    device events over back-to-back launches on one stream, with the bytes each moves (frames read, the accumulator's 4 bytes per
    sample read and written, the frame written) and bytes per µs;
  * Converter.push ms for 120 -> 24 (sub = 1 and 4) and 60 -> 24 (sub = 4), 180 degrees, at 1920x1080 and 3840x2160, beside
    fldr_rate.Converter.push on the same clip in the same run (host frames in and out: includes PCIe and host copies).

    python tools/bench_shutter.py [--steps 50] [--alternations 3] [--out profiles/shutter_forward.json]

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_shutter.py --trace [--depth 8|10]
        a short loop of the five kernel calls and of fldr_rate_forward on one pair, for the kernel trace: the shutter kernels beside
        yuv420_to_planar_pair_kernel (the input converter) and scene_accumulate_kernel in one table.  The JSON line it prints carries
        the bytes each of them moves per launch, to set against the table's times.

Every kernel result is checked against tests/shutter_oracle.py before timing."""
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
import fldr_model  # noqa: E402
import fldr_rate  # noqa: E402
import fldr_shutter as T  # noqa: E402
import fldr_video  # noqa: E402
import shutter_oracle as SO  # noqa: E402
import yuv_oracle as O  # noqa: E402

MAT, RNG = "bt709", "limited"
H4, W4 = 2160, 3840


def fmt_name(depth):
    return "nv12" if depth == 8 else "p010"


def kernel_calls(dev, depth):
    """[(name, bytes moved, callable)] on eight random 4K frames, checked against the oracle."""
    fmt = fldr_video.Format("nv12", MAT, RNG, depth)
    g = np.random.default_rng(depth)
    dt, top = (np.uint8, 256) if depth == 8 else (np.uint16, 65536)
    host = [tuple(g.integers(0, top, s).astype(dt) for s in fldr_video.plane_shapes(fmt, H4, W4)) for _ in range(8)]
    d = [tuple(torch.from_numpy(p).to(dev) for p in f) for f in host]
    w = [1, 2, 3, 4, 5, 6, 7, 8]
    out = fldr_video.empty_frame(fmt, H4, W4, dev)
    acc = T.accumulate(d, w, fmt)
    T.resolve(acc, sum(w), H4, W4, fmt, out=out)
    want = SO.mix(host, w, "nv12", depth)
    if not all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(out, want)):
        raise SystemExit("accumulate + resolve differ from the oracle")
    T.mix(d, w, fmt, out=out)
    if not all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(out, want)):
        raise SystemExit("mix differs from the oracle")
    samples = H4 * W4 * 3 // 2
    F, A = samples * (2 if depth == 10 else 1), 4 * samples
    calls = [("accumulate_n%d" % n, n * F + 2 * A, (lambda n=n: T.accumulate(d[:n], w[:n], fmt, acc=acc, first=False))) for n in (1, 4, 8)]
    calls.append(("resolve", A + F, lambda: T.resolve(acc, 36, H4, W4, fmt, out=out)))
    calls.append(("mix_n8", 9 * F, lambda: T.mix(d, w, fmt, out=out)))
    return calls, acc


def kernels(a, dev, res):
    for depth in (8, 10):
        calls, acc = kernel_calls(dev, depth)
        row = {}
        for name, nbytes, call in calls:
            per = []
            for _ in range(a.alternations):
                for _ in range(5):
                    call()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                acc.zero_()                                              # the sums of the timed launches stay far inside 32 bits
                e0.record()
                for _ in range(a.steps):
                    call()
                e1.record()
                torch.cuda.synchronize()
                per.append(e0.elapsed_time(e1) * 1e3 / a.steps)
            us = statistics.median(per)
            row[name] = {"us": us, "runs": per, "bytes": nbytes, "bytes_per_us": nbytes / us}
        res["kernels_us"][fmt_name(depth)] = row


def trace(a, dev, nm):
    calls, acc = kernel_calls(dev, a.depth)
    fmt = fldr_video.Format("nv12", MAT, RNG, a.depth)
    nr = fldr_rate.NativeRate(nm)
    g = np.random.default_rng(1)
    dt, top = (np.uint8, 256) if a.depth == 8 else (np.uint16, 65536)
    frames = [tuple(torch.from_numpy(g.integers(0, top, s).astype(dt)).to(dev) for s in fldr_video.plane_shapes(fmt, H4, W4)) for _ in range(2)]
    t = torch.tensor([0.5], device=dev)
    ws = nr.workspace(H4, W4)
    outs = [fldr_video.empty_frame(fmt, H4, W4, dev)]
    for _ in range(a.steps):
        acc.zero_()
        for _, _, call in calls:
            call()
        nr.forward(frames, t, fmt, outs=outs, ws=ws, read=False)
    torch.cuda.synchronize()
    b = 2 if a.depth == 10 else 1
    moved = {name: nbytes for name, nbytes, _ in calls}
    moved["yuv420_to_planar_pair_kernel"] = (3 + 6) * H4 * W4 * b       # two frames in, the planar pair out
    moved["scene_accumulate_kernel"] = 2 * H4 * W4 * b                   # the two luma planes
    print(json.dumps({"trace": fmt_name(a.depth), "loops": a.steps, "bytes_per_launch": moved}))


def pushes(a, dev, nm, res):
    fmt = fldr_video.Format("nv12", MAT, RNG)
    out = {}
    for (h, w) in ((1080, 1920), (2160, 3840)):
        n = a.session_pushes
        u8 = Hn.synthetic_pair(h + 4 * n, w + 6 * n, seed=7).numpy()[0]
        clip = [O.pack_nv12(*O.bgr_to_yuv420(np.ascontiguousarray(u8[:, 4 * k:4 * k + h, 6 * k:6 * k + w]), MAT, RNG)) for k in range(n)]
        row = {}
        for name, make in (("shutter_120_to_24_sub1", lambda: T.Converter(nm, h, w, fmt, 120, 24, (1, 2), 1, scene=True)),
                           ("shutter_120_to_24_sub4", lambda: T.Converter(nm, h, w, fmt, 120, 24, (1, 2), 4, scene=True)),
                           ("shutter_60_to_24_sub4", lambda: T.Converter(nm, h, w, fmt, 60, 24, (1, 2), 4, scene=True)),
                           ("rate_120_to_24", lambda: fldr_rate.Converter(nm, h, w, fmt, 120, 24, scene=True)),
                           ("rate_60_to_24", lambda: fldr_rate.Converter(nm, h, w, fmt, 60, 24, scene=True))):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--session-pushes", type=int, default=12)
    ap.add_argument("--no-pushes", action="store_true", help="skip the push measurement")
    ap.add_argument("--trace", action="store_true", help="only a short loop of the kernels and of fldr_rate_forward, for a kernel trace")
    ap.add_argument("--depth", type=int, default=8, choices=[8, 10], help="with --trace: the depth of the frames")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    nm = fldr_model.NativeModel.from_npz(Hn.DEFAULT_WEIGHTS, device=0)
    if a.trace:
        a.steps = min(a.steps, 10)
        trace(a, dev, nm)
        nm.close()
        return
    res = {"size": [H4, W4], "steps": a.steps, "device": torch.cuda.get_device_name(0), "kernels_us": {}}
    with torch.no_grad():
        kernels(a, dev, res)
        if not a.no_pushes:
            pushes(a, dev, nm, res)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    nm.close()


if __name__ == "__main__":
    main()
