#!/usr/bin/env python3
"""The rate API (libfldr_rate.so) at 3840x2160 on bench.py's frame pairs (fldr_harness.synthetic_pair, seeds 0..) as NV12 and P010
(BT.709 limited, converted by tests/yuv_oracle.py / tests/yuv_hd_oracle.py):

  * ms per pair with 3 pairs in flight on 3 streams: fldr_rate_forward against fldr_video_forward on the same pairs, alternated in the
    same run (--alternations times each), for NV12 and for P010;
  * µs per fldr_scene_measure alone (its three launches, back to back on one stream, by device events) on a textured pair and on a
    black pair, NV12 and P010;
  * Converter.push output frames/s at 1920x1080 and 3840x2160 for 24 -> 60 with the cut detector on and off, beside Session.push with
    n_t = 2 from the same run (host frames in and out: includes PCIe and host copies).

    python tools/bench_rate.py [--steps 20] [--warmup 3] [--alternations 3] [--out profiles/rate_forward.json]

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_rate.py --trace textured|black [--depth 8|10]
        a short loop of fldr_rate_forward on one kind of pair only, for the kernel trace: scene_accumulate_kernel beside
        yuv420_to_planar_pair_kernel (the input converter, which moves 4.5 times the bytes) in one table.

Every frame of the timed loops is checked before timing: the outputs against fldr_video_forward's bytes, the measure against
tests/scene_oracle.py."""
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
import fldr_video  # noqa: E402
import scene_oracle as S  # noqa: E402
import yuv_hd_oracle as HD  # noqa: E402
import yuv_oracle as O  # noqa: E402

MAT, RNG = "bt709", "limited"


def host_pair(H, W, seed, depth):
    """(planes of I0, planes of I1) as NV12 / P010 of synthetic_pair(seed)."""
    u8 = Hn.synthetic_pair(H, W, seed=seed).numpy()
    if depth == 8:
        return [O.pack_nv12(*O.bgr_to_yuv420(u8[i], MAT, RNG)) for i in range(2)]
    w = (u8.astype(np.uint16) << 2) | (u8 >> 6)
    return [HD.pack_planes(*HD.bgr_to_yuv420(w[i], MAT, RNG, 10), "nv12", 10) for i in range(2)]


def black_pair(H, W, depth):
    dt, y, c = (np.uint8, 16, 128) if depth == 8 else (np.uint16, 64 << 6, 512 << 6)
    return [(np.full((H, W), y, dt), np.full(((H + 1) // 2, 2 * ((W + 1) // 2)), c, dt)) for _ in range(2)]


def to_dev(planes, dev):
    return tuple(torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in planes)


def trace(a, dev, nr):
    """A short loop for rocprofv3 --kernel-trace --stats."""
    H, W = 2160, 3840
    fmt = fldr_video.Format("nv12", MAT, RNG, a.depth)
    pair = black_pair(H, W, a.depth) if a.trace == "black" else host_pair(H, W, 0, a.depth)
    frames = [to_dev(p, dev) for p in pair]
    t = torch.tensor([0.5], device=dev)
    ws = nr.workspace(H, W)
    outs = [fldr_video.empty_frame(fmt, H, W, dev)]
    for _ in range(a.steps):
        nr.forward(frames, t, fmt, outs=outs, ws=ws, read=False)
    torch.cuda.synchronize()
    print(json.dumps({"trace": a.trace, "depth": a.depth, "forwards": a.steps,
                      "scene": fldr_rate.read_result(nr.state_of(ws, H, W)), "oracle": S.measure(pair[0], pair[1], fmt)}))


def in_flight(a, dev, nm, nr, depth, res):
    H, W, NS = 2160, 3840, a.streams
    NP = max(NS + 1, 4)
    nv = fldr_video.NativeVideo(nm)
    fmt = fldr_video.Format("nv12", MAT, RNG, depth)
    host = [host_pair(H, W, p, depth) for p in range(NP)]
    pairs = [[to_dev(f, dev) for f in pr] for pr in host]
    t = torch.tensor([0.5], device=dev)
    streams = [torch.cuda.Stream(device=dev) for _ in range(NS)]
    ws_r = [nr.workspace(H, W) for _ in range(NS)]
    ws_v = [nv.workspace(H, W) for _ in range(NS)]
    outs_r = [[fldr_video.empty_frame(fmt, H, W, dev)] for _ in range(NS)]
    outs_v = [[fldr_video.empty_frame(fmt, H, W, dev)] for _ in range(NS)]

    def rate_step(i):
        return nr.forward(pairs[i % NP], t, fmt, outs=outs_r[i % NS], ws=ws_r[i % NS], read=False)[0][0]

    def video_step(i):
        return nv.forward(pairs[i % NP], t, fmt, fmt, outs=outs_v[i % NS], ws=ws_v[i % NS])[0]

    for i in range(NP * NS):                                             # the expected bytes, pair by pair and stream by stream
        with torch.cuda.stream(streams[i % NS]):
            gr, gv = rate_step(i), video_step(i)
        torch.cuda.synchronize()
        if not all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(gr, gv)):
            raise SystemExit("fldr_rate_forward's output of pair %d differs from fldr_video_forward's" % (i % NP))
        got, want = fldr_rate.read_result(nr.state_of(ws_r[i % NS], H, W)), S.measure(host[i % NP][0], host[i % NP][1], fmt)
        if got != want or got["cut"]:
            raise SystemExit("the measure of pair %d is %r, the oracle's %r" % (i % NP, got, want))

    def ms_per_pair(step):
        for i in range(a.warmup * NS):
            with torch.cuda.stream(streams[i % NS]):
                step(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = a.steps * NS
        for i in range(n):
            with torch.cuda.stream(streams[i % NS]):
                step(i)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    runs = {"rate_forward": [], "video_forward": []}
    for _ in range(a.alternations):
        runs["rate_forward"].append(ms_per_pair(rate_step))
        runs["video_forward"].append(ms_per_pair(video_step))
    med = {k: statistics.median(v) for k, v in runs.items()}
    res["ms_per_pair_in_flight"][fmt_name(depth)] = {"runs": runs, "median": med, "rate_vs_video": med["rate_forward"] / med["video_forward"]}

    # the measure alone: textured and black
    alone = {}
    for kind, pr in (("textured", host[0]), ("black", black_pair(H, W, depth))):
        frames = [to_dev(f, dev) for f in pr]
        st = fldr_rate.scene_state(dev)
        if fldr_rate.scene_measure(frames, fmt, state=st) != S.measure(pr[0], pr[1], fmt):
            raise SystemExit("the measure of the %s pair differs from the oracle's" % kind)
        n = 50
        per = []
        for _ in range(a.alternations):
            for _ in range(5):
                fldr_rate.scene_measure(frames, fmt, state=st, read=False)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fldr_rate.scene_measure(frames, fmt, state=st, read=False)
            e1.record()
            torch.cuda.synchronize()
            per.append(e0.elapsed_time(e1) * 1e3 / n)
        alone[kind] = {"us_per_measure": statistics.median(per), "runs": per}
    res["measure_alone_us"][fmt_name(depth)] = alone


def fmt_name(depth):
    return "nv12" if depth == 8 else "p010"


def sessions(a, dev, nm, res):
    fmt = fldr_video.Format("nv12", MAT, RNG)
    out = {}
    for (h, w) in ((1080, 1920), (2160, 3840)):
        n = a.session_pushes
        u8 = Hn.synthetic_pair(h + 4 * n, w + 6 * n, seed=7).numpy()[0]
        clip = [O.pack_nv12(*O.bgr_to_yuv420(np.ascontiguousarray(u8[:, 4 * k:4 * k + h, 6 * k:6 * k + w]), MAT, RNG)) for k in range(n)]
        row = {}
        for name, make in (("converter_24_to_60_scene_on", lambda: fldr_rate.Converter(nm, h, w, fmt, 24, 60, scene=True)),
                           ("converter_24_to_60_scene_off", lambda: fldr_rate.Converter(nm, h, w, fmt, 24, 60, scene=False)),
                           ("session_nt2", lambda: fldr_video.Session(nm, h, w, 2, fmt, fmt))):
            s = make()
            s.push(clip[0])
            s.push(clip[1])                                               # warm
            t0 = time.perf_counter()
            n_out = 0
            for k in range(2, n):
                n_out += len(s.push(clip[k]))
            dt = time.perf_counter() - t0
            s.close()
            row[name] = {"output_frames_per_s": n_out / dt, "ms_per_push": dt * 1e3 / (n - 2), "outputs": n_out}
        out["%dx%d" % (w, h)] = row
    res["push"] = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--streams", type=int, default=3)
    ap.add_argument("--session-pushes", type=int, default=12)
    ap.add_argument("--no-sessions", action="store_true", help="skip the push measurement")
    ap.add_argument("--trace", choices=["textured", "black"], default=None, help="only a short fldr_rate_forward loop, for a kernel trace")
    ap.add_argument("--depth", type=int, default=8, choices=[8, 10], help="with --trace: the depth of the pair")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    nm = fldr_model.NativeModel.from_npz(Hn.DEFAULT_WEIGHTS, device=0)
    nr = fldr_rate.NativeRate(nm)
    if a.trace:
        trace(a, dev, nr)
        nm.close()
        return
    res = {"size": [2160, 3840], "streams": a.streams, "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "ms_per_pair_in_flight": {}, "measure_alone_us": {}}
    with torch.no_grad():
        for depth in (8, 10):
            in_flight(a, dev, nm, nr, depth, res)
        if not a.no_sessions:
            sessions(a, dev, nm, res)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    nm.close()


if __name__ == "__main__":
    main()
