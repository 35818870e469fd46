#!/usr/bin/env python3
"""libfldr_chroma.so at 3840x2160, BT.709 limited:

  * each converter alone (fldr_chroma_to_planar on one frame, fldr_chroma_from_planar) for P210, yuv422p10le, UYVY, NV16, yuv444p and
    yuv444p10le: microseconds per launch and effective GB/s (bytes read plus bytes written over the time).  The launches are captured
    into a graph (64 per graph, rotating over --buffers frame sets so that the working set exceeds the 256 MiB Infinity Cache) and the
    graph is replayed between two device events, so the figure is the kernel's, not the host's launch rate;
  * fldr_chroma_forward (P210 -> P210, NV16 -> NV16) beside fldr_video_forward (P010 -> P010, NV12 -> NV12) and the model's own planar
    forward of the same depth, n_t = 1, one stream, alternated in the same run (--alternations windows of --steps forwards each).  The
    conversion overhead of a forward is its time minus the model forward's; per byte it is divided by the bytes its two conversions move.
    The yardstick is the 4:2:0 figure; its spread over the alternations is the margin.

    python tools/bench_chroma.py [--steps 100] [--warmup 5] [--alternations 5] [--out profiles/chroma.json]"""
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

import fldr_chroma as V  # noqa: E402
import fldr_harness as Hn  # noqa: E402
import fldr_model  # noqa: E402
import fldr_video  # noqa: E402
import yuv_hd_oracle as HD  # noqa: E402

MAT, RNG = "bt709", "limited"
H, W = 2160, 3840
CONVERTERS = [("p210", "422", "semiplanar", 10), ("yuv422p10le", "422", "planar", 10), ("uyvy", "422", "uyvy", 8), ("nv16", "422", "semiplanar", 8),
              ("yuv444p", "444", "planar", 8), ("yuv444p10le", "444", "planar", 10)]


def frame_bytes(fmt):
    return sum(r * c for r, c in V.plane_shapes(fmt, H, W)) * (2 if fmt.bits == 10 else 1)


def planar_bytes(fmt):
    return 3 * H * W * (2 if fmt.bits == 10 else 1)


def graph_time_us(launch, n_per_graph, replays, stream):
    """Median over 5 windows of the time of one launch, from `replays` replays of a graph of n_per_graph launches."""
    with torch.cuda.stream(stream):
        for i in range(n_per_graph):
            launch(i)                                                          # warm: code objects loaded before the capture
    stream.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        for i in range(n_per_graph):
            launch(i)
    g.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(replays):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / (replays * n_per_graph))
    return statistics.median(times), times


def converters(a, dev):
    res = {}
    st = torch.cuda.Stream(device=dev)
    g = np.random.default_rng(0)
    for name, s, l, d in CONVERTERS:
        fmt = V.Format(s, l, MAT, RNG, d)
        dt, ndt = V.plane_dtype(fmt), V.plane_dtype(fmt, numpy=True)
        mx = 1023 if d == 10 else 255
        shift = 6 if (d == 10 and l == "semiplanar") else 0
        frames, planars = [], []
        for _ in range(a.buffers):
            frames.append(tuple(torch.from_numpy(g.integers(0, mx + 1, sh).astype(ndt) << shift).to(dev) for sh in V.plane_shapes(fmt, H, W)))
            planars.append(torch.from_numpy(g.integers(0, mx + 1, (1, 3, H, W)).astype(ndt)).to(dev))
        outs = [V.empty_frame(fmt, H, W, dev) for _ in range(a.buffers)]
        dsts = [torch.empty(1, 3, H, W, dtype=dt, device=dev) for _ in range(a.buffers)]
        nb = frame_bytes(fmt) + planar_bytes(fmt)
        us_in, runs_in = graph_time_us(lambda i: V.to_planar([frames[i % a.buffers]], fmt, planar=dsts[i % a.buffers]), 64, a.replays, st)
        us_out, runs_out = graph_time_us(lambda i: V.from_planar(planars[i % a.buffers][0], fmt, out=outs[i % a.buffers]), 64, a.replays, st)
        res[name] = {"bytes_moved": nb,
                     "to_planar": {"us": us_in, "GBps": nb / us_in * 1e-3, "windows_us": runs_in},
                     "from_planar": {"us": us_out, "GBps": nb / us_out * 1e-3, "windows_us": runs_out}}
        del frames, planars, outs, dsts
        torch.cuda.empty_cache()
    return res


def pair_of_depth(d, seed):
    u8 = Hn.synthetic_pair(H, W, seed=seed).numpy()
    return u8 if d == 8 else ((u8.astype(np.uint16) << 2) | (u8 >> 6))


def forwards(a, dev, nm):
    nc, nv = V.NativeChroma(nm), fldr_video.NativeVideo(nm)
    t = torch.tensor([0.5], device=dev)
    steps = {}
    moved = {}
    for d in (8, 10):
        bgr = pair_of_depth(d, 0)
        bgr_dev = torch.from_numpy(bgr)[None].to(dev)
        cf = V.Format("422", "semiplanar", MAT, RNG, d)                        # NV16 / P210
        cframes = [V.from_planar(bgr_dev[0, i], cf) for i in range(2)]
        vf = fldr_video.Format("nv12", MAT, RNG, d)                            # NV12 / P010
        vframes = [tuple(torch.from_numpy(x).to(dev) for x in HD.pack_planes(*HD.bgr_to_yuv420(bgr[i], MAT, RNG, d), "nv12", d)) for i in range(2)]
        ws_c, ws_v, ws_m = nc.workspace(H, W), nv.workspace(H, W), nm.workspace(H, W)
        outs_c, outs_v = [V.empty_frame(cf, H, W, dev)], [fldr_video.empty_frame(vf, H, W, dev)]
        tag = "u%d" % d
        steps["chroma_" + tag] = (lambda cframes=cframes, cf=cf, outs_c=outs_c, ws_c=ws_c: nc.forward(cframes, t, cf, cf, outs=outs_c, ws=ws_c))
        steps["video_" + tag] = (lambda vframes=vframes, vf=vf, outs_v=outs_v, ws_v=ws_v: nv.forward(vframes, t, vf, vf, outs=outs_v, ws=ws_v))
        if d == 8:
            steps["model_" + tag] = (lambda bgr_dev=bgr_dev, ws_m=ws_m: nm.interpolate_u8(bgr_dev, t, ws=ws_m))
        else:
            steps["model_" + tag] = (lambda bgr_dev=bgr_dev, ws_m=ws_m: nm.interpolate_u10(bgr_dev, t, ws=ws_m))
        b = 2 if d == 10 else 1
        # bytes the two conversions of one forward move: two frames in + the planar pair out, one planar frame in + one frame out
        moved["chroma_" + tag] = 3 * (frame_bytes(cf) + planar_bytes(cf))
        moved["video_" + tag] = 3 * ((H * W + 2 * ((H + 1) // 2) * ((W + 1) // 2)) * b + 3 * H * W * b)

    def window(step):
        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.steps

    runs = {k: [] for k in steps}
    with torch.no_grad():
        for _ in range(a.alternations):
            for k, step in steps.items():
                runs[k].append(window(step))
    res = {"ms_per_forward": {"runs": runs, "median": {k: statistics.median(v) for k, v in runs.items()}}, "conversion_bytes": moved}
    over = {}
    for k in moved:
        m = "model_" + k.split("_")[1]
        per = [(x - y) * 1e6 / moved[k] for x, y in zip(runs[k], runs[m])]     # ns per byte, window by window
        over[k] = {"overhead_ms_median": statistics.median(x - y for x, y in zip(runs[k], runs[m])), "ns_per_byte": per,
                   "ns_per_byte_median": statistics.median(per), "ns_per_byte_min": min(per), "ns_per_byte_max": max(per)}
    res["conversion_overhead"] = over
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--buffers", type=int, default=8)
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    nm = fldr_model.NativeModel.from_npz(Hn.DEFAULT_WEIGHTS, device=0)
    res = {"size": [H, W], "format": "%s %s" % (MAT, RNG), "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup,
           "alternations": a.alternations, "buffers": a.buffers}
    res["converters"] = converters(a, dev)
    res["forward"] = forwards(a, dev, nm)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    nm.close()


if __name__ == "__main__":
    main()
