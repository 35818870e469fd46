#!/usr/bin/env python3
"""libfldr_pack10.so at 3840x2160 and 4096x2160, BT.709 limited, beside libfldr_chroma.so in the same run:

  * each converter alone (to_planar on one frame, from_planar) for v210 at its customary pitch (128 bytes per 48 pixels), Y210 and Y410
    with tight rows, and the chroma library's P210 and yuv422p10le converters as the yardstick: microseconds per launch, bytes read plus
    written and TB/s.  The launches are captured into a graph (64 per graph, rotating over --buffers frame sets so that the working set
    exceeds the 256 MiB Infinity Cache) and the graph is replayed between two device events (tools/bench_chroma.py's graph_time_us).  The
    whole list is measured --rounds times in turn, so that every figure has a spread and the comparisons are between neighbours in time;
  * a v210 -> v210 forward beside a P210 -> P210 forward and the model's own 10-bit planar forward at 3840x2160, n_t = 1, one stream,
    alternated (--alternations windows of --steps forwards each).

The expectations set when the library was added are evaluated and written out (`checks`), never enforced: a v210 converter
should take no longer than the P210 one of the same run at either width (+ 5 %), and the 4096-wide v210 frame (4096 % 6 = 4) should cost
no more per byte than the 3840-wide one (+ 5 %).

    python tools/bench_pack10.py [--steps 100] [--warmup 5] [--alternations 5] [--rounds 3] [--out profiles/pack10.json]"""
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

import fldr_chroma as K  # noqa: E402
import fldr_harness as Hn  # noqa: E402
import fldr_model  # noqa: E402
import fldr_pack10 as V  # noqa: E402
from bench_chroma import graph_time_us  # noqa: E402

MAT, RNG = "bt709", "limited"
SIZES = [(2160, 3840), (2160, 4096)]
MARGIN = 1.05


def pack10_case(name, H, W, dev, g, buffers):
    """-> (bytes moved, launch of to_planar, launch of from_planar) for container `name` on `buffers` rotating frame sets."""
    fmt = V.Format(name, MAT, RNG)
    (rows, words), = V.plane_shapes(fmt, H, W)
    ndt = V.plane_dtype(fmt, numpy=True)
    item = np.dtype(ndt).itemsize
    pitch_words = V.v210_pitch(W) // 4 if name == "v210" else words

    def plane(fill):
        host = np.zeros((rows, pitch_words), ndt)
        if fill:
            host[:, :words] = g.integers(0, 1 << (8 * item), (rows, words), dtype=ndt)
        return (torch.from_numpy(host).to(dev)[:, :words],)
    frames, outs = [plane(True) for _ in range(buffers)], [plane(False) for _ in range(buffers)]
    planars = [torch.from_numpy(g.integers(0, 1024, (1, 3, H, W)).astype(np.uint16)).to(dev) for _ in range(buffers)]
    dsts = [torch.empty(1, 3, H, W, dtype=torch.uint16, device=dev) for _ in range(buffers)]
    nb = rows * words * item + 6 * H * W
    return (nb, lambda i: V.to_planar([frames[i % buffers]], fmt, planar=dsts[i % buffers], W=W),
            lambda i: V.from_planar(planars[i % buffers][0], fmt, out=outs[i % buffers]))


def chroma_case(layout, H, W, dev, g, buffers):
    fmt = K.Format("422", layout, MAT, RNG, 10)
    shift = 6 if layout == "semiplanar" else 0
    frames = [tuple(torch.from_numpy(g.integers(0, 1024, sh).astype(np.uint16) << shift).to(dev) for sh in K.plane_shapes(fmt, H, W))
              for _ in range(buffers)]
    outs = [K.empty_frame(fmt, H, W, dev) for _ in range(buffers)]
    planars = [torch.from_numpy(g.integers(0, 1024, (1, 3, H, W)).astype(np.uint16)).to(dev) for _ in range(buffers)]
    dsts = [torch.empty(1, 3, H, W, dtype=torch.uint16, device=dev) for _ in range(buffers)]
    nb = 2 * sum(r * c for r, c in K.plane_shapes(fmt, H, W)) + 6 * H * W
    return (nb, lambda i: K.to_planar([frames[i % buffers]], fmt, planar=dsts[i % buffers]),
            lambda i: K.from_planar(planars[i % buffers][0], fmt, out=outs[i % buffers]))


def converters(a, dev):
    res = {}
    st = torch.cuda.Stream(device=dev)
    g = np.random.default_rng(0)
    for H, W in SIZES:
        cases = {}
        for name in ("v210", "y210", "y410"):
            cases[name] = pack10_case(name, H, W, dev, g, a.buffers)
        for name, layout in (("p210", "semiplanar"), ("yuv422p10le", "planar")):
            cases[name] = chroma_case(layout, H, W, dev, g, a.buffers)
        runs = {name: {"to_planar": [], "from_planar": []} for name in cases}
        for _ in range(a.rounds):
            for name, (nb, to, frm) in cases.items():
                runs[name]["to_planar"].append(graph_time_us(to, 64, a.replays, st)[0])
                runs[name]["from_planar"].append(graph_time_us(frm, 64, a.replays, st)[0])
        size = {}
        for name, (nb, _, _) in cases.items():
            size[name] = {"bytes_moved": nb, "bytes_per_pixel": nb / (H * W)}
            for d in ("to_planar", "from_planar"):
                us = statistics.median(runs[name][d])
                size[name][d] = {"us": us, "TBps": nb / us * 1e-6, "ns_per_MB": us * 1e3 / (nb * 1e-6), "rounds_us": runs[name][d],
                                 "spread": (max(runs[name][d]) - min(runs[name][d])) / us}
        res["%dx%d" % (W, H)] = size
        del cases
        torch.cuda.empty_cache()
    return res


def forwards(a, dev, nm):
    H, W = SIZES[0]
    npk, kc = V.NativePack10(nm), K.NativeChroma(nm)
    t = torch.tensor([0.5], device=dev)
    u8 = Hn.synthetic_pair(H, W, seed=0).numpy()
    bgr_dev = torch.from_numpy((u8.astype(np.uint16) << 2) | (u8 >> 6))[None].to(dev)
    vf, kf = V.Format("v210", MAT, RNG), K.Format("422", "semiplanar", MAT, RNG, 10)
    vframes = [V.from_planar(bgr_dev[0, i], vf) for i in range(2)]
    kframes = [K.from_planar(bgr_dev[0, i], kf) for i in range(2)]
    ws_v, ws_k, ws_m = npk.workspace(H, W), kc.workspace(H, W), nm.workspace(H, W)
    outs_v, outs_k = [V.empty_frame(vf, H, W, dev)], [K.empty_frame(kf, H, W, dev)]
    steps = {"v210": lambda: npk.forward(vframes, t, vf, vf, outs=outs_v, ws=ws_v, W=W),
             "p210": lambda: kc.forward(kframes, t, kf, kf, outs=outs_k, ws=ws_k),
             "model_u10": lambda: nm.interpolate_u10(bgr_dev, t, ws=ws_m)}

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
    return {"size": [H, W], "ms_per_forward": {"runs": runs, "median": {k: statistics.median(v) for k, v in runs.items()}},
            "conversion_overhead_ms_median": {k: statistics.median(x - y for x, y in zip(runs[k], runs["model_u10"])) for k in ("v210", "p210")}}


def checks(conv):
    out = {}
    small, large = ("%dx%d" % (W, H) for H, W in SIZES)
    for d in ("to_planar", "from_planar"):
        for size in (small, large):
            v, p = conv[size]["v210"][d]["us"], conv[size]["p210"][d]["us"]
            out["v210_%s_%s_vs_p210" % (d, size)] = {"v210_us": v, "p210_us": p, "ratio": v / p, "within_5_percent": v <= MARGIN * p}
        s, l = conv[small]["v210"][d]["ns_per_MB"], conv[large]["v210"][d]["ns_per_MB"]
        out["v210_%s_per_byte_4096_vs_3840" % d] = {"ns_per_MB_3840": s, "ns_per_MB_4096": l, "ratio": l / s, "within_5_percent": l <= MARGIN * s}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--buffers", type=int, default=8)
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"sizes": SIZES, "format": "%s %s" % (MAT, RNG), "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup,
           "alternations": a.alternations, "rounds": a.rounds, "buffers": a.buffers, "replays": a.replays}
    res["converters"] = converters(a, dev)
    res["checks"] = checks(res["converters"])
    nm = fldr_model.NativeModel.from_npz(Hn.DEFAULT_WEIGHTS, device=0)
    res["forward"] = forwards(a, dev, nm)
    nm.close()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
