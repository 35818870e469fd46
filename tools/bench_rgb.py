#!/usr/bin/env python3
"""libfldr_rgb.so at 3840x2160 and 4096x2160, beside the Y410 converters of libfldr_pack10.so in the same run:

  * each converter alone (to_planar on one frame, from_planar) for every layout and depth with tight rows, and the packed 10-bit
    library's Y410 converters as the yardstick: microseconds per launch, bytes read plus written and TB/s.  The launches are captured
    into a graph (64 per graph, rotating over --buffers frame sets so that the working set exceeds the 256 MiB Infinity Cache) and the
    graph is replayed between two device events (tools/bench_chroma.py's graph_time_us).  The whole list is measured --rounds times in
    turn, so that every figure has a spread and the comparisons are between neighbours in time;
  * the alpha pass alone (fldr_rgb_alpha, one output) for NEARER and BLEND, on BGRA, X2RGB10 and GBRAP frames, the same way;
  * BGRA -> BGRA and X2RGB10 -> X2RGB10 forwards (OPAQUE) beside the model's own planar 8- and 10-bit forwards at 3840x2160, n_t = 1,
    one stream, alternated (--alternations windows of --steps forwards each).

The expectation set when the library was added is evaluated and written out (`checks`), never enforced: X2RGB10 moves the bytes of Y410
(4 W in, 6 W out per row) with less arithmetic, so each of its converters should take no longer than the Y410 one of the same run
(+ 10 %).

    python tools/bench_rgb.py [--steps 100] [--warmup 5] [--alternations 5] [--rounds 3] [--out profiles/rgb.json]"""
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
import fldr_pack10 as P  # noqa: E402
import fldr_rgb as V  # noqa: E402
from bench_chroma import graph_time_us  # noqa: E402

SIZES = [(2160, 3840), (2160, 4096)]
FORMATS = [("bgra", 8), ("rgba", 8), ("argb", 8), ("abgr", 8), ("x2rgb10", 10), ("x2bgr10", 10), ("gbrp", 8), ("gbrap", 8), ("gbrp", 10), ("gbrap", 10)]
ALPHA_FORMATS = [("bgra", 8), ("x2rgb10", 10), ("gbrap", 8), ("gbrap", 10)]
MARGIN = 1.10


def _name(layout, depth):
    return "%s_%d" % (layout, depth)


def _frames(fmt, H, W, dev, g, buffers, fill=True):
    ndt = V.plane_dtype(fmt, numpy=True)
    top = 1 << (10 if ndt == np.uint16 else 8 * np.dtype(ndt).itemsize)
    out = []
    for _ in range(buffers):
        out.append(tuple(torch.from_numpy(g.integers(0, top, s, dtype=ndt) if fill else np.zeros(s, ndt)).to(dev) for s in V.plane_shapes(fmt, H, W)))
    return out


def _plane_bytes(fmt, H, W):
    return [r * c * np.dtype(V.plane_dtype(fmt, numpy=True)).itemsize for r, c in V.plane_shapes(fmt, H, W)]


def rgb_case(layout, depth, H, W, dev, g, buffers):
    """-> (bytes to_planar moves, bytes from_planar moves, launch of to_planar, launch of from_planar) on `buffers` rotating frame sets."""
    fmt = V.Format(layout, depth)
    frames, outs = _frames(fmt, H, W, dev, g, buffers), _frames(fmt, H, W, dev, g, buffers, fill=False)
    pdt = V.planar_dtype(fmt, numpy=True)
    planars = [torch.from_numpy(g.integers(0, 1 << depth, (1, 3, H, W)).astype(pdt)).to(dev) for _ in range(buffers)]
    dsts = [torch.empty(1, 3, H, W, dtype=V.planar_dtype(fmt), device=dev) for _ in range(buffers)]
    pb, planar_bytes = _plane_bytes(fmt, H, W), 3 * H * W * np.dtype(pdt).itemsize
    return (sum(pb[:3]) + planar_bytes, sum(pb) + planar_bytes,              # to_planar never reads an A plane; from_planar fills it
            lambda i: V.to_planar([frames[i % buffers]], fmt, planar=dsts[i % buffers]),
            lambda i: V.from_planar(planars[i % buffers][0], fmt, out=outs[i % buffers]))


def y410_case(H, W, dev, g, buffers):
    fmt = P.Format("y410", "bt709", "limited")
    frames = [(torch.from_numpy(g.integers(0, 1 << 32, (H, W), dtype=np.uint32)).to(dev),) for _ in range(buffers)]
    outs = [(torch.zeros(H, W, dtype=torch.uint32, device=dev),) for _ in range(buffers)]
    planars = [torch.from_numpy(g.integers(0, 1024, (1, 3, H, W)).astype(np.uint16)).to(dev) for _ in range(buffers)]
    dsts = [torch.empty(1, 3, H, W, dtype=torch.uint16, device=dev) for _ in range(buffers)]
    nb = 4 * H * W + 6 * H * W
    return (nb, nb, lambda i: P.to_planar([frames[i % buffers]], fmt, planar=dsts[i % buffers], W=W),
            lambda i: P.from_planar(planars[i % buffers][0], fmt, out=outs[i % buffers]))


def alpha_case(layout, depth, policy, H, W, dev, g, buffers):
    """-> (bytes one launch moves, the launch): the alpha of one output frame from two inputs, all in (layout, depth)."""
    fin, fout = V.Format(layout, depth), V.Format(layout, depth, policy)
    a, b, outs = (_frames(fin, H, W, dev, g, buffers) for _ in range(3))
    t = torch.tensor([0.25], device=dev)
    unit = _plane_bytes(fin, H, W)[-1]                                          # the pixel words, or the A plane
    reads = (2 if policy == "blend" else 1) + (1 if layout != "gbrap" else 0)   # the inputs, and the words rewritten
    return (reads + 1) * unit, lambda i: V.alpha([a[i % buffers], b[i % buffers]], fin, [outs[i % buffers]], fout, t)


def _stats(nb, runs):
    us = statistics.median(runs)
    return {"us": us, "bytes_moved": nb, "TBps": nb / us * 1e-6, "ns_per_MB": us * 1e3 / (nb * 1e-6), "rounds_us": runs,
            "spread": (max(runs) - min(runs)) / us}


def converters(a, dev):
    res = {}
    st = torch.cuda.Stream(device=dev)
    g = np.random.default_rng(0)
    for H, W in SIZES:
        cases = {_name(l, d): rgb_case(l, d, H, W, dev, g, a.buffers) for l, d in FORMATS}
        cases["y410"] = y410_case(H, W, dev, g, a.buffers)
        runs = {name: {"to_planar": [], "from_planar": []} for name in cases}
        for _ in range(a.rounds):
            for name, (_, _, to, frm) in cases.items():
                runs[name]["to_planar"].append(graph_time_us(to, 64, a.replays, st)[0])
                runs[name]["from_planar"].append(graph_time_us(frm, 64, a.replays, st)[0])
        res["%dx%d" % (W, H)] = {name: {"to_planar": _stats(nb_to, runs[name]["to_planar"]), "from_planar": _stats(nb_from, runs[name]["from_planar"])}
                                 for name, (nb_to, nb_from, _, _) in cases.items()}
        del cases
        torch.cuda.empty_cache()
    return res


def alpha_passes(a, dev):
    res = {}
    st = torch.cuda.Stream(device=dev)
    g = np.random.default_rng(1)
    for H, W in SIZES:
        size = {}
        for layout, depth in ALPHA_FORMATS:
            cases = {policy: alpha_case(layout, depth, policy, H, W, dev, g, a.buffers) for policy in ("nearer", "blend")}
            runs = {policy: [] for policy in cases}
            for _ in range(a.rounds):
                for policy, (_, launch) in cases.items():
                    runs[policy].append(graph_time_us(launch, 64, a.replays, st)[0])
            size[_name(layout, depth)] = {policy: _stats(nb, runs[policy]) for policy, (nb, _) in cases.items()}
            del cases
            torch.cuda.empty_cache()
        res["%dx%d" % (W, H)] = size
    return res


def forwards(a, dev, nm):
    H, W = SIZES[0]
    nr = V.NativeRgb(nm)
    t = torch.tensor([0.5], device=dev)
    u8 = Hn.synthetic_pair(H, W, seed=0).numpy().reshape(1, 2, 3, H, W)
    u8_dev = torch.from_numpy(u8).to(dev)
    u10_dev = torch.from_numpy((u8.astype(np.uint16) << 2) | (u8 >> 6)).to(dev)
    f8, f10 = V.Format("bgra"), V.Format("x2rgb10")
    frames8 = [V.from_planar(u8_dev[0, i], f8) for i in range(2)]
    frames10 = [V.from_planar(u10_dev[0, i], f10) for i in range(2)]
    ws8, ws10, ws_m = nr.workspace(H, W), nr.workspace(H, W), nm.workspace(H, W)
    outs8, outs10 = [V.empty_frame(f8, H, W, dev)], [V.empty_frame(f10, H, W, dev)]
    steps = {"bgra": lambda: nr.forward(frames8, t, f8, f8, outs=outs8, ws=ws8),
             "x2rgb10": lambda: nr.forward(frames10, t, f10, f10, outs=outs10, ws=ws10),
             "model_u8": lambda: nm.interpolate_u10(u8_dev, t, out="u8", ws=ws_m),
             "model_u10": lambda: nm.interpolate_u10(u10_dev, t, ws=ws_m)}

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
            "conversion_overhead_ms_median": {k: statistics.median(x - y for x, y in zip(runs[k], runs[m]))
                                              for k, m in (("bgra", "model_u8"), ("x2rgb10", "model_u10"))}}


def checks(conv):
    out = {}
    for size in ("%dx%d" % (W, H) for H, W in SIZES):
        for d in ("to_planar", "from_planar"):
            y = conv[size]["y410"][d]["us"]
            for name in ("x2rgb10_10", "x2bgr10_10"):
                v = conv[size][name][d]["us"]
                out["%s_%s_%s_vs_y410" % (name, d, size)] = {"us": v, "y410_us": y, "ratio": v / y, "within_10_percent": v <= MARGIN * y}
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
    res = {"sizes": SIZES, "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "alternations": a.alternations,
           "rounds": a.rounds, "buffers": a.buffers, "replays": a.replays}
    res["converters"] = converters(a, dev)
    res["checks"] = checks(res["converters"])
    res["alpha"] = alpha_passes(a, dev)
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
