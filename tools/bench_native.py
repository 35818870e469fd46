#!/usr/bin/env python3
"""The C model API (libfldr_model.so) against the Python forward, in one process at 3840x2160 (bench.py's frame size and pairs):

  * host us per forward call: wall time of the enqueue alone (no synchronisation inside the timed calls), native vs Python eager;
  * single-stream latency: one forward then a synchronisation, median ms — native, Python eager, Python graph replay;
  * ms per pair with 3 pairs in flight on 3 streams: native eager, Python eager, Python graph replay (fldr_harness.GraphedInterpolator).

    python tools/bench_native.py [--steps 30] [--warmup 5] [--out profiles/native_forward.json]

Every native frame of the timed loops is checked against the Python frame of the same pair before timing (the same bits)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fldr-vfi_amd"))

import torch  # noqa: E402

import fldr_harness as Hn  # noqa: E402
import fldr_model  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--streams", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    model, _, args = Hn.prepare_model(dev)
    nm = fldr_model.NativeModel.from_module(model)
    H, W, NS = a.height, a.width, a.streams
    NP = max(NS + 1, 4)
    with torch.no_grad():
        frames = [Hn.frames_from_uint8(Hn.synthetic_pair(H, W, seed=p)).to(dev) for p in range(NP)]
        pyrs = [Hn.build_pyramid(Hn.pad_frames(f, args), args) for f in frames]
    t_py = torch.tensor([[0.5]], device=dev)
    t_nat = torch.tensor([0.5], device=dev)
    streams = [torch.cuda.Stream(device=dev) for _ in range(NS)]
    wss = [nm.workspace(H, W) for _ in range(NS)]
    outs = [torch.empty(1, 3, *pyrs[0][0].shape[3:], dtype=torch.float64, device=dev) for _ in range(NS)]

    def native(k, s_i):
        return nm.forward_pyramid(pyrs[k], t_nat, H, W, ws=wss[s_i], out=outs[s_i])

    def python(k):
        return Hn.interpolate(model, args, frames[k], t_py, pyramid=pyrs[k])

    # the same bits, pair by pair
    with torch.no_grad():
        for k in range(NP):
            ref = python(k)
            got = native(k, 0)[:, :, :H, :W]
            torch.cuda.synchronize()
            if not torch.equal(ref, got):
                raise SystemExit("native frame of pair %d differs from the Python frame" % k)
    res = {"size": [H, W], "streams": NS, "pairs": NP, "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}

    # host time per call: enqueue only (the queue is drained between groups of calls so that a full queue cannot block the host)
    def host_us(fn, reps):
        v = []
        with torch.no_grad():
            for r in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(r % NP)
                v.append((time.perf_counter() - t0) * 1e6)
        torch.cuda.synchronize()
        return statistics.median(v[a.warmup:])
    res["host_us_per_forward"] = {"native": host_us(lambda k: native(k, 0), a.steps + a.warmup),
                                  "python_eager": host_us(python, a.steps + a.warmup)}

    # single-stream latency
    def latency_ms(fn, reps):
        v = []
        with torch.no_grad():
            for r in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(r % NP)
                torch.cuda.synchronize()
                v.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(v[a.warmup:])
    pools = [torch.cuda.graph_pool_handle() for _ in range(NS)]
    graphs = {(s, k): Hn.GraphedInterpolator(model, args, frames[k], t_py, pyramid=pyrs[k], stream=streams[s], pool=pools[s], check=True)
              for s in range(NS) for k in range(NP)}
    torch.cuda.synchronize()
    res["latency_ms"] = {"native": latency_ms(lambda k: native(k, 0), a.steps + a.warmup),
                         "python_eager": latency_ms(python, a.steps + a.warmup),
                         "python_graph": latency_ms(lambda k: graphs[(0, k)].replay(), a.steps + a.warmup)}

    # NS pairs in flight on NS streams
    def in_flight_ms_per_pair(step):
        with torch.no_grad():
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

    res["ms_per_pair_in_flight"] = {
        "native_eager": in_flight_ms_per_pair(lambda i: native(i % NP, i % NS)),
        "python_eager": in_flight_ms_per_pair(lambda i: python(i % NP)),
        "python_graph": in_flight_ms_per_pair(lambda i: graphs[(i % NS, i % NP)].replay()),
    }
    r = res["ms_per_pair_in_flight"]
    res["native_eager_vs_python_graph"] = r["native_eager"] / r["python_graph"]
    res["targets"] = {"native_host_us_le_300": res["host_us_per_forward"]["native"] <= 300.0,
                      "native_eager_within_3pct_of_python_graph": res["native_eager_vs_python_graph"] <= 1.03}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    nm.close()


if __name__ == "__main__":
    main()
