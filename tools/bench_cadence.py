#!/usr/bin/env python3
"""The cadence API (libfldr_cadence.so) at 3840x2160, NV12 and P010 (BT.709 limited), on a moving texture
(fldr_harness.synthetic_pair, as tools/bench_pipe.py's clip), in one process:

  * µs per fldr_repeat_measure beside µs per fldr_scene_measure on the same frame pairs — a moving pair, a repeat (the same frame with
    a code changed on eight samples) and a black pair —, each measure's three launches back to back on one stream, by device events,
    the two alternated --alternations times.  Both read the two luma planes once.
  * ms per CONTAINER frame of a cadence stream, 60p carrying 3:2 film (cycle 5, drop 3) -> 60 and -> 120, beside fldr_rate 24 -> 60 / 120
    pushed the survivors alone — the floor: the difference is the repeat measure plus the second upload of every frame —, alternated
    --alternations times, the C entry points called directly (host frames in and out: includes PCIe and host copies).  Both times are
    divided by the number of container frames.

    python tools/bench_cadence.py [--real 6] [--cycles 2] [--alternations 3] [--out profiles/cadence.json]

Before any timing every measure is compared with its oracle (tests/cadence_oracle.py, tests/scene_oracle.py) and the stream's frames
with the converter's on the survivors, byte for byte."""
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
import fldr_rate  # noqa: E402
import fldr_video  # noqa: E402
import scene_oracle as S  # noqa: E402
import yuv_hd_oracle as HD  # noqa: E402
import yuv_oracle as O  # noqa: E402

MAT, RNG = "bt709", "limited"
H, W = 2160, 3840
CYCLE, DROP, COUNTS = 5, 3, (3, 2)


def fmt_name(depth):
    return "nv12" if depth == 8 else "p010"


def make_clip(n, depth):
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


def perturbed(planes, depth, seed):
    """The frame with one code of y8 added to (or taken from) eight luma samples."""
    g = np.random.default_rng(seed)
    y = planes[0].copy()
    step = 1 if depth == 8 else 1 << 8
    for _ in range(8):
        r, c = int(g.integers(0, H)), int(g.integers(0, W))
        y[r, c] = y[r, c] + step if S.y8(y[r:r + 1, c:c + 1], "nv12", depth)[0, 0] < 128 else y[r, c] - step
    return (y,) + tuple(planes[1:])


def telecine(real, depth):
    """Every real frame shown 3, 2, 3, 2 ... times, the repeats perturbed -> (container frames, the numbers of the first instances)."""
    frames, firsts = [], []
    for k, f in enumerate(real):
        firsts.append(len(frames))
        frames.append(f)
        for i in range(1, COUNTS[k % 2]):
            frames.append(perturbed(f, depth, 100 * k + i))
    return frames, firsts


def to_dev(planes, dev):
    return tuple(torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in planes)


def black(depth):
    dt, y, c = (np.uint8, 16, 128) if depth == 8 else (np.uint16, 64 << 6, 512 << 6)
    return (np.full((H, W), y, dt), np.full(((H + 1) // 2, 2 * ((W + 1) // 2)), c, dt))


def measures_alone(a, dev, real, depth, res):
    fmt = fldr_video.Format("nv12", MAT, RNG, depth)
    pairs = {"moving": (real[0], real[1]), "repeat": (real[0], perturbed(real[0], depth, 1)), "black": (black(depth), black(depth))}
    out = {}
    for kind, pr in pairs.items():
        frames = [to_dev(f, dev) for f in pr]
        rs, ss = fldr_cadence.repeat_state(dev), fldr_rate.scene_state(dev)
        got = fldr_cadence.repeat_measure(frames, fmt, state=rs)
        if got != dict(C.measure(pr[0], pr[1], ("nv12", depth)), reserved=[0, 0]):
            raise SystemExit("the repeat measure of the %s pair differs from the oracle's: %r" % (kind, got))
        if fldr_rate.scene_measure(frames, fmt, state=ss) != S.measure(pr[0], pr[1], fmt):
            raise SystemExit("the scene measure of the %s pair differs from the oracle's" % kind)
        calls = {"repeat_measure": lambda: fldr_cadence.repeat_measure(frames, fmt, state=rs, read=False),
                 "scene_measure": lambda: fldr_rate.scene_measure(frames, fmt, state=ss, read=False)}
        runs = {k: [] for k in calls}
        for _ in range(a.alternations):
            for name, call in calls.items():
                for _ in range(5):
                    call()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.measures):
                    call()
                e1.record()
                torch.cuda.synchronize()
                runs[name].append(e0.elapsed_time(e1) * 1e3 / a.measures)
        med = {k: statistics.median(v) for k, v in runs.items()}
        out[kind] = {"us_per_measure": med, "runs": runs, "repeat_over_scene": med["repeat_measure"] / med["scene_measure"], "result": got}
        print("%s %s: repeat measure %.1f us, scene measure %.1f us" % (fmt_name(depth), kind, med["repeat_measure"], med["scene_measure"]), flush=True)
    res["measure_alone"][fmt_name(depth)] = out


def end_to_end(a, nm, real, depth, res):
    fmt = fldr_video.Format("nv12", MAT, RNG, depth)
    frames, firsts = telecine(real, depth)
    frames = frames[:len(frames) // CYCLE * CYCLE]
    firsts = [n for n in firsts if n < len(frames)]
    ms = [None] + [C.measure(frames[n - 1], frames[n], ("nv12", depth)) for n in range(1, len(frames))]
    kept, _ = C.survivors(ms, CYCLE, DROP)
    if kept != firsts:
        raise SystemExit("the oracle keeps %r, the first instances are %r" % (kept, firsts))
    out = {}
    for out_rate in (60, 120):
        cad = fldr_cadence.Cadence(nm, H, W, fmt, 60, out_rate, CYCLE, DROP, scene=True)
        conv = fldr_rate.Converter(nm, H, W, fmt, 24, out_rate, scene=True)
        got = [o for f in frames for o in cad.push(f)] + cad.flush()
        want = [o for n in kept for o in conv.push(frames[n])] + conv.flush()
        if len(got) != len(want) or not all(np.array_equal(x, y) for fa, fb in zip(got, want) for x, y in zip(fa, fb)):
            raise SystemExit("60 (5, 3) -> %d: the stream's frames differ from the converter's on the survivors" % out_rate)
        structs = [fldr_video.frame_struct(f) for f in frames]
        cad_outs, conv_outs = cad._out_structs(), conv._out_structs()
        LC, LR = fldr_cadence.lib(), fldr_rate.lib()
        n = ctypes.c_int(0)

        def run_cadence():
            LC.fldr_cadence_reset(cad._h)
            total = 0
            t0 = time.perf_counter()
            for _ in range(a.cycles):
                for fr in structs:
                    rc = LC.fldr_cadence_push(cad._h, ctypes.byref(fr), cad_outs, ctypes.byref(n), None)
                    if rc:
                        raise SystemExit("fldr_cadence_push: %d" % rc)
                    total += n.value
            return time.perf_counter() - t0, total

        def run_floor():
            LR.fldr_rate_reset(conv._h)
            total = 0
            t0 = time.perf_counter()
            for _ in range(a.cycles):
                for k in kept:
                    rc = LR.fldr_rate_push(conv._h, ctypes.byref(structs[k]), conv_outs, ctypes.byref(n), None)
                    if rc:
                        raise SystemExit("fldr_rate_push: %d" % rc)
                    total += n.value
            return time.perf_counter() - t0, total
        container = len(structs) * a.cycles
        runs = {"cadence": [], "rate_on_survivors": []}
        for alt in range(a.alternations + 1):                            # pass 0 warms both objects
            for name, run in (("cadence", run_cadence), ("rate_on_survivors", run_floor)):
                dt, n_out = run()
                if alt:
                    runs[name].append({"ms_per_container_frame": dt * 1e3 / container, "output_frames_per_s": n_out / dt, "outputs": n_out})
        cad.close()
        conv.close()
        med = {k: statistics.median(r["ms_per_container_frame"] for r in v) for k, v in runs.items()}
        out["60_to_%d" % out_rate] = {"container_frames": container, "survivors": len(kept) * a.cycles, "ms_per_container_frame": med,
                                      "cost_ms_per_container_frame": med["cadence"] - med["rate_on_survivors"],
                                      "cadence_over_floor": med["cadence"] / med["rate_on_survivors"], "runs": runs}
        print("%s 60 (5, 3) -> %d: cadence %.2f ms per container frame, fldr_rate 24 -> %d on the survivors %.2f" % (
            fmt_name(depth), out_rate, med["cadence"], out_rate, med["rate_on_survivors"]), flush=True)
    res["end_to_end"][fmt_name(depth)] = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--real", type=int, default=6, help="real frames of the clip (3:2: five container frames per two)")
    ap.add_argument("--cycles", type=int, default=2, help="times the container clip is pushed in one timed run")
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--measures", type=int, default=50, help="measures per timed loop")
    ap.add_argument("--depths", default="8,10", help="8: NV12, 10: P010")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    nm = fldr_model.NativeModel.from_npz(Hn.DEFAULT_WEIGHTS, device=0)
    res = {"size": [H, W], "device": torch.cuda.get_device_name(0), "cycle": CYCLE, "drop": DROP, "alternations": a.alternations,
           "measure_alone": {}, "end_to_end": {}}
    for depth in [int(v) for v in a.depths.split(",")]:
        real = make_clip(a.real, depth)
        measures_alone(a, dev, real, depth, res)
        end_to_end(a, nm, real, depth, res)
        if a.out:                                                        # written after every format: a cut-off run keeps what it measured
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: v for k, v in res.items() if k not in ("measure_alone", "end_to_end")}))
    nm.close()


if __name__ == "__main__":
    main()
