#!/usr/bin/env python3
"""The video API (libfldr_video.so) at 3840x2160 on bench.py's frame pairs (fldr_harness.synthetic_pair, seeds 0..), converted to NV12
by the oracle (tests/yuv_oracle.py, BT.709 limited):

  * ms per pair with 3 pairs in flight on 3 streams: fldr_video_forward NV12 -> NV12 against fldr_model_forward interleaved BGR -> BGR
    on the oracle's BGR frames of the same pairs, alternated in the same run (--alternations times each);
  * Session.push output frames/s at 1920x1080 and 3840x2160, n_t = 1 and 7 (host frames in and out: includes PCIe and host copies).

    python tools/bench_video.py [--steps 20] [--warmup 3] [--alternations 3] [--depth 8|10] [--out profiles/video_forward.json]

--depth 10: the same measurement on 10-bit frames — P010 -> P010 (the 8-bit pairs' texture quantised to 1023 levels, converted by
tests/yuv_hd_oracle.py) against fldr_model_forward planar uint16 BGR -> planar uint16 BGR (the model's 10-bit forms) on the oracle's BGR
words; sessions push P010.

Every frame of the timed loops is checked against the expected bytes before timing (the oracle's YUV of the model's output on the
oracle's BGR frames; for the BGR path, the model's planar output interleaved)."""
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
import fldr_video  # noqa: E402
import yuv_hd_oracle as HD  # noqa: E402
import yuv_oracle as O  # noqa: E402

MAT, RNG = "bt709", "limited"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--streams", type=int, default=3)
    ap.add_argument("--session-pushes", type=int, default=8)
    ap.add_argument("--depth", type=int, default=8, choices=[8, 10])
    ap.add_argument("--no-sessions", action="store_true", help="skip the Session.push measurement")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.depth == 10:
        return main10(a)
    dev = torch.device("cuda:0")
    nm = fldr_model.NativeModel.from_npz(Hn.DEFAULT_WEIGHTS, device=0)
    nv = fldr_video.NativeVideo(nm)
    H, W, NS = 2160, 3840, a.streams
    NP = max(NS + 1, 4)
    fmt = fldr_video.Format("nv12", MAT, RNG)
    yuv_dev, bgr_dev, want_yuv, want_bgr = [], [], [], []
    for p in range(NP):
        u8 = Hn.synthetic_pair(H, W, seed=p).numpy()
        yuv = [O.bgr_to_yuv420(u8[i], MAT, RNG) for i in range(2)]
        bgr = np.stack([O.yuv420_to_bgr(*yuv[i], MAT, RNG) for i in range(2)])                # what a caller converting on the host gets
        yuv_dev.append([tuple(torch.from_numpy(x).to(dev) for x in O.pack_nv12(*yuv[i])) for i in range(2)])
        bgr_dev.append([torch.from_numpy(np.ascontiguousarray(bgr[i].transpose(1, 2, 0))).to(dev) for i in range(2)])
        ref = nm.interpolate_u8(torch.from_numpy(bgr)[None].to(dev), [0.5])[0].cpu().numpy()  # planar [3,H,W]
        want_bgr.append(torch.from_numpy(np.ascontiguousarray(ref.transpose(1, 2, 0))).to(dev))
        y, u, v = O.bgr_to_yuv420(ref, MAT, RNG)
        want_yuv.append(tuple(torch.from_numpy(x).to(dev) for x in O.pack_nv12(y, u, v)))
    t = torch.tensor([0.5], device=dev)
    streams = [torch.cuda.Stream(device=dev) for _ in range(NS)]
    ws_v = [nv.workspace(H, W) for _ in range(NS)]
    ws_m = [nm.workspace(H, W) for _ in range(NS)]
    outs_v = [[fldr_video.empty_frame(fmt, H, W, dev)] for _ in range(NS)]

    def yuv_step(i):
        return nv.forward(yuv_dev[i % NP], t, fmt, fmt, outs=outs_v[i % NS], ws=ws_v[i % NS])[0]

    def bgr_step(i):
        return nm.interpolate_u8(pair=tuple(bgr_dev[i % NP]), t=t, order="bgr", out_layout="hwc", ws=ws_m[i % NS])[0]

    # the expected bytes, pair by pair and stream by stream
    for i in range(NP * NS):
        with torch.cuda.stream(streams[i % NS]):
            gy, gb = yuv_step(i), bgr_step(i)
        torch.cuda.synchronize()
        if not all(torch.equal(g, w) for g, w in zip(gy, want_yuv[i % NP])):
            raise SystemExit("YUV output of pair %d differs from the oracle's" % (i % NP))
        if not torch.equal(gb, want_bgr[i % NP]):
            raise SystemExit("BGR output of pair %d differs from the model's planar output" % (i % NP))
    res = {"size": [H, W], "streams": NS, "pairs": NP, "steps": a.steps, "warmup": a.warmup, "format": "nv12 %s %s" % (MAT, RNG),
           "device": torch.cuda.get_device_name(0)}

    def in_flight_ms_per_pair(step):
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

    runs = {"yuv_nv12": [], "bgr_interleaved": []}
    with torch.no_grad():
        for _ in range(a.alternations):
            runs["yuv_nv12"].append(in_flight_ms_per_pair(yuv_step))
            runs["bgr_interleaved"].append(in_flight_ms_per_pair(bgr_step))
    med = {k: statistics.median(v) for k, v in runs.items()}
    res["ms_per_pair_in_flight"] = {"runs": runs, "median": med}
    res["yuv_vs_bgr"] = med["yuv_nv12"] / med["bgr_interleaved"]
    res["targets"] = {"yuv_within_3pct_of_bgr": res["yuv_vs_bgr"] <= 1.03}

    # sessions: host frames in, host frames out
    sess = {}
    for (h, w) in (() if a.no_sessions else ((1080, 1920), (2160, 3840))):
        u8 = Hn.synthetic_pair(h + 4 * a.session_pushes, w + 6 * a.session_pushes, seed=7).numpy()[0]
        clip = [O.pack_nv12(*O.bgr_to_yuv420(np.ascontiguousarray(u8[:, 4 * k:4 * k + h, 6 * k:6 * k + w]), MAT, RNG))
                for k in range(a.session_pushes)]
        for n_t in (1, 7):
            s = fldr_video.Session(nm, h, w, n_t, fmt, fmt)
            s.push(clip[0])
            s.push(clip[1])                                                   # warm
            t0 = time.perf_counter()
            n_out = 0
            for k in range(2, a.session_pushes):
                n_out += len(s.push(clip[k]))
            dt = time.perf_counter() - t0
            s.close()
            sess["%dx%d_nt%d" % (w, h, n_t)] = {"output_frames_per_s": n_out / dt, "ms_per_push": dt * 1e3 / (a.session_pushes - 2)}
    res["session_push"] = sess
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    nm.close()


def pair10(H, W, seed):
    """fldr_harness.synthetic_pair's frames at ten bits: uint16 [2,3,H,W], code values 0 .. 1023."""
    base = Hn.texture(H + 64, W + 64, seed)
    q = lambda x: (x.clamp(0, 1) * 1023).round().to(torch.int32).numpy().astype(np.uint16)
    return np.stack([q(base[0, :, 32:H + 32, 32:W + 32]), q(base[0, :, 36:H + 36, 38:W + 38])])


def main10(a):
    dev = torch.device("cuda:0")
    nm = fldr_model.NativeModel.from_npz(Hn.DEFAULT_WEIGHTS, device=0)
    nv = fldr_video.NativeVideo(nm)
    H, W, NS = 2160, 3840, a.streams
    NP = max(NS + 1, 4)
    fmt = fldr_video.Format("nv12", MAT, RNG, 10)
    i32 = lambda x: x.cpu().to(torch.int32)
    yuv_dev, bgr_dev, want_yuv, want_bgr = [], [], [], []
    for p in range(NP):
        b10 = pair10(H, W, p)
        yuv = [HD.bgr_to_yuv420(b10[i], MAT, RNG, 10) for i in range(2)]
        bgr = np.stack([HD.yuv420_to_bgr(*yuv[i], MAT, RNG, 10) for i in range(2)])
        yuv_dev.append([tuple(torch.from_numpy(x).to(dev) for x in HD.pack_planes(*yuv[i], "nv12", 10)) for i in range(2)])
        bgr_dev.append(torch.from_numpy(bgr)[None].to(dev))
        ref = nm.interpolate_u10(bgr_dev[-1], [0.5])
        want_bgr.append(i32(ref))
        y, u, v = HD.bgr_to_yuv420(i32(ref)[0].numpy().astype(np.uint16), MAT, RNG, 10)
        want_yuv.append(tuple(torch.from_numpy(x.astype(np.int32)) for x in HD.pack_planes(y, u, v, "nv12", 10)))
    t = torch.tensor([0.5], device=dev)
    streams = [torch.cuda.Stream(device=dev) for _ in range(NS)]
    ws_v = [nv.workspace(H, W) for _ in range(NS)]
    ws_m = [nm.workspace(H, W) for _ in range(NS)]
    outs_v = [[fldr_video.empty_frame(fmt, H, W, dev)] for _ in range(NS)]

    def yuv_step(i):
        return nv.forward(yuv_dev[i % NP], t, fmt, fmt, outs=outs_v[i % NS], ws=ws_v[i % NS])[0]

    def bgr_step(i):
        return nm.interpolate_u10(bgr_dev[i % NP], t, ws=ws_m[i % NS])

    for i in range(NP * NS):
        with torch.cuda.stream(streams[i % NS]):
            gy, gb = yuv_step(i), bgr_step(i)
        torch.cuda.synchronize()
        if not all(torch.equal(i32(g), w) for g, w in zip(gy, want_yuv[i % NP])):
            raise SystemExit("P010 output of pair %d differs from the oracle's" % (i % NP))
        if not torch.equal(i32(gb), want_bgr[i % NP]):
            raise SystemExit("planar 10-bit output of pair %d differs" % (i % NP))
    res = {"size": [H, W], "streams": NS, "pairs": NP, "steps": a.steps, "warmup": a.warmup, "format": "p010 %s %s" % (MAT, RNG), "depth": 10,
           "device": torch.cuda.get_device_name(0)}

    def in_flight_ms_per_pair(step):
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

    runs = {"yuv_p010": [], "bgr_planar_u10": []}
    with torch.no_grad():
        for _ in range(a.alternations):
            runs["yuv_p010"].append(in_flight_ms_per_pair(yuv_step))
            runs["bgr_planar_u10"].append(in_flight_ms_per_pair(bgr_step))
    med = {k: statistics.median(v) for k, v in runs.items()}
    res["ms_per_pair_in_flight"] = {"runs": runs, "median": med}
    res["yuv_vs_bgr"] = med["yuv_p010"] / med["bgr_planar_u10"]
    sess = {}
    for (h, w) in (() if a.no_sessions else ((1080, 1920), (2160, 3840))):
        b10 = pair10(h + 4 * a.session_pushes, w + 6 * a.session_pushes, 7)[0]
        clip = [HD.pack_planes(*HD.bgr_to_yuv420(np.ascontiguousarray(b10[:, 4 * k:4 * k + h, 6 * k:6 * k + w]), MAT, RNG, 10), "nv12", 10)
                for k in range(a.session_pushes)]
        for n_t in (1, 7):
            s = fldr_video.Session(nm, h, w, n_t, fmt, fmt)
            s.push(clip[0])
            s.push(clip[1])
            t0 = time.perf_counter()
            n_out = 0
            for k in range(2, a.session_pushes):
                n_out += len(s.push(clip[k]))
            dt = time.perf_counter() - t0
            s.close()
            sess["%dx%d_nt%d" % (w, h, n_t)] = {"output_frames_per_s": n_out / dt, "ms_per_push": dt * 1e3 / (a.session_pushes - 2)}
    res["session_push"] = sess
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    nm.close()


if __name__ == "__main__":
    main()
