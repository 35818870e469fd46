"""Streams for the probe API's tests: the film streams of tests/pulldown_frames.py and the repeat patterns of tests/cadence_frames.py
(imported, not changed), plus true interlaced video, top and bottom field first, woven from the instants of a moving clip
(cadence_frames._clip), and a still stream.  Shared by tests/test_probe_cpu.py, which asserts on the CPU that the oracle's verdict on
every stream is the expected one, and tests/test_gpu_probe.py, which relies on it.

Every stream is (frames, expected): the container frames and the expected verdict words.  Frames are shared: never written."""
import functools

import cadence_frames as CF
import probe_oracle as O
import pulldown_frames as PF
import rate_frames as RF

H, W = CF.H, CF.W                                 # 256 x 448
FORMATS = [("nv12", 8), ("i420", 10)]             # NV12 and yuv420p10le
N_VIDEO = 8                                       # frames of the video streams: 16 instants
N_CADENCE = 14                                    # container frames of the repeat patterns: 12 measured, two cycles of five and more

# name -> expected verdict words (kind always; the others where the kind defines them)
EXPECTED = {
    "3:2 tff": dict(kind=O.FILM, cycle=5, drop=1),
    "3:2 bff": dict(kind=O.FILM, cycle=5, drop=1),
    "3:2 tff perturbed": dict(kind=O.FILM, cycle=5, drop=1),
    "2:2 shifted": dict(kind=O.FILM, cycle=1, drop=0),
    "progressive": dict(kind=O.PROGRESSIVE, cycle=1, drop=0),
    "repeats 3:2": dict(kind=O.PROGRESSIVE, cycle=5, drop=3),
    "repeats 2:2": dict(kind=O.PROGRESSIVE, cycle=2, drop=1),
    "repeats 4+1": dict(kind=O.PROGRESSIVE, cycle=5, drop=1),
    "video tff": dict(kind=O.INTERLACED, tff=1, mixed=0),
    "video bff": dict(kind=O.INTERLACED, tff=0, mixed=0),
    "video insert": dict(kind=O.INTERLACED, tff=1, mixed=1),
    "still": dict(kind=O.UNKNOWN),
}
STREAMS = tuple(EXPECTED)


@functools.lru_cache(maxsize=None)
def video(layout, depth, tff, n=N_VIDEO, seed=31):
    """n frames of true video: frame k weaves the instants 2 k and 2 k + 1 of a moving clip, the earlier one into the top field when
    tff, into the bottom field otherwise."""
    clip = [RF.planes_of_bgr(f, layout, depth) for f in CF._clip(2 * n, seed=seed)]
    return [PF.weave(clip[2 * k], clip[2 * k + 1]) if tff else PF.weave(clip[2 * k + 1], clip[2 * k]) for k in range(n)]


@functools.lru_cache(maxsize=None)
def stream(name, layout, depth):
    if name in PF.STREAMS:
        frames = PF.stream(name, layout, depth)[0]
    elif name == "progressive":
        frames = PF.progressive(layout, depth, 8)
    elif name.startswith("repeats "):
        frames = CF.stream(name.split()[1], layout, depth, N_CADENCE)[0]
    elif name.startswith("video "):
        frames = video(layout, depth, name.endswith("tff"))
    elif name == "still":
        frames = [CF.real_frames(layout, depth)[0]] * 8
    else:
        raise KeyError(name)
    return PF._freeze(list(frames)), EXPECTED[name]
