"""Interlaced container streams for the pulldown API's tests: the film of tests/cadence_frames.py (a moving clip with a cut in it; imported,
not changed) woven field by field into 3:2 pulldown top-field-first and bottom-field-first, into 2:2 with the fields one frame out of
phase, and into plain progressive frames with four frames of true video among them.  Shared by tests/test_pulldown_cpu.py, which asserts
on the CPU that the oracle's survivors of every stream are its film frames, and tests/test_gpu_pulldown.py, which relies on it.

Every stream is (frames, film, spec): the container frames, the film frames the survivors must equal, in order, and the declaration
{"cycle", "drop", "anchor", "in_rate", "out_rate"}.  Frames are shared: never written."""
import functools

import numpy as np

import cadence_frames as CF
import cadence_oracle as CO
import rate_frames as RF

H, W = CF.H, CF.W                                 # 256 x 448
FORMATS = [("nv12", 8), ("i420", 10)]             # NV12 and yuv420p10le
N_FILM = 8                                        # film frames of the 3:2 streams: two cycles of five container frames
N_VIDEO = 4
STREAMS = ("3:2 tff", "3:2 bff", "2:2 shifted", "video insert", "3:2 tff perturbed")


def weave(top, bottom):
    """The frame whose even rows, in every plane, are `top`'s and whose odd rows are `bottom`'s."""
    out = []
    for t, b in zip(top, bottom):
        o = t.copy()
        o[1::2] = b[1::2]
        out.append(o)
    return tuple(out)


def perturbed_field(planes, layout, depth, parity, seed):
    """A copy of a frame with 1 .. 8 luma samples of the rows y % 2 == parity moved by one code of y8, as cadence_frames.perturbed moves them."""
    g = np.random.default_rng(seed)
    y = planes[0].copy()
    step = 1 if depth == 8 else (1 << 8 if layout == "nv12" else 1 << 2)
    for _ in range(int(g.integers(1, 9))):
        r, c = 2 * int(g.integers(0, y.shape[0] // 2)) + parity, int(g.integers(0, y.shape[1]))
        dark = CO.S.y8(y[r:r + 1, c:c + 1], layout, depth)[0, 0] < 128
        y[r, c] = y[r, c] + step if dark else y[r, c] - step
    return (y,) + tuple(planes[1:])


def telecine32(film, first_parity):
    """3:2 pulldown: film frame k lasts 2, 3, 2, 3, .. fields; the fields alternate in parity from first_parity (0: top field first);
    container frame n weaves fields 2 n and 2 n + 1.  -> (frames, [(film frame of the top field, film frame of the bottom field)])."""
    fields = [k for k in range(len(film)) for _ in range(2 + k % 2)]
    frames, source = [], []
    for n in range(len(fields) // 2):
        a, b = fields[2 * n], fields[2 * n + 1]
        t, bt = (a, b) if first_parity == 0 else (b, a)
        frames.append(weave(film[t], film[bt]))
        source.append((t, bt))
    return frames, source


@functools.lru_cache(maxsize=None)
def video_frames(layout, depth):
    """N_VIDEO frames of true video: the two fields of each come from different instants of a clip of its own."""
    clip = [RF.planes_of_bgr(f, layout, depth) for f in CF._clip(2 * N_VIDEO, seed=23)]
    return [weave(clip[2 * k], clip[2 * k + 1]) for k in range(N_VIDEO)]


def _freeze(frames):
    for f in frames:
        for p in f:
            p.flags.writeable = False
    return frames


@functools.lru_cache(maxsize=None)
def stream(name, layout, depth):
    real = CF.real_frames(layout, depth)
    if name.startswith("3:2"):
        film = real[:N_FILM]
        frames, source = telecine32(film, 1 if "bff" in name else 0)
        if name.endswith("perturbed"):
            # the second instance of every repeated field (the top field of frames 2, 7, the bottom field of frames 4, 9 in tff)
            seen = set()
            for n, (t, b) in enumerate(source):
                order = ((0, t), (1, b))
                for parity, k in order:
                    if (parity, k) in seen:
                        frames[n] = perturbed_field(frames[n], layout, depth, parity, seed=100 * n + parity)
                    seen.add((parity, k))
        spec = {"cycle": 5, "drop": 1, "anchor": 0, "in_rate": 30, "out_rate": 60}
    elif name == "2:2 shifted":
        # 25 fps film in 50i, the bottom field one frame late: frame n = top of G[n], bottom of G[n - 1].  The stream begins on a whole
        # frame and the film holds its last frame for two, so that no field at either end of the stream is an orphan.
        film = real[:6] + [real[5]]
        frames = [weave(film[n], film[max(n - 1, 0)]) for n in range(len(film))]
        spec = {"cycle": 1, "drop": 0, "anchor": 0, "in_rate": 25, "out_rate": 50}
    elif name == "video insert":
        film = real[:3] + video_frames(layout, depth) + real[3:6]
        frames = [tuple(p.copy() for p in f) for f in film]
        spec = {"cycle": 1, "drop": 0, "anchor": 0, "in_rate": 30, "out_rate": 60}
    else:
        raise KeyError(name)
    return _freeze(list(frames)), film, spec


def progressive(layout, depth, n=6):
    """Plain progressive frames in an interlaced container: the film itself."""
    return CF.real_frames(layout, depth)[:n]
