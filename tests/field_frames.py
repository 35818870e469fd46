"""Frames for the field API's tests: noise, flat and perturbed frames in the four containers (NV12, I420, P010, yuv420p10le) as tuples of
numpy planes, and woven sequences made of tests/rate_frames.py's pictures."""
import functools

import numpy as np

import field_oracle as F
import rate_frames as RF

FORMATS = [("nv12", 8), ("nv12", 10), ("i420", 8), ("i420", 10)]


def plane_shapes(layout, H, W):
    ch, cw = (H + 1) // 2, (W + 1) // 2
    return [(H, W), (ch, 2 * cw)] if layout == "nv12" else [(H, W), (ch, cw), (ch, cw)]


def pack(values, layout, depth, junk=None):
    """A plane of code values -> the container's samples; junk (0 .. 63 per sample): the bits a reader must ignore — the low six of a
    P010 word, the high six of a yuv420p10le word."""
    if depth != 10:
        return values.astype(np.uint8)
    v = values.astype(np.uint16)
    j = np.zeros_like(v) if junk is None else junk.astype(np.uint16)
    return (v << 6 | j) if layout == "nv12" else (v | j << 10)


def noise(rng, layout, depth, H, W, dirty=False):
    """One H x W frame of noise; depth 10 in the container's canonical form unless `dirty`."""
    planes = []
    for shape in plane_shapes(layout, H, W):
        v = rng.integers(0, F.mx(depth) + 1, shape)
        planes.append(pack(v, layout, depth, rng.integers(0, 64, shape) if dirty and depth == 10 else None))
    return tuple(planes)


def flat(layout, depth, H, W, code):
    return tuple(pack(np.full(shape, code), layout, depth) for shape in plane_shapes(layout, H, W))


def add(frame, layout, depth, p, y, x, delta):
    """A copy of `frame` with delta added to the code value of sample (y, x) of plane p (x in samples of the row, components interleaved)."""
    out = [q.copy() for q in frame]
    v = int(F.value(out[p][y:y + 1, x:x + 1], layout, depth)[0, 0]) + delta
    assert 0 <= v <= F.mx(depth)
    out[p][y, x] = pack(np.array([[v]]), layout, depth)[0, 0]
    return tuple(out)


@functools.lru_cache(maxsize=16)
def pictures(H, W, layout, depth, seed=3):
    """Two pictures of one moving scene (fldr_harness.synthetic_pair) in the container."""
    import fldr_harness as Hn
    u8 = Hn.synthetic_pair(H, W, seed=seed).numpy()
    return tuple(RF.planes_of_bgr(u8[i], layout, depth) for i in range(2))


def interlace(top_picture, bottom_picture, tff=True):
    """The woven frame whose first field comes from the first picture and whose second from the second."""
    first, second = (0, 1) if tff else (1, 0)
    out = []
    for a, b in zip(top_picture, bottom_picture):
        p = a.copy()
        p[first::2] = a[first::2]
        p[second::2] = b[second::2]
        out.append(p)
    return tuple(out)
