"""The RGB frame layouts and alpha rules of include/fldr_rgb.h in numpy, stated from the header's table (not from the kernels): what the
tests of libfldr_rgb.so compare with.  A frame is a tuple of 2-D arrays, one per plane:

    bgra, rgba, argb, abgr   one uint8 plane [H, 4 W]: four bytes per pixel in the named order
    x2rgb10                  one uint32 plane [H, W]: B bits 0-9, G 10-19, R 20-29, alpha 30-31
    x2bgr10                  one uint32 plane [H, W]: R bits 0-9, G 10-19, B 20-29, alpha 30-31
    gbrp, gbrap              three / four planes [H, W] in the order G, B, R(, A): uint8, or at depth 10 uint16 with the value in the low
                             10 bits

Colour values are code values: nothing is computed on them.  The three alpha rules are functions of the two inputs' alpha planes and the
time as a float32.
"""
import numpy as np

LAYOUTS = ("bgra", "rgba", "argb", "abgr", "x2rgb10", "x2bgr10", "gbrp", "gbrap")
BYTE_ORDER = {"bgra": "bgra", "rgba": "rgba", "argb": "argb", "abgr": "abgr"}         # the channel of byte i of a pixel
FIELDS = {"x2rgb10": {"b": 0, "g": 10, "r": 20, "a": 30}, "x2bgr10": {"r": 0, "g": 10, "b": 20, "a": 30}}      # the lowest bit of each field
PLANES = {"gbrp": "gbr", "gbrap": "gbra"}
# every valid (layout, depth)
FORMATS = [(l, 8) for l in ("bgra", "rgba", "argb", "abgr")] + [("x2rgb10", 10), ("x2bgr10", 10)] + [(l, d) for l in ("gbrp", "gbrap") for d in (8, 10)]
FFMPEG = {("bgra", 8): "bgra", ("rgba", 8): "rgba", ("argb", 8): "argb", ("abgr", 8): "abgr", ("x2rgb10", 10): "x2rgb10le",
          ("x2bgr10", 10): "x2bgr10le", ("gbrp", 8): "gbrp", ("gbrap", 8): "gbrap", ("gbrp", 10): "gbrp10le", ("gbrap", 10): "gbrap10le"}


def planes(layout):
    return len(PLANES[layout]) if layout in PLANES else 1


def row_bytes(layout, depth, W):
    """Bytes of a row of each plane."""
    return 4 * W if layout not in PLANES else W * (2 if depth == 10 else 1)


def sample_dtype(depth):
    """The type of a colour plane of the model's planar BGR frame."""
    return np.uint16 if depth == 10 else np.uint8


def alpha_bits(layout, depth):
    """The width of the layout's alpha: 8, 10, 2, or 0 where it has none."""
    if layout in BYTE_ORDER:
        return 8
    if layout in FIELDS:
        return 2
    return 0 if layout == "gbrp" else (10 if depth == 10 else 8)


def alpha_max(layout, depth):
    return (1 << alpha_bits(layout, depth)) - 1


def pack(layout, depth, b, g, r, a=None, dirt=None):
    """Planes b, g, r [H, W] (values below 2^depth) and alpha (None: opaque) -> the frame.  dirt: a numpy Generator that fills every bit a
    reader must ignore (bits 10-15 of a 16-bit planar word) with noise; the other layouts have no such bit (alpha is a value)."""
    b, g, r = (np.asarray(p) for p in (b, g, r))
    H, W = b.shape
    if a is None:
        a = np.full((H, W), alpha_max(layout, depth) if alpha_bits(layout, depth) else 0)
    ch = {"b": b, "g": g, "r": r, "a": np.asarray(a)}
    if layout in BYTE_ORDER:
        assert depth == 8
        out = np.empty((H, W, 4), np.uint8)
        for i, c in enumerate(BYTE_ORDER[layout]):
            assert ch[c].max(initial=0) <= 255
            out[:, :, i] = ch[c]
        return (out.reshape(H, 4 * W),)
    if layout in FIELDS:
        assert depth == 10
        w = np.zeros((H, W), np.uint32)
        for c, lo in FIELDS[layout].items():
            assert ch[c].max(initial=0) <= (3 if c == "a" else 1023)
            w |= ch[c].astype(np.uint32) << np.uint32(lo)
        return (w,)
    dt = sample_dtype(depth)
    out = []
    for c in PLANES[layout]:
        assert ch[c].max(initial=0) < (1 << depth)
        p = ch[c].astype(dt)
        if dirt is not None and depth == 10:
            p = p | (dirt.integers(0, 64, (H, W)).astype(np.uint16) << 10)
        out.append(np.ascontiguousarray(p))
    return tuple(out)


def unpack(layout, depth, frame):
    """The frame -> (b, g, r, a): planes [H, W] of sample_dtype(depth); a is None where the layout has no alpha (uint8 for the 2-bit
    field)."""
    ch = {"a": None}
    if layout in BYTE_ORDER:
        p = np.asarray(frame[0])
        px = p.reshape(p.shape[0], p.shape[1] // 4, 4)
        for i, c in enumerate(BYTE_ORDER[layout]):
            ch[c] = np.ascontiguousarray(px[:, :, i])
    elif layout in FIELDS:
        w = np.asarray(frame[0]).astype(np.uint32)
        for c, lo in FIELDS[layout].items():
            ch[c] = ((w >> np.uint32(lo)) & np.uint32(3 if c == "a" else 1023)).astype(np.uint8 if c == "a" else np.uint16)
    else:
        for c, p in zip(PLANES[layout], frame):
            ch[c] = np.asarray(p) & 0x3ff if depth == 10 else np.asarray(p)
    return ch["b"], ch["g"], ch["r"], ch["a"]


def planar_bgr(layout, depth, frame):
    """The model's planar frame [3, H, W] of a frame."""
    b, g, r, _ = unpack(layout, depth, frame)
    return np.stack([b, g, r]).astype(sample_dtype(depth))


# ---- alpha --------------------------------------------------------------------------------------------------------------------------
def alpha_opaque(layout, depth, H, W):
    return np.full((H, W), alpha_max(layout, depth), np.uint16)


def alpha_nearer(a0, a1, t):
    """The alpha of in[t < 0.5 ? 0 : 1], the comparison in float32 (a NaN fails it: in[1])."""
    return np.asarray(a0 if np.float32(t) < np.float32(0.5) else a1).copy()


def blend_weight(t):
    """w = t >= 0 ? min(rint(t * 65536), 65536) : 0 with t a float32 (a NaN fails the comparison)."""
    t = np.float32(t)
    if not t >= np.float32(0):
        return 0
    return int(min(np.rint(t * np.float32(65536.0)), np.float32(65536.0)))


def alpha_blend(a0, a1, t):
    """(a0 * (65536 - w) + a1 * w + 32768) >> 16 in uint32."""
    w = np.uint32(blend_weight(t))
    a0, a1 = np.asarray(a0).astype(np.uint32), np.asarray(a1).astype(np.uint32)
    return ((a0 * (np.uint32(65536) - w) + a1 * w + np.uint32(32768)) >> np.uint32(16)).astype(np.uint16)


def alpha_of(policy, a0, a1, t):
    """The alpha plane of an output under `policy`: None (pack's opaque) for "opaque", else the rule's."""
    if policy == "opaque":
        return None
    return alpha_nearer(a0, a1, t) if policy == "nearer" else alpha_blend(a0, a1, t)
