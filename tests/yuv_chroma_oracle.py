"""numpy oracle of the colour definition of libfldr_chroma.so: YUV 4:2:2 and 4:4:4 <-> planar BGR in the integer fixed point of
libfldr_video.so (tests/yuv_hd_oracle.py: the same constants(), 16 fraction bits and offsets), at depth 8 or 10.  Every expression is the
kernels' own, in int64.

4:2:2: chroma is co-sited with the even luma columns ("left") and has no vertical taps; mid = 128 << (depth - 8).
    to BGR      h = C[y, ca(x)] + C[y, cb(x)] with the 4:2:0 oracle's ca, cb; cu = 4 h - 8 mid; then the 4:2:0 expressions (yv, >> 19, clamp)
    from BGR    p = K?R R + K?G G + K?B B; s = 2 (p[y, c0] + 2 p[y, c1] + p[y, c2]) with the 4:2:0 oracle's clamped c0, c1, c2;
                C = clamp(((s + 2^18) >> 19) + mid); Y as at 4:2:0
4:4:4: yuv444_to_rgb / rgb_to_yuv444 of tests/yuv_hd_oracle.py, unchanged.

Planes are numpy arrays of code values (uint8 at depth 8, uint16 at depth 10): Y [H,W]; U, V [H, ceil(W/2)] at 4:2:2, [H,W] at 4:4:4; BGR
frames are planar [3,H,W].  Containers (pack / unpack): "planar" (Y, U, V; depth 10: the value in the low 10 bits), "semiplanar" (Y, UV
interleaved; depth 10: the value in the high 10 bits), "uyvy" / "yuyv" (one plane of 4-byte groups, 4:2:2 at depth 8)."""
import numpy as np

from yuv_hd_oracle import MATRICES, RANGES, _clamp, constants, dtype_of, rgb_to_yuv444, yuv444_to_rgb  # noqa: F401

SAMPLINGS = ("422", "444")
LAYOUTS = ("planar", "semiplanar", "uyvy", "yuyv")


def chroma_width(sampling, W):
    return W if sampling == "444" else (W + 1) // 2


def yuv_to_bgr(Y, U, V, sampling, matrix, rng, depth=8):
    """YUV planes of code values -> planar BGR [3,H,W]."""
    H, W = Y.shape
    assert U.shape == (H, chroma_width(sampling, W)) and V.shape == U.shape
    if sampling == "444":
        R, G, B = yuv444_to_rgb(Y, U, V, matrix, rng, depth)
        return np.stack([B, G, R]).astype(dtype_of(depth))
    k = constants(matrix, rng, depth)
    mid = 128 << (depth - 8)
    cw = U.shape[1]
    x = np.arange(W)
    ca = np.where(x % 2 == 0, x // 2, (x - 1) // 2)
    cb = np.minimum(np.where(x % 2 == 0, x // 2, (x + 1) // 2), cw - 1)

    def up(P):
        P = P.astype(np.int64)
        return 4 * (P[:, ca] + P[:, cb]) - 8 * mid
    cu, cv = up(U), up(V)
    yv = (Y.astype(np.int64) - k["YOFF"]) * 8 * k["KY"]
    R = (yv + k["KRV"] * cv + (1 << 18)) >> 19
    G = (yv - k["KGU"] * cu - k["KGV"] * cv + (1 << 18)) >> 19
    B = (yv + k["KBU"] * cu + (1 << 18)) >> 19
    return np.stack([_clamp(B, depth), _clamp(G, depth), _clamp(R, depth)])


def bgr_to_yuv(bgr, sampling, matrix, rng, depth=8):
    """Planar BGR [3,H,W] code values -> (Y, U, V)."""
    if sampling == "444":
        Y, U, V = rgb_to_yuv444(bgr[2], bgr[1], bgr[0], matrix, rng, depth)
        return tuple(np.ascontiguousarray(p.astype(dtype_of(depth))) for p in (Y, U, V))
    k = constants(matrix, rng, depth)
    mid = 128 << (depth - 8)
    B, G, R = (bgr[c].astype(np.int64) for c in range(3))
    H, W = B.shape
    cw = (W + 1) // 2
    Y = ((k["KYR"] * R + k["KYG"] * G + k["KYB"] * B + (1 << 15)) >> 16) + k["YOFF"]
    i = np.arange(cw)
    c0, c1, c2 = np.clip(2 * i - 1, 0, W - 1), 2 * i, np.minimum(2 * i + 1, W - 1)

    def down(kr_, kg_, kb_):
        p = kr_ * R + kg_ * G + kb_ * B
        s = 2 * (p[:, c0] + 2 * p[:, c1] + p[:, c2])
        return np.ascontiguousarray(_clamp(((s + (1 << 18)) >> 19) + mid, depth))
    return _clamp(Y, depth), down(k["KUR"], k["KUG"], k["KUB"]), down(k["KVR"], k["KVG"], k["KVB"])


# ---- containers -------------------------------------------------------------------------------------------------------------------
def pack(Y, U, V, sampling, layout, depth=8, dirt=None):
    """Code-value planes -> the planes of the container.  dirt: a numpy Generator that fills the bits the container does not use (the six
    spare bits of a 16-bit word; with odd W the second luma byte of the last uyvy / yuyv group) with random bits: readers ignore them.
    Without dirt those bits are zero, except that second luma byte, which is a copy of the last luma sample (what a writer produces)."""
    H, W = Y.shape
    if layout in ("uyvy", "yuyv"):
        assert sampling == "422" and depth == 8
        half = (W + 1) // 2
        Y2 = np.empty((H, 2 * half), np.uint8)
        Y2[:, :W] = Y
        if W % 2:
            Y2[:, W] = dirt.integers(0, 256, H).astype(np.uint8) if dirt is not None else Y[:, W - 1]
        out = np.empty((H, 4 * half), np.uint8)
        yo, uo = (1, 0) if layout == "uyvy" else (0, 1)
        out[:, yo::4], out[:, yo + 2::4], out[:, uo::4], out[:, uo + 2::4] = Y2[:, 0::2], Y2[:, 1::2], U, V
        return (out,)
    if layout == "semiplanar":
        uv = np.empty((H, 2 * U.shape[1]), U.dtype)
        uv[:, 0::2], uv[:, 1::2] = U, V
        planes = [Y, uv]
    else:
        planes = [Y, U, V]
    if depth == 8:
        return tuple(np.ascontiguousarray(p) for p in planes)
    out = []
    for p in planes:
        w = p.astype(np.uint16)
        if layout == "semiplanar":
            w = w << 6
            if dirt is not None:
                w = w | dirt.integers(0, 64, w.shape).astype(np.uint16)
        elif dirt is not None:
            w = w | (dirt.integers(0, 64, w.shape).astype(np.uint16) << 10)
        out.append(np.ascontiguousarray(w))
    return tuple(out)


def unpack(planes, sampling, layout, W, depth=8):
    """The inverse: container planes -> (Y, U, V) code values (W: the luma width, which a packed plane does not tell when odd)."""
    if layout in ("uyvy", "yuyv"):
        p = planes[0]
        yo, uo = (1, 0) if layout == "uyvy" else (0, 1)
        Y2 = np.empty((p.shape[0], p.shape[1] // 2), np.uint8)
        Y2[:, 0::2], Y2[:, 1::2] = p[:, yo::4], p[:, yo + 2::4]
        return np.ascontiguousarray(Y2[:, :W]), np.ascontiguousarray(p[:, uo::4]), np.ascontiguousarray(p[:, uo + 2::4])
    if depth == 10:
        planes = [(p >> 6) if layout == "semiplanar" else (p & 0x3ff) for p in planes]
    if layout == "semiplanar":
        return planes[0], np.ascontiguousarray(planes[1][:, 0::2]), np.ascontiguousarray(planes[1][:, 1::2])
    return tuple(planes)


def containers():
    """Every (sampling, layout, depth) the library takes."""
    out = [(s, l, d) for s in SAMPLINGS for l in ("planar", "semiplanar") for d in (8, 10)]
    return out + [("422", "uyvy", 8), ("422", "yuyv", 8)]
