"""numpy oracle of the colour definition of libfldr_video.so with a `depth` argument (8 or 10): YUV 4:2:0 <-> BGR in integer fixed point,
BT.601 / BT.709, limited / full range, chroma sited "left".  At depth 8 it is tests/yuv_oracle.py byte for byte (tested); at depth d

    sy = 219 * 2^(d-8) / (2^d - 1), sc = 224 * 2^(d-8) / (2^d - 1)   (limited: Y 64..940, C 64..960 at d = 10; full: 1, 1)
    yoff = 16 << (d-8), chroma centre 128 << (d-8), clamps to 0 .. 2^d - 1

with the same Kr / Kb, 16 fraction bits, siting and tap weights.  Every expression is the kernels' own, in int64.

Planes are numpy arrays of code values (uint8 at depth 8, uint16 at depth 10): Y [H,W], U and V [ceil(H/2), ceil(W/2)]; BGR frames are
planar [3,H,W].  The two 10-bit containers: P010 (FLDR_VIDEO_NV12 at depth 10) keeps the value in the high 10 bits of each little-endian
word, yuv420p10le (FLDR_VIDEO_I420) in the low 10 bits."""
import numpy as np

MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
RANGES = ("limited", "full")
NAMES = ["KYR", "KYG", "KYB", "KUR", "KUG", "KUB", "KVR", "KVG", "KVB", "KY", "KRV", "KBU", "KGU", "KGV", "YOFF"]


def dtype_of(depth):
    return np.uint8 if depth == 8 else np.uint16


def scales(rng, depth):
    if rng != "limited":
        return 1.0, 1.0
    m = float((1 << depth) - 1)
    return 219.0 * (1 << (depth - 8)) / m, 224.0 * (1 << (depth - 8)) / m


def constants(matrix, rng, depth=8):
    """The integer table, derived from Kr and Kb: each coefficient round(c * 2^16)."""
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    sy, sc = scales(rng, depth)
    r = lambda v: int(np.floor(v * 65536.0 + 0.5))
    kyr, kyb = r(kr * sy), r(kb * sy)
    kyg = r(sy) - kyr - kyb
    kub = r(sc * 0.5)
    kur = r(-sc * 0.5 * kr / (1.0 - kb))
    kug = -kub - kur
    kvr = r(sc * 0.5)
    kvb = r(-sc * 0.5 * kb / (1.0 - kr))
    kvg = -kvr - kvb
    return dict(KYR=kyr, KYG=kyg, KYB=kyb, KUR=kur, KUG=kug, KUB=kub, KVR=kvr, KVG=kvg, KVB=kvb,
                KY=r(1.0 / sy), KRV=r(2.0 * (1.0 - kr) / sc), KBU=r(2.0 * (1.0 - kb) / sc),
                KGU=r(2.0 * (1.0 - kb) * kb / kg / sc), KGV=r(2.0 * (1.0 - kr) * kr / kg / sc),
                YOFF=(16 << (depth - 8)) if rng == "limited" else 0)


def _clamp(a, depth):
    return np.clip(a, 0, (1 << depth) - 1).astype(dtype_of(depth))


def chroma_size(H, W):
    return (H + 1) // 2, (W + 1) // 2


def yuv420_to_bgr(Y, U, V, matrix, rng, depth=8):
    """YUV 4:2:0 planes of code values -> planar BGR [3,H,W]."""
    k = constants(matrix, rng, depth)
    mid = 128 << (depth - 8)
    H, W = Y.shape
    ch, cw = chroma_size(H, W)
    assert U.shape == (ch, cw) and V.shape == (ch, cw)
    x = np.arange(W)
    ca = np.where(x % 2 == 0, x // 2, (x - 1) // 2)
    cb = np.minimum(np.where(x % 2 == 0, x // 2, (x + 1) // 2), cw - 1)
    y = np.arange(H)
    ra = np.clip(np.where(y % 2 == 0, y // 2 - 1, (y - 1) // 2), 0, ch - 1)
    rb = np.clip(np.where(y % 2 == 0, y // 2, (y + 1) // 2), 0, ch - 1)
    wa = np.where(y % 2 == 0, 1, 3)[:, None]
    wb = 4 - wa

    def up(P):
        P = P.astype(np.int64)
        h = P[:, ca] + P[:, cb]
        return wa * h[ra, :] + wb * h[rb, :]
    cu = up(U) - 8 * mid
    cv = up(V) - 8 * mid
    yv = (Y.astype(np.int64) - k["YOFF"]) * 8 * k["KY"]
    R = (yv + k["KRV"] * cv + (1 << 18)) >> 19
    G = (yv - k["KGU"] * cu - k["KGV"] * cv + (1 << 18)) >> 19
    B = (yv + k["KBU"] * cu + (1 << 18)) >> 19
    return np.stack([_clamp(B, depth), _clamp(G, depth), _clamp(R, depth)])


def bgr_to_yuv420(bgr, matrix, rng, depth=8):
    """Planar BGR [3,H,W] code values -> (Y [H,W], U, V [ceil(H/2), ceil(W/2)])."""
    k = constants(matrix, rng, depth)
    mid = 128 << (depth - 8)
    B, G, R = (bgr[c].astype(np.int64) for c in range(3))
    H, W = B.shape
    ch, cw = chroma_size(H, W)
    Y = ((k["KYR"] * R + k["KYG"] * G + k["KYB"] * B + (1 << 15)) >> 16) + k["YOFF"]
    i = np.arange(cw)
    j = np.arange(ch)
    c0, c1, c2 = np.clip(2 * i - 1, 0, W - 1), 2 * i, np.minimum(2 * i + 1, W - 1)
    r0, r1 = 2 * j, np.minimum(2 * j + 1, H - 1)

    def down(kr_, kg_, kb_):
        p = kr_ * R + kg_ * G + kb_ * B
        v = p[r0, :] + p[r1, :]
        s = v[:, c0] + 2 * v[:, c1] + v[:, c2]
        return np.ascontiguousarray(_clamp(((s + (1 << 18)) >> 19) + mid, depth))
    return _clamp(Y, depth), down(k["KUR"], k["KUG"], k["KUB"]), down(k["KVR"], k["KVG"], k["KVB"])


# ---- 4:4:4 forms of the same constants ----------------------------------------------------------------------------------------------
def rgb_to_yuv444(R, G, B, matrix, rng, depth=8):
    k = constants(matrix, rng, depth)
    mid, mx = 128 << (depth - 8), (1 << depth) - 1
    R, G, B = (np.asarray(a, dtype=np.int64) for a in (R, G, B))
    Y = ((k["KYR"] * R + k["KYG"] * G + k["KYB"] * B + (1 << 15)) >> 16) + k["YOFF"]
    U = ((k["KUR"] * R + k["KUG"] * G + k["KUB"] * B + (1 << 15)) >> 16) + mid
    V = ((k["KVR"] * R + k["KVG"] * G + k["KVB"] * B + (1 << 15)) >> 16) + mid
    return np.clip(Y, 0, mx), np.clip(U, 0, mx), np.clip(V, 0, mx)


def yuv444_to_rgb(Y, U, V, matrix, rng, depth=8):
    k = constants(matrix, rng, depth)
    mid, mx = 128 << (depth - 8), (1 << depth) - 1
    Y, U, V = (np.asarray(a, dtype=np.int64) for a in (Y, U, V))
    cu, cv = 8 * (U - mid), 8 * (V - mid)
    yv = (Y - k["YOFF"]) * 8 * k["KY"]
    R = (yv + k["KRV"] * cv + (1 << 18)) >> 19
    G = (yv - k["KGU"] * cu - k["KGV"] * cv + (1 << 18)) >> 19
    B = (yv + k["KBU"] * cu + (1 << 18)) >> 19
    return np.clip(R, 0, mx), np.clip(G, 0, mx), np.clip(B, 0, mx)


# ---- containers -------------------------------------------------------------------------------------------------------------------
def pack_planes(Y, U, V, layout, depth=8, dirt=None):
    """Code-value planes -> the planes of the container: nv12 -> (Y, UV interleaved), i420 -> (Y, U, V).  At depth 10 the words are
    uint16: P010 (nv12) holds value << 6, yuv420p10le (i420) the value.  dirt: a numpy Generator that fills the six bits the
    container does not use with random bits (readers must ignore them)."""
    if layout == "nv12":
        uv = np.empty((U.shape[0], 2 * U.shape[1]), U.dtype)
        uv[:, 0::2], uv[:, 1::2] = U, V
        planes = [Y, uv]
    else:
        planes = [Y, U, V]
    if depth == 8:
        return tuple(np.ascontiguousarray(p) for p in planes)
    out = []
    for p in planes:
        w = p.astype(np.uint16)
        if layout == "nv12":
            w = w << 6
            if dirt is not None:
                w = w | dirt.integers(0, 64, w.shape).astype(np.uint16)
        elif dirt is not None:
            w = w | (dirt.integers(0, 64, w.shape).astype(np.uint16) << 10)
        out.append(np.ascontiguousarray(w))
    return tuple(out)


def unpack_planes(planes, layout, depth=8):
    """The inverse: container planes -> (Y, U, V) code values."""
    if depth == 10:
        planes = [(p >> 6) if layout == "nv12" else (p & 0x3ff) for p in planes]
    if layout == "nv12":
        return planes[0], planes[1][:, 0::2], planes[1][:, 1::2]
    return tuple(planes)
