"""numpy oracle of the colour definition of libfldr_video.so (include/fldr_video.h, fldr-vfi_amd/video/yuv_color.h): 8-bit YUV 4:2:0
<-> 8-bit BGR in integer fixed point, BT.601 / BT.709, limited / full range, chroma sited "left" (chroma sample (i, j) at luma
(2i, 2j + 1/2)).  Every expression is the kernels' own, in int64 (the kernels' int32 intermediates never overflow: tested), so the
bytes are the same.

Planes are numpy uint8 arrays: Y [H,W], U and V [ceil(H/2), ceil(W/2)]; BGR frames are planar [3,H,W] (plane c = BGR channel c)."""
import numpy as np

MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
RANGES = ("limited", "full")


def constants(matrix, rng):
    """The integer table, derived from Kr and Kb: each coefficient round(c * 2^16)."""
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    lim = rng == "limited"
    sy = 219.0 / 255.0 if lim else 1.0
    sc = 224.0 / 255.0 if lim else 1.0
    r = lambda v: int(np.floor(v * 65536.0 + 0.5))
    kyr, kyb = r(kr * sy), r(kb * sy)
    kyg = r(sy) - kyr - kyb                                   # KYR + KYG + KYB = round(sy * 2^16)
    kub = r(sc * 0.5)
    kur = r(-sc * 0.5 * kr / (1.0 - kb))
    kug = -kub - kur                                          # KUR + KUG = -KUB: grey has no chroma
    kvr = r(sc * 0.5)
    kvb = r(-sc * 0.5 * kb / (1.0 - kr))
    kvg = -kvr - kvb
    return dict(KYR=kyr, KYG=kyg, KYB=kyb, KUR=kur, KUG=kug, KUB=kub, KVR=kvr, KVG=kvg, KVB=kvb,
                KY=r(1.0 / sy), KRV=r(2.0 * (1.0 - kr) / sc), KBU=r(2.0 * (1.0 - kb) / sc),
                KGU=r(2.0 * (1.0 - kb) * kb / kg / sc), KGV=r(2.0 * (1.0 - kr) * kr / kg / sc),
                YOFF=16 if lim else 0)


def _clamp8(a):
    return np.clip(a, 0, 255).astype(np.uint8)


def chroma_size(H, W):
    return (H + 1) // 2, (W + 1) // 2


def yuv420_to_bgr(Y, U, V, matrix, rng):
    """YUV 4:2:0 planes -> planar BGR [3,H,W] uint8."""
    k = constants(matrix, rng)
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
        h = P[:, ca] + P[:, cb]                               # horizontal: 2 on x/2 (even x) or 1 + 1 (odd x)
        return wa * h[ra, :] + wb * h[rb, :]                  # vertical: (1, 3) or (3, 1); total 8
    cu = up(U) - 1024
    cv = up(V) - 1024
    yv = (Y.astype(np.int64) - k["YOFF"]) * 8 * k["KY"]
    R = (yv + k["KRV"] * cv + (1 << 18)) >> 19
    G = (yv - k["KGU"] * cu - k["KGV"] * cv + (1 << 18)) >> 19
    B = (yv + k["KBU"] * cu + (1 << 18)) >> 19
    return np.stack([_clamp8(B), _clamp8(G), _clamp8(R)])


def bgr_to_yuv420(bgr, matrix, rng):
    """Planar BGR [3,H,W] uint8 -> (Y [H,W], U, V [ceil(H/2), ceil(W/2)]) uint8."""
    k = constants(matrix, rng)
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
        v = p[r0, :] + p[r1, :]                               # vertical 1, 1
        s = v[:, c0] + 2 * v[:, c1] + v[:, c2]                # horizontal 1, 2, 1; total 8
        return np.ascontiguousarray(_clamp8(((s + (1 << 18)) >> 19) + 128))
    return _clamp8(Y), down(k["KUR"], k["KUG"], k["KUB"]), down(k["KVR"], k["KVG"], k["KVB"])


# ---- 4:4:4 forms of the same constants (the round-trip bound of the definition) ---------------------------------------------------
def rgb_to_yuv444(R, G, B, matrix, rng):
    k = constants(matrix, rng)
    R, G, B = (np.asarray(a, dtype=np.int64) for a in (R, G, B))
    Y = ((k["KYR"] * R + k["KYG"] * G + k["KYB"] * B + (1 << 15)) >> 16) + k["YOFF"]
    U = ((k["KUR"] * R + k["KUG"] * G + k["KUB"] * B + (1 << 15)) >> 16) + 128
    V = ((k["KVR"] * R + k["KVG"] * G + k["KVB"] * B + (1 << 15)) >> 16) + 128
    return np.clip(Y, 0, 255), np.clip(U, 0, 255), np.clip(V, 0, 255)


def yuv444_to_rgb(Y, U, V, matrix, rng):
    """Same as the 4:2:0 upsampling with every chroma weight on one sample (cu = 8 (U - 128))."""
    k = constants(matrix, rng)
    Y, U, V = (np.asarray(a, dtype=np.int64) for a in (Y, U, V))
    cu, cv = 8 * (U - 128), 8 * (V - 128)
    yv = (Y - k["YOFF"]) * 8 * k["KY"]
    R = (yv + k["KRV"] * cv + (1 << 18)) >> 19
    G = (yv - k["KGU"] * cu - k["KGV"] * cv + (1 << 18)) >> 19
    B = (yv + k["KBU"] * cu + (1 << 18)) >> 19
    return np.clip(R, 0, 255), np.clip(G, 0, 255), np.clip(B, 0, 255)


# ---- packing into the two layouts -----------------------------------------------------------------------------------------------
def pack_nv12(Y, U, V):
    """-> (Y, UV) with UV [ch, 2 cw] interleaved U, V."""
    uv = np.empty((U.shape[0], 2 * U.shape[1]), np.uint8)
    uv[:, 0::2], uv[:, 1::2] = U, V
    return Y, uv


def unpack_nv12(uv):
    return uv[:, 0::2], uv[:, 1::2]


def i420_bytes(Y, U, V):
    """One raw I420 frame (ffmpeg -pix_fmt yuv420p): Y, then U, then V, rows packed."""
    return Y.tobytes() + U.tobytes() + V.tobytes()
