"""The numpy statement of include/fldr_conform.h, section "THE RULE": the float64 matrix terms, the 14-bit integer table (coefs), the integer
conversion of a frame with its placement on a canvas (conform, in int64), and a float64 statement of the same conversion with unrounded
coefficients and no intermediate rounding (conform_float), which the CPU tests hold the integer rule to.  A format is (layout, matrix,
range, depth) with the names of tests/yuv_oracle.py; frames are tuples of 2-D numpy planes as fldr_video lays them out; sizes are (H, W)."""
import itertools

import numpy as np

from yuv_oracle import MATRICES, RANGES

LAYOUTS = ("nv12", "i420")
DEPTHS = (8, 10)
NAMES = ("KYY", "KYU", "KYV", "KUU", "KUV", "KVU", "KVV")
DITHER_NONE, DITHER_ORDERED = 0, 1
# every (matrix, range, depth): 8 a side, 64 pairs; with the two layouts a side, 256 format pairs
COLOURS = list(itertools.product(MATRICES, RANGES, DEPTHS))
FORMATS = [(l,) + c for l in LAYOUTS for c in COLOURS]


def side(rng, depth):
    """(yo, ys, cc, cs, mx) of a side."""
    sh, mx, lim = depth - 8, (1 << depth) - 1, rng == "limited"
    return (16 << sh if lim else 0), (219 << sh if lim else mx), 1 << (depth - 1), (224 << sh if lim else mx), mx


def matrix_terms(a, b):
    """(myu, myv, muu, muv, mvu, mvv) of YCbCr(a) -> YCbCr(b); the exact unit and zeros for equal matrices, by definition."""
    if a == b:
        return 0.0, 0.0, 1.0, 0.0, 0.0, 1.0
    kra, kba = MATRICES[a]
    kga = 1.0 - kra - kba
    krb, kbb = MATRICES[b]
    kgb = 1.0 - krb - kbb
    myu = 2.0 * (1.0 - kba) * (kbb - kgb * kba / kga)
    myv = 2.0 * (1.0 - kra) * (krb - kgb * kra / kga)
    muu = (2.0 * (1.0 - kba) - myu) / (2.0 * (1.0 - kbb))
    muv = -myv / (2.0 * (1.0 - kbb))
    mvv = (2.0 * (1.0 - kra) - myv) / (2.0 * (1.0 - krb))
    mvu = -myu / (2.0 * (1.0 - krb))
    return myu, myv, muu, muv, mvu, mvv


def coefs_float(src, dst):
    """The seven coefficients before rounding, as multiples of 1 (not of 16384): src, dst = (matrix, range, depth)."""
    myu, myv, muu, muv, mvu, mvv = matrix_terms(src[0], dst[0])
    _, ys_s, _, cs_s, _ = side(src[1], src[2])
    _, ys_d, _, cs_d, _ = side(dst[1], dst[2])
    ys_s, cs_s, ys_d, cs_d = float(ys_s), float(cs_s), float(ys_d), float(cs_d)
    return dict(KYY=ys_d / ys_s, KYU=myu * ys_d / cs_s, KYV=myv * ys_d / cs_s, KUU=muu * cs_d / cs_s, KUV=muv * cs_d / cs_s,
                KVU=mvu * cs_d / cs_s, KVV=mvv * cs_d / cs_s)


def coefs(src, dst):
    """The integer table: r(v) = floor(v * 16384 + 0.5) of each coefficient, as a dict by name."""
    return {k: int(np.floor(v * 16384.0 + 0.5)) for k, v in coefs_float(src, dst).items()}


def bayer(rows, cols):
    """B8[y & 7][x & 7] over a rows x cols plane, by the header's formula."""
    y, x = np.mgrid[0:rows, 0:cols].astype(np.int64)
    b = np.zeros((rows, cols), np.int64)
    for i in range(3):
        b |= ((((x >> i) ^ (y >> i)) & 1) << (5 - 2 * i)) | (((y >> i) & 1) << (4 - 2 * i))
    return b


def value(plane, layout, depth):
    """The sample values of a plane as int64."""
    p = plane.astype(np.int64)
    return p if depth != 10 else (p >> 6 if layout == "nv12" else p & 0x3ff)


def canonical(vals, layout, depth):
    if depth != 10:
        return vals.astype(np.uint8)
    return (vals << 6 if layout == "nv12" else vals).astype(np.uint16)


def split(frame, layout, depth):
    """(Y, U, V) sample values (int64) of a frame."""
    if layout == "nv12":
        uv = value(frame[1], layout, depth)
        return value(frame[0], layout, depth), uv[:, 0::2], uv[:, 1::2]
    return tuple(value(p, layout, depth) for p in frame)


def join(Y, U, V, layout, depth):
    """The frame of three value planes, in the container's canonical form."""
    if layout == "nv12":
        uv = np.empty((U.shape[0], 2 * U.shape[1]), np.int64)
        uv[:, 0::2], uv[:, 1::2] = U, V
        return canonical(Y, layout, depth), canonical(uv, layout, depth)
    return tuple(canonical(p, layout, depth) for p in (Y, U, V))


def upsampled(P, H, W, cc):
    """up() of tests/yuv_oracle.yuv420_to_bgr with cc in place of 128: the chroma plane P at the H x W luma sites, total weight 8, minus 8 cc."""
    ch, cw = P.shape
    x = np.arange(W)
    ca = np.where(x % 2 == 0, x // 2, (x - 1) // 2)
    cb = np.minimum(np.where(x % 2 == 0, x // 2, (x + 1) // 2), cw - 1)
    y = np.arange(H)
    ra = np.clip(np.where(y % 2 == 0, y // 2 - 1, (y - 1) // 2), 0, ch - 1)
    rb = np.clip(np.where(y % 2 == 0, y // 2, (y + 1) // 2), 0, ch - 1)
    wa = np.where(y % 2 == 0, 1, 3)[:, None]
    wb = 4 - wa
    h = P[:, ca] + P[:, cb]
    return wa * h[ra, :] + wb * h[rb, :] - 8 * cc


def sums(Y, U, V, src, dst):
    """The three integer sums before the rounding term and the shift (int64): luma over 2^17, chroma over 2^14."""
    k = coefs(src[1:], dst[1:])
    yo_s, _, cc_s, _, _ = side(src[2], src[3])
    H, W = Y.shape
    cu, cv = upsampled(U, H, W, cc_s), upsampled(V, H, W, cc_s)
    return (8 * k["KYY"] * (Y - yo_s) + k["KYU"] * cu + k["KYV"] * cv, k["KUU"] * (U - cc_s) + k["KUV"] * (V - cc_s),
            k["KVU"] * (U - cc_s) + k["KVV"] * (V - cc_s))


def conform(frame, src, dst, out_size=None, at=(0, 0), dither=DITHER_NONE, clamped=None):
    """frame in src = (layout, matrix, range, depth) -> the out_size canvas in dst with the picture's top-left luma sample at `at` =
    (x, y).  clamped: a list that receives the number of samples the final clamp changed."""
    Y, U, V = split(frame, src[0], src[3])
    H, W = Y.shape
    oH, oW = out_size or (H, W)
    dx, dy = at
    assert dx % 2 == 0 and dy % 2 == 0 and 0 <= dx <= oW - W and 0 <= dy <= oH - H
    yo_d, _, cc_d, _, mx_d = side(dst[2], dst[3])
    sy, su, sv = sums(Y, U, V, src, dst)
    och, ocw = (oH + 1) // 2, (oW + 1) // 2
    ch, cw = U.shape
    if dither:
        ry, rc = (2 * bayer(oH, oW) + 1) << 10, (2 * bayer(och, ocw) + 1) << 7
    else:
        ry, rc = np.full((oH, oW), 1 << 16, np.int64), np.full((och, ocw), 1 << 13, np.int64)
    oy = np.full((oH, oW), yo_d, np.int64)
    ou = np.full((och, ocw), cc_d, np.int64)
    ov = np.full((och, ocw), cc_d, np.int64)
    raw = [yo_d + ((sy + ry[dy:dy + H, dx:dx + W]) >> 17)]
    cr = rc[dy // 2:dy // 2 + ch, dx // 2:dx // 2 + cw]
    raw += [cc_d + ((su + cr) >> 14), cc_d + ((sv + cr) >> 14)]
    if clamped is not None:
        clamped.append(sum(int(((p < 0) | (p > mx_d)).sum()) for p in raw))
    oy[dy:dy + H, dx:dx + W] = np.clip(raw[0], 0, mx_d)
    ou[dy // 2:dy // 2 + ch, dx // 2:dx // 2 + cw] = np.clip(raw[1], 0, mx_d)
    ov[dy // 2:dy // 2 + ch, dx // 2:dx // 2 + cw] = np.clip(raw[2], 0, mx_d)
    return join(oy, ou, ov, dst[0], dst[3])


def conform_float(frame, src, dst):
    """The float64 statement: the same sites and taps, unrounded coefficients, no rounding anywhere -> (Y', U', V') as float64 planes,
    unclamped."""
    Y, U, V = (p.astype(np.float64) for p in split(frame, src[0], src[3]))
    k = coefs_float(src[1:], dst[1:])
    yo_s, _, cc_s, _, _ = side(src[2], src[3])
    yo_d, _, cc_d, _, _ = side(dst[2], dst[3])
    H, W = Y.shape
    cu, cv = upsampled(U, H, W, cc_s) / 8.0, upsampled(V, H, W, cc_s) / 8.0
    return (yo_d + k["KYY"] * (Y - yo_s) + k["KYU"] * cu + k["KYV"] * cv, cc_d + k["KUU"] * (U - cc_s) + k["KUV"] * (V - cc_s),
            cc_d + k["KVU"] * (U - cc_s) + k["KVV"] * (V - cc_s))


def worst_sums():
    """(the largest |luma sum + rounding|, the largest |chroma sum + rounding|) any source code values can reach, over all 64 colour pairs:
    what must fit int32."""
    worst_y = worst_c = 0
    for s, d in itertools.product(COLOURS, COLOURS):
        k = coefs(s, d)
        yo_s, _, cc_s, _, mx_s = side(s[1], s[2])
        yo_d = side(d[1], d[2])[0]
        cmax = 8 * max(cc_s, mx_s - cc_s)                               # |cu|, |cv| <= 8 max|c - cc_s|
        ymax = max(yo_s, mx_s - yo_s)
        worst_y = max(worst_y, 8 * abs(k["KYY"]) * ymax + (abs(k["KYU"]) + abs(k["KYV"])) * cmax + (1 << 17) + (yo_d << 17))
        cm = cmax // 8
        worst_c = max(worst_c, (abs(k["KUU"]) + abs(k["KUV"])) * cm + (1 << 14) + (1 << 23), (abs(k["KVU"]) + abs(k["KVV"])) * cm + (1 << 14) + (1 << 23))
    return worst_y, worst_c


def view(frame, layout, x, y, size):
    """The window of `size` = (H, W) of a frame that starts at even (x, y): plane slices."""
    H, W = size
    ch, cw = (H + 1) // 2, (W + 1) // 2
    if layout == "nv12":
        return frame[0][y:y + H, x:x + W], frame[1][y // 2:y // 2 + ch, x:x + 2 * cw]
    return frame[0][y:y + H, x:x + W], frame[1][y // 2:y // 2 + ch, x // 2:x // 2 + cw], frame[2][y // 2:y // 2 + ch, x // 2:x // 2 + cw]
