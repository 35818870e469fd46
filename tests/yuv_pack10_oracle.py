"""numpy statement of the three containers of libfldr_pack10.so (include/fldr_pack10.h): v210, Y210 and Y410 <-> planes of 10-bit code
values.  Only the bit layouts live here; the colour definition is tests/yuv_chroma_oracle.py's at depth 10 (yuv_to_bgr / bgr_to_yuv,
imported, not copied): v210 and Y210 are 4:2:2, Y410 is 4:4:4.

    v210   rows of ceil(W/6) groups of four little-endian dwords, three 10-bit fields each (bits 0-9, 10-19, 20-29; bits 30-31 unused):
           U0 Y0 V0 | Y1 U1 Y2 | V1 Y3 U2 | Y4 V2 Y5
    y210   16-bit words Y0 U Y1 V per two pixels, the value in the high 10 bits
    y410   one dword per pixel: U bits 0-9, Y 10-19, V 20-29, alpha 30-31

Planes are numpy arrays: Y [H,W], U and V [H, ceil(W/2)] (v210, y210) or [H,W] (y410), uint16 code values 0 .. 1023; a frame is a tuple of
one array, uint32 [H, 4 ceil(W/6)] (v210), uint16 [H, 4 ceil(W/2)] (y210) or uint32 [H, W] (y410)."""
import numpy as np

from yuv_chroma_oracle import MATRICES, RANGES, bgr_to_yuv, chroma_width, yuv_to_bgr  # noqa: F401

CONTAINERS = ("v210", "y210", "y410")
SAMPLING = {"v210": "422", "y210": "422", "y410": "444"}
# (plane, slot) of the three fields of each of a group's four words, lowest field first: slots index the group's 6 luma / 3 chroma samples
V210_FIELDS = ((("U", 0), ("Y", 0), ("V", 0)), (("Y", 1), ("U", 1), ("Y", 2)), (("V", 1), ("Y", 3), ("U", 2)), (("Y", 4), ("V", 2), ("Y", 5)))


def containers():
    """Every container the library takes."""
    return list(CONTAINERS)


def row_words(container, W):
    """Words (of the plane's dtype) in a row of W pixels."""
    return 4 * ((W + 5) // 6) if container == "v210" else 4 * ((W + 1) // 2) if container == "y210" else W


def v210_pitch(W):
    """The customary pitch of a v210 row in bytes."""
    return 128 * ((W + 47) // 48)


def _extend(P, n, dirt):
    """P [H, w] -> [H, n]: the columns past w are the spare slots: random code values with dirt, copies of the last column without."""
    H, w = P.shape
    out = np.empty((H, n), np.uint32)
    out[:, :w] = P
    if n > w:
        out[:, w:] = dirt.integers(0, 1024, (H, n - w)) if dirt is not None else P[:, w - 1:w]
    return out


def pack(Y, U, V, container, dirt=None):
    """Code-value planes -> (plane,).  dirt: a numpy Generator that fills everything a reader must ignore with random bits: bits 30-31 of a
    v210 word and its spare slots (W % 6 != 0), the low six bits of a y210 word and the spare luma word of an odd-width row, the alpha bits
    of y410.  Without dirt those are what a writer produces: zero pad bits, spare luma slots = luma W - 1, spare chroma slots = the row's
    last chroma sample, alpha = 3."""
    H, W = Y.shape
    assert U.shape == (H, chroma_width(SAMPLING[container], W)) and V.shape == U.shape
    if container == "v210":
        ng = (W + 5) // 6
        S = {"Y": _extend(Y, 6 * ng, dirt), "U": _extend(U, 3 * ng, dirt), "V": _extend(V, 3 * ng, dirt)}
        out = np.zeros((H, 4 * ng), np.uint32)
        for w, fields in enumerate(V210_FIELDS):
            for b, (p, slot) in enumerate(fields):
                out[:, w::4] |= S[p][:, slot::(6 if p == "Y" else 3)] << np.uint32(10 * b)
        if dirt is not None:
            out |= dirt.integers(0, 4, out.shape).astype(np.uint32) << np.uint32(30)
        return (out,)
    if container == "y210":
        half = (W + 1) // 2
        Y2 = _extend(Y, 2 * half, dirt)
        out = np.empty((H, 4 * half), np.uint16)
        out[:, 0::4], out[:, 1::4], out[:, 2::4], out[:, 3::4] = Y2[:, 0::2] << 6, U.astype(np.uint16) << 6, Y2[:, 1::2] << 6, V.astype(np.uint16) << 6
        if dirt is not None:
            out |= dirt.integers(0, 64, out.shape).astype(np.uint16)
        return (out,)
    assert container == "y410"
    alpha = dirt.integers(0, 4, Y.shape).astype(np.uint32) if dirt is not None else np.uint32(3)
    return (np.ascontiguousarray(U.astype(np.uint32) | (Y.astype(np.uint32) << 10) | (V.astype(np.uint32) << 20) | (alpha << np.uint32(30))),)


def unpack(planes, container, W):
    """The inverse: (plane,) -> (Y, U, V) code values (uint16) of a row of W pixels."""
    p = planes[0]
    cw = chroma_width(SAMPLING[container], W)
    if container == "v210":
        H, ng = p.shape[0], p.shape[1] // 4
        S = {"Y": np.empty((H, 6 * ng), np.uint16), "U": np.empty((H, 3 * ng), np.uint16), "V": np.empty((H, 3 * ng), np.uint16)}
        for w, fields in enumerate(V210_FIELDS):
            for b, (q, slot) in enumerate(fields):
                S[q][:, slot::(6 if q == "Y" else 3)] = (p[:, w::4] >> np.uint32(10 * b)) & 0x3ff
        return tuple(np.ascontiguousarray(a) for a in (S["Y"][:, :W], S["U"][:, :cw], S["V"][:, :cw]))
    if container == "y210":
        v = p >> 6
        Y2 = np.empty((p.shape[0], p.shape[1] // 2), np.uint16)
        Y2[:, 0::2], Y2[:, 1::2] = v[:, 0::4], v[:, 2::4]
        return np.ascontiguousarray(Y2[:, :W]), np.ascontiguousarray(v[:, 1::4]), np.ascontiguousarray(v[:, 3::4])
    assert container == "y410"
    return tuple(np.ascontiguousarray(((p >> np.uint32(s)) & 0x3ff).astype(np.uint16)) for s in (10, 0, 20))
