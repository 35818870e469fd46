"""The colour definition of the video API in float64, written from the standards and not from the kernels: no shifts, no integer tables, no
rounding, no shared code with tests/yuv_oracle.py / tests/yuv_hd_oracle.py.  It is what the integer oracles (and through them the kernels)
are held to, within half a code for the rounding plus the quantisation of the 16-bit coefficients (tests/test_video_cpu.py,
tests/test_video10_cpu.py).

  R'G'B' in [0, 1] = code / (2^d - 1).  E'y = Kr R' + Kg G' + Kb B', E'cb = (B' - E'y) / (2 (1 - Kb)), E'cr = (R' - E'y) / (2 (1 - Kr))
  (BT.601: Kr 0.299, Kb 0.114; BT.709: Kr 0.2126, Kb 0.0722; Kg = 1 - Kr - Kb).
  Limited range at depth d: Y = (219 E'y + 16) 2^(d-8), C = (224 E'c + 128) 2^(d-8).  Full range: Y = (2^d - 1) E'y, C = (2^d - 1) E'c + 2^(d-1).
  4:2:0, chroma sample (i, j) sited at luma (2i, 2j + 1/2): upsampling is linear interpolation between the two nearest chroma samples per
  axis (vertical weights 1/4 and 3/4; horizontal 1 on a co-sited column, 1/2 + 1/2 between two), downsampling the 1-2-1 / 4 filter along x
  and 1-1 / 2 along y centred on the sample; indices outside the plane repeat the edge.

Functions return unrounded float64 code values, clipped to 0 .. 2^d - 1 only where `clip` says so."""
import numpy as np

KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}


def levels(rng, depth):
    """(luma excursion, chroma excursion, luma offset, chroma centre, white RGB code) in codes."""
    s = float(1 << (depth - 8))
    mx = float((1 << depth) - 1)
    return (219.0 * s, 224.0 * s, 16.0 * s, 128.0 * s, mx) if rng == "limited" else (mx, mx, 0.0, 128.0 * s, mx)


def rgb_to_ycbcr(R, G, B, matrix, rng, depth=8):
    """Code values -> (Y, Cb, Cr) float code values, not clipped."""
    kr, kb = KR_KB[matrix]
    ey_scale, ec_scale, yoff, mid, mx = levels(rng, depth)
    r, g, b = (np.asarray(a, np.float64) / mx for a in (R, G, B))
    ey = kr * r + (1.0 - kr - kb) * g + kb * b
    return yoff + ey_scale * ey, mid + ec_scale * (b - ey) / (2.0 * (1.0 - kb)), mid + ec_scale * (r - ey) / (2.0 * (1.0 - kr))


def ycbcr_to_rgb(Y, Cb, Cr, matrix, rng, depth=8):
    """(Y, Cb, Cr) code values (float allowed) -> (R, G, B) float code values, not clipped."""
    kr, kb = KR_KB[matrix]
    ey_scale, ec_scale, yoff, mid, mx = levels(rng, depth)
    ey = (np.asarray(Y, np.float64) - yoff) / ey_scale
    ecb = (np.asarray(Cb, np.float64) - mid) / ec_scale
    ecr = (np.asarray(Cr, np.float64) - mid) / ec_scale
    r = ey + 2.0 * (1.0 - kr) * ecr
    b = ey + 2.0 * (1.0 - kb) * ecb
    g = (ey - kr * r - kb * b) / (1.0 - kr - kb)
    return mx * r, mx * g, mx * b


def clip(a, depth=8):
    return np.clip(a, 0.0, float((1 << depth) - 1))


def _edge(idx, n):
    return np.clip(idx, 0, n - 1)


def upsample_chroma(C, H, W):
    """A chroma plane [ceil(H/2), ceil(W/2)] -> [H, W] float64: linear interpolation at the luma positions for "left" siting."""
    C = np.asarray(C, np.float64)
    ch, cw = C.shape
    x = np.arange(W)
    # luma x sits at chroma coordinate x / 2: on sample x/2 (even x) or half way between (x-1)/2 and (x+1)/2 (odd x)
    x0, fx = np.floor(x / 2.0).astype(int), (x / 2.0) % 1.0
    h = (1.0 - fx)[None, :] * C[:, _edge(x0, cw)] + fx[None, :] * C[:, _edge(x0 + 1, cw)]
    # luma y sits at chroma coordinate (y - 1/2) / 2
    y = np.arange(H)
    cy = (y - 0.5) / 2.0
    y0 = np.floor(cy).astype(int)
    fy = cy - y0
    return (1.0 - fy)[:, None] * h[_edge(y0, ch), :] + fy[:, None] * h[_edge(y0 + 1, ch), :]


def downsample_chroma(P):
    """A full-resolution plane [H, W] -> [ceil(H/2), ceil(W/2)] float64: (1, 2, 1) / 4 along x around luma column 2i, (1, 1) / 2 over luma
    rows 2j, 2j + 1."""
    P = np.asarray(P, np.float64)
    H, W = P.shape
    i, j = np.arange((W + 1) // 2), np.arange((H + 1) // 2)
    v = 0.5 * (P[_edge(2 * j, H), :] + P[_edge(2 * j + 1, H), :])
    return 0.25 * v[:, _edge(2 * i - 1, W)] + 0.5 * v[:, 2 * i] + 0.25 * v[:, _edge(2 * i + 1, W)]


def yuv420_to_bgr(Y, U, V, matrix, rng, depth=8):
    """-> planar BGR [3,H,W] float64, clipped."""
    H, W = np.asarray(Y).shape
    R, G, B = ycbcr_to_rgb(Y, upsample_chroma(U, H, W), upsample_chroma(V, H, W), matrix, rng, depth)
    return np.stack([clip(B, depth), clip(G, depth), clip(R, depth)])


def bgr_to_yuv420(bgr, matrix, rng, depth=8):
    """-> (Y [H,W], U, V [ceil(H/2), ceil(W/2)]) float64, clipped."""
    Y, Cb, Cr = rgb_to_ycbcr(bgr[2], bgr[1], bgr[0], matrix, rng, depth)
    return clip(Y, depth), clip(downsample_chroma(Cb), depth), clip(downsample_chroma(Cr), depth)


def coefficient_bound(k, depth, direction):
    """The largest |integer result - float result| the 16-bit coefficients of table `k` (a dict as yuv_hd_oracle.constants returns) allow,
    without the rounding's half code: per output expression, the sum over its coefficients of 2^-17 (a coefficient is round(c 2^16) / 2^16)
    times the largest |operand| in codes; the largest over the expressions of `direction` ("to_rgb" / "to_yuv")."""
    mx, mid = (1 << depth) - 1, 1 << (depth - 1)
    q = 2.0 ** -17
    if direction == "to_rgb":
        ymax, cmax = max(mx - k["YOFF"], k["YOFF"]), max(mid, mx - mid)           # |Y - yoff|, |C - centre|
        return max(q * (ymax + cmax), q * (ymax + 2 * cmax))                        # R, B: KY, one chroma coefficient; G: KY and two
    return 3 * q * mx                                                               # Y, U, V: three coefficients on R, G, B
