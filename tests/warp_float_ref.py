"""The backward warp, the splat metric built on it and the bilinear resize in float64, written from their definitions and not from the
kernels or the oracle: plain index arithmetic in numpy, no call to grid_sample or interpolate, no shared code with
oracle/fldr_oracle.py.  It is what the fp32 oracle (and through it the HIP kernels) is held to (tests/test_warp_ref_cpu.py,
tests/test_gpu_warp_ops.py).

  Backward warp of a plane X[H, W] by a flow (fx, fy) in pixels.  Output pixel (i, j) (column i, row j) looks at v = (i + fx, j + fy).
  The model normalises v to g = 2 v / max(S - 1, 1) - 1 per axis of S samples and hands g to a sampler whose convention
  (align_corners = False) places g = -1 and g = +1 on the outer EDGES of the first and last sample: s = ((g + 1) S - 1) / 2 in sample
  units.  (The two conventions differ, so a zero flow is a slight zoom about the centre: s = v S / (S - 1) - 1/2.)  The value is the
  bilinear interpolation of the four samples around s, samples outside the plane counting as zero.
  Mask: the same interpolation of a plane of ones, i.e. the sum of the weights of the corners inside the plane; the output is kept
  where that sum is at least `threshold` (0.999) and zeroed elsewhere.
  Splat metric: z = mean over channels of alpha |I - bwarp(other, flow)| with the mask applied.
  Bilinear resize of X[h, w] to [H, W] (align_corners = False): output o of an axis reads source position r = max(scale (o + 1/2) -
  1/2, 0) with scale = in / out, between samples i0 = floor(r) and min(i0 + 1, in - 1) with weight r - i0 on the latter; times mul."""
import numpy as np

MASK_THRESHOLD = 0.999


def _positions(flow, H, W):
    """flow [N,2,H,W] -> sample-unit positions (sx, sy), each [N,H,W] float64."""
    f = np.asarray(flow, np.float64)
    vx = np.arange(W, dtype=np.float64)[None, None, :] + f[:, 0]
    vy = np.arange(H, dtype=np.float64)[None, :, None] + f[:, 1]
    gx = 2.0 * vx / max(W - 1, 1) - 1.0
    gy = 2.0 * vy / max(H - 1, 1) - 1.0
    return ((gx + 1.0) * W - 1.0) / 2.0, ((gy + 1.0) * H - 1.0) / 2.0


def _corners(flow, H, W):
    """The four corners of every output pixel: [(column index, row index, weight, inside)], arrays [N,H,W]."""
    sx, sy = _positions(flow, H, W)
    x0, y0 = np.floor(sx), np.floor(sy)
    ax, ay = sx - x0, sy - y0
    out = []
    for dy, wy in ((0, 1.0 - ay), (1, ay)):
        for dx, wx in ((0, 1.0 - ax), (1, ax)):
            cx, cy = x0 + dx, y0 + dy
            inside = (cx >= 0) & (cx <= W - 1) & (cy >= 0) & (cy <= H - 1)
            out.append((np.where(inside, cx, 0).astype(np.int64), np.where(inside, cy, 0).astype(np.int64), wx * wy, inside))
    return out


def bwarp_mask_value(flow, H, W):
    """[N,1,H,W]: the sum of the weights of the corners inside the plane (what the threshold is applied to)."""
    return sum(np.where(ins, wt, 0.0) for _, _, wt, ins in _corners(flow, H, W))[:, None]


def bwarp(x, flow, withmask=True, threshold=MASK_THRESHOLD):
    """x [N,C,H,W], flow [N,2,H,W] -> float64 [N,C,H,W]."""
    x = np.asarray(x, np.float64)
    N, C, H, W = x.shape
    corners = _corners(flow, H, W)
    n = np.arange(N)[:, None, None]
    out = np.zeros((N, C, H, W))
    for c in range(C):
        for cx, cy, wt, ins in corners:
            out[:, c] += np.where(ins, x[n, c, cy, cx] * wt, 0.0)
    if withmask:
        out *= (bwarp_mask_value(flow, H, W) >= threshold)
    return out


def zmetric(self_img, other, flow, alpha):
    """-> float64 [N,1,H,W]."""
    d = np.abs(np.asarray(self_img, np.float64) - bwarp(other, flow, True))
    return (alpha * d).mean(axis=1, keepdims=True)


def _axis(n_in, n_out):
    r = np.maximum((n_in / n_out) * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5, 0.0)
    i0 = np.minimum(np.floor(r).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, r - i0


def resize_bilinear(x, H, W, mul=1.0):
    """x [N,C,h,w] -> float64 [N,C,H,W]."""
    x = np.asarray(x, np.float64)
    y0, y1, ly = _axis(x.shape[2], H)
    x0, x1, lx = _axis(x.shape[3], W)
    rows0, rows1 = x[:, :, y0], x[:, :, y1]
    top = rows0[..., x0] * (1.0 - lx) + rows0[..., x1] * lx
    bot = rows1[..., x0] * (1.0 - lx) + rows1[..., x1] * lx
    ly = ly[:, None]
    return (top * (1.0 - ly) + bot * ly) * mul
