"""Seeded inputs of the backward-warp, splat-metric and bilinear-resize tests, shared by the CPU tests (tests/test_warp_ref_cpu.py:
the oracle against the float64 statement of tests/warp_float_ref.py) and the GPU tests (tests/test_gpu_warp_ops.py: the kernels
against the oracle).  Plain torch-CPU generators; every tensor depends only on its arguments.

Shapes are (N, C, H, W), at most 83 wide and 45 high: one row, one column, the smallest 2-D frame, exact and ragged 64 x 4 tiles in
x and y, three channel counts and a second sample.

Flow kinds (pixels; channel 0 = x, 1 = y):
  zero     all flows 0;
  noise A  uniform of amplitude A as the other tests of this suite count it, (rand - 0.5) A, i.e. +-A / 2; A = 2 and 14;
  aligned  the flow that lands pixel i exactly on source sample i of grid_sample(align_corners=False) after the model's
           normalisation by max(S - 1, 1): f = (i + 0.5)(S - 1) / S - i on an axis of S > 1 samples, 0.5 on an axis of one, plus
           uniform +-0.4 px along axes of 3 or more samples only.  The kind that the mask does not zero: with `zero` flows nothing
           survives at H <= 2 or W = 1 (every position sits half a sample outside);
  wild     +-1e9 on a seeded third of the pixels (x, y or both components), `noise 2` elsewhere.  Nothing larger and nothing
           non-finite: the reference's float-to-index cast is undefined beyond int64."""
import torch

SHAPES = [(1, 1, 1, 1), (1, 2, 1, 65), (2, 3, 5, 1), (1, 3, 2, 2), (1, 3, 4, 64), (2, 1, 5, 65), (1, 4, 3, 63), (2, 3, 9, 83)]

FLOW_KINDS = ["zero", "noise2", "noise14", "aligned", "wild"]
NOISE_AMPLITUDE = {"noise2": 2.0, "noise14": 14.0}
ALIGNED_NOISE = 0.4
WILD = 1.0e9

T_VALUES = (0.0, 0.125, 0.7, 1.0)
T_MODES = (None, "t", "1-t")

# (h, w, H, W, mul)
RESIZE_CASES = [(9, 15, 9, 15, 1.0), (9, 15, 18, 30, 2.0), (1, 15, 4, 65, 1.0), (9, 1, 5, 1, 3.0), (1, 1, 3, 63, 1.0),
                (12, 65, 5, 64, 0.5), (7, 33, 1, 1, 1.0), (5, 64, 20, 65, 4.0)]
RESIZE_NC = [(1, 1), (1, 4), (2, 4)]          # (N, C): N C = 1, 4, 8


def _gen(*key):
    seed = 20240
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _uniform(g, shape, amp):
    return (torch.rand(*shape, generator=g) * 2 - 1) * amp


def _aligned_axis(S):
    i = torch.arange(S, dtype=torch.float64)
    return ((i + 0.5) * (S - 1) / S - i).float() if S > 1 else torch.full((1,), 0.5)


def flow(kind, shape, seed=0):
    """-> (flow [N,2,H,W] fp32, wild [N,1,H,W] bool: the pixels that carry a +-1e9 component; all False but for `wild`)."""
    N, _, H, W = shape
    g = _gen(FLOW_KINDS.index(kind), N, H, W, seed)
    wild = torch.zeros(N, 1, H, W, dtype=torch.bool)
    if kind == "zero":
        return torch.zeros(N, 2, H, W), wild
    if kind in NOISE_AMPLITUDE:
        return _uniform(g, (N, 2, H, W), NOISE_AMPLITUDE[kind] / 2), wild
    if kind == "aligned":
        f = torch.empty(N, 2, H, W)
        f[:, 0] = _aligned_axis(W).view(1, 1, W)
        f[:, 1] = _aligned_axis(H).view(1, H, 1)
        n = _uniform(g, (N, 2, H, W), ALIGNED_NOISE)
        if W >= 3:
            f[:, 0] += n[:, 0]
        if H >= 3:
            f[:, 1] += n[:, 1]
        return f, wild
    assert kind == "wild", kind
    f = _uniform(g, (N, 2, H, W), NOISE_AMPLITUDE["noise2"] / 2)
    wild = torch.rand(N, 1, H, W, generator=g) < 1.0 / 3.0
    which = torch.randint(0, 3, (N, 1, H, W), generator=g)                # 0: x, 1: y, 2: both
    sign = torch.randint(0, 2, (N, 2, H, W), generator=g).float() * 2 - 1
    hit = torch.cat([wild & (which != 1), wild & (which != 0)], 1)
    return torch.where(hit, sign * WILD, f), wild


def image(shape, seed=0):
    """Unit-range planes: uniform in [-1, 1]."""
    return _uniform(_gen(101, *shape, seed), shape, 1.0)


def flow_planes(shape, seed=0):
    """Planes to be warped that are themselves flows, as in the model's flowback: uniform in +-7 px."""
    return _uniform(_gen(102, *shape, seed), shape, 7.0)


def t_values(k, N):
    """One t per sample for the k-th shape: over the shapes every value of T_VALUES occurs, so t and 1 - t both reach 0 and 1."""
    return torch.tensor([T_VALUES[(k + n) % len(T_VALUES)] for n in range(N)]).view(N, 1, 1, 1)


def t_scale(mode, t):
    """The fp32 factor of a scale mode: None -> 1 (no product is formed), 't' -> t, '1-t' -> 1 - t."""
    return None if mode is None else (t if mode == "t" else 1 - t)


def scaled(x, mode, t):
    s = t_scale(mode, t)
    return x if s is None else s * x


def resize_source(case, nc, seed=0):
    h, w, _, _, _ = case
    N, C = nc
    return torch.randn(N, C, h, w, generator=_gen(103, N, C, h, w, seed))
