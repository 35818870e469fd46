"""Seeded inputs of the forward-splat tests, shared by the CPU tests (tests/test_splat_ref_cpu.py: the oracle against the float64
statement of tests/splat_float_ref.py, the search model, the mutants) and the GPU tests (tests/test_gpu_splat_ops.py:
fldr_softsplat_acc64 and the producers of its bounds tables against the same statement).  Plain torch-CPU generators; every tensor
depends only on its case, the problem number and (for the metric) the mode.

A case is (config, N, C, H, W, flow kind, metric kind).  The shapes (H, W) are the smallest that reach each branch of the kernel
(csrc/splat_acc64_kernels.hip): image tiles are 64 x 24 walked as a column of three, feature tiles 32 x 8, source blocks 64 x 4,
super-blocks 256 x 64, the queue holds 512 blocks and 64 super-blocks, maps of at most 2304 pixels need no tables.

  image configuration (C <= 3)
    (1, 1) (1, 70) (70, 1) (2, 2)                  degenerate maps;
    (23, 63) (24, 64) (25, 65) (72, 64) (73, 68)   one short of a tile, one tile, one past it, the column of three and one row past it;
                                                   W % 4 != 0 takes the one-pixel walk, W % 4 == 0 the runs of four;
    (36, 64) (37, 64)                              2304 pixels (whole-map walk) and 2368 (tables);
    (1040, 65) (1040, 68)                          520 blocks > 512, 17 super-blocks: block-queue overflow under both walks;
    (4100, 8) (8, 16388)                           65 super-blocks > 64: the super-block search, one super-block wide / high.
  feature configuration (C > 3: groups of 16 channels; C = 4 leaves twelve dead channels, C = 17 a nearly empty second group and a
  third packed group of 8)
    (7, 31) (8, 32) (9, 33) (36, 64) (37, 64), and (1040, 65) at C = 16, (4100, 8) at C = 4.

Flow kinds (pixels; channel 0 = x, 1 = y).  A_s = min(9, S / 2) on an axis of S samples keeps the thin maps populated:
  zero      no motion;
  integer   whole pixels, +-min(3, S // 2): every weight is 0 or 1;
  graze     integer + s d, s = +-1: three corners carry weights of about d and d^2.  d = 2^-20 where the target coordinates are below
            16; beyond, d = 2 ulp32 of the larger target coordinate, because the target position is an fp32 sum (x + flow) and a finer
            offset would be rounded away (1.5e-5 at 64 <= coordinate < 128);
  edge      nearly half of the sources land on columns -1, W - 1, W or rows -1, H - 1, H, plus a fraction of 0, 1/2, 2^-16 or
            1 - 2^-16 (a hair inside and a hair outside the frame), the rest move by less than half a pixel; where W >= 4, column
            W - 1 is reached in the even rows only by the sources of column 0, which land 2^-16 inside of column W;
  smooth    the bilinear upsampling of a low-resolution field of amplitude min(6, S / 2), as the model's flows are;
  random    uniform +-A_s;
  wild      half of the pixels uniform +-2 max(H, W) in both components, the others `random`, and (maps of more than 16 pixels) the first two pixels of
            every block's first column at -2 max(H, W) and +2 max(H, W): every block's bounds span the map (the 1 x 4 blocks of
            W = 65 too), so every block reaches every tile, and the near half keeps the map populated;
  outliers  `smooth` with 1 % of the vectors at +-3e9;
  collapse  every source lands in one cell (plus a fraction: its four neighbours);
  gone      `smooth` plus an offset of two map sizes: everything leaves the frame.
  half      (only with the `beyond` metric) whole pixels plus exactly 0.5 in x: weights 0.5.
Metric kinds (softmax; `linear` takes a positive metric of the same spread; summation and average take none):
  None; unit = randn; model = -20 u, u uniform in [0, 1) (never positive, as zmetric gives); wide = uniform +-30;
  beyond = uniform in [71, 85]: exp(m) > 2^102, so every normaliser lies beyond 2^100 and the true division behind st_recip_safe runs
  (the small side, below 2^-100, cannot be had without products below 2^-100, which the tests exclude); paired with `integer`,
  `zero` and `half` flows only, so that no product leaves the normal range.
Images are uniform in [-1, 1] on a grid of 2^-8, so that no nonzero value is small enough to push a product under 2^-100."""
import collections

import torch
import torch.nn.functional as F

Case = collections.namedtuple("Case", "config N C H W flow metric")

MODES = ("summation", "average", "linear", "softmax")
FLOW_KINDS = ["zero", "integer", "graze", "edge", "smooth", "random", "wild", "outliers", "collapse", "gone"]
METRIC_KINDS = [None, "unit", "model", "wide", "beyond"]
OUTLIER = 3.0e9
OUTLIER_SHARE = 0.01
BEYOND_RANGE = (71.0, 85.0)
EDGE_HAIR = 2.0 ** -16

IMAGE_SHAPES = [(1, 1), (1, 70), (70, 1), (2, 2), (23, 63), (24, 64), (25, 65), (72, 64), (73, 68), (36, 64), (37, 64)]
FEATURE_SHAPES = [(7, 31), (8, 32), (9, 33), (36, 64), (37, 64)]
FEATURE_C = (4, 16, 17, 48)
OVERFLOW_IMAGE = [(1040, 65), (1040, 68)]           # block-queue overflow
SUPER_IMAGE = [(4100, 8), (8, 16388)]               # super-block search
BIG_FEATURE = [(1040, 65, 16), (4100, 8, 4)]
MAX_PIXELS = 8 * 16388                              # the one map beyond the 67 600 pixels of (1040, 65)


def _image_cases():
    out = []
    for i, (H, W) in enumerate(IMAGE_SHAPES):
        for j in range(2):                          # two kinds per shape: 22 cases, every kind at least twice
            kind = FLOW_KINDS[(2 * i + j) % len(FLOW_KINDS)]
            metric = METRIC_KINDS[(i + 2 * j) % 4]
            if kind == "integer" or (kind == "zero" and j == 0):
                metric = "beyond"
            out.append(Case("image", 2 if (H, W) == (25, 65) else 1, 1 + (i + j) % 3, H, W, kind, metric))
    out.append(Case("image", 1, 3, 24, 64, "half", "beyond"))
    for k, (H, W) in enumerate(OVERFLOW_IMAGE + SUPER_IMAGE):
        out.append(Case("image", 1, 1 + k % 3, H, W, "wild", METRIC_KINDS[1 + k % 3]))
        out.append(Case("image", 1, 3 - k % 3, H, W, "smooth", METRIC_KINDS[(2 + k) % 4]))
    return out


def _feature_cases():
    out = []
    for i, (H, W) in enumerate(FEATURE_SHAPES):
        for j in range(4):                          # four kinds per shape: 20 cases, every kind twice, every C five times
            kind = FLOW_KINDS[(4 * i + j) % len(FLOW_KINDS)]
            metric = METRIC_KINDS[(i + j) % 4]
            if kind == "integer":
                metric = "beyond"
            out.append(Case("feature", 2 if (H, W, j) == (9, 33, 0) else 1, FEATURE_C[(i + j) % 4], H, W, kind, metric))
    out.append(Case("feature", 1, 17, 8, 32, "half", "beyond"))
    for H, W, C in BIG_FEATURE:
        out.append(Case("feature", 1, C, H, W, "wild", "model"))
        out.append(Case("feature", 1, C, H, W, "smooth", "unit"))
    return out


IMAGE_CASES = _image_cases()
FEATURE_CASES = _feature_cases()
CASES = IMAGE_CASES + FEATURE_CASES
# the shapes either side of the table threshold run through the other route as well (tests/test_gpu_splat_ops.py)
ROUTE_SHAPES = [(36, 64), (37, 64)]
# tile-edge and overflow shapes: what the test build's walks (one-pixel items, folded channel groups) are held to
HOOK_SHAPES = [(23, 63), (24, 64), (25, 65), (72, 64), (73, 68), (7, 31), (8, 32), (9, 33), (1040, 65), (1040, 68)]


def case_id(case):
    return "%s-%dx%dx%dx%d-%s-%s" % (case.config[:4], case.N, case.C, case.H, case.W, case.flow, case.metric)


def _gen(case, *key):
    seed = 4099
    for k in (CASES.index(case) if case in CASES else 977, case.N, case.C, case.H, case.W) + key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _uniform(g, shape, amp=1.0):
    return (torch.rand(*shape, generator=g) * 2 - 1) * amp


def _amp(S, top=9.0):
    return min(top, S / 2.0)


def _axes_amp(g, N, H, W, top=9.0):
    return _uniform(g, (N, 2, H, W)) * torch.tensor([_amp(W, top), _amp(H, top)]).view(1, 2, 1, 1)


def _smooth(g, N, H, W):
    lo = _uniform(g, (N, 2, max(H // 8, 1) + 1, max(W // 8, 1) + 1)) * torch.tensor([_amp(W, 6.0), _amp(H, 6.0)]).view(1, 2, 1, 1)
    return F.interpolate(lo, size=(H, W), mode="bilinear", align_corners=False)


def _whole(g, N, H, W):
    kx, ky = min(3, W // 2), min(3, H // 2)
    return torch.stack([torch.randint(-kx, kx + 1, (N, H, W), generator=g), torch.randint(-ky, ky + 1, (N, H, W), generator=g)], 1).float()


def _grid(N, H, W):
    xs = torch.arange(W, dtype=torch.float64).view(1, 1, W).expand(N, H, W)
    ys = torch.arange(H, dtype=torch.float64).view(1, H, 1).expand(N, H, W)
    return torch.stack([xs, ys], 1)


def graze_offset(target):
    """d of the `graze` kind for a whole-pixel target coordinate pair [N,2,H,W] (float64): 2^-20, or two fp32 ulps of the larger one."""
    m = target.abs().amax(1, keepdim=True).clamp(min=1.0)
    ulp = torch.pow(2.0, torch.floor(torch.log2(m)) - 23)
    return torch.clamp(2 * ulp, min=2.0 ** -20)


def flow(case, problem=0):
    """-> fp32 [N,2,H,W]; `problem` selects the second problem of a two-problem launch (another seed, the same kind)."""
    N, H, W, kind = case.N, case.H, case.W, case.flow
    g = _gen(case, 1, problem)
    if kind == "zero":
        return torch.zeros(N, 2, H, W)
    if kind == "integer":
        return _whole(g, N, H, W)
    if kind == "half":
        f = _whole(g, N, H, W)
        f[:, 0] += 0.5
        return f
    if kind == "graze":
        grid = _grid(N, H, W)
        target = grid + _whole(g, N, H, W).double()
        s = torch.randint(0, 2, (N, 2, H, W), generator=g).double() * 2 - 1
        return (target + s * graze_offset(target) - grid).float()          # exact: multiples of d below 8 in magnitude
    if kind == "edge":
        grid = _grid(N, H, W)
        lim = torch.tensor([W, H], dtype=torch.float64).view(1, 2, 1, 1)
        pick = torch.randint(0, 3, (N, 2, H, W), generator=g)             # -1, S - 1, S
        pick[:, 0, 0::2][pick[:, 0, 0::2] == 1] = 2                       # (even rows keep column W - 1 free for the hair below)
        landing = torch.where(pick == 0, -torch.ones_like(lim), torch.where(pick == 1, lim - 1, lim)).expand(N, 2, H, W)
        frac = torch.tensor([0.0, 0.5, EDGE_HAIR, 1 - EDGE_HAIR], dtype=torch.float64)[torch.randint(0, 4, (N, 2, H, W), generator=g)]
        near = _uniform(g, (N, 2, H, W), 0.49).double()
        on_edge = torch.rand(N, 2, H, W, generator=g) < 0.25             # per component: about half of the sources have one
        f = torch.where(on_edge, landing + frac - grid, near).float()
        if W >= 4:                                                        # column W - 1 is reached by one hair only, in the even rows:
            f[:, 0, :, W - 1] = 1.0                                       # its own sources land exactly on column W,
            f[:, 0, :, W - 2] = -0.25                                     # its neighbours lean away from it,
            f[:, 0, :, 0] = W - EDGE_HAIR                                 # and column 0's sources land a hair inside of column W
            f[:, 1, :, 0] = 0.0
        return f
    if kind == "smooth":
        return _smooth(g, N, H, W)
    if kind == "random":
        return _axes_amp(g, N, H, W)
    if kind == "wild":
        near = _axes_amp(g, N, H, W)
        far = _uniform(g, (N, 2, H, W), 2.0 * max(H, W))
        f = torch.where(torch.rand(N, 1, H, W, generator=g) < 0.5, far, near)
        if H * W > 16:                                                    # the first two pixels of every block's first column: both extremes
            f[:, :, 0::4, 0::64] = -2.0 * max(H, W)
            f[:, :, 1::4, 0::64] = 2.0 * max(H, W)
        return f
    if kind == "outliers":
        f = _smooth(g, N, H, W)
        hit = torch.rand(N, 1, H, W, generator=g) < OUTLIER_SHARE
        sign = torch.randint(0, 2, (N, 2, H, W), generator=g).float() * 2 - 1
        return torch.where(hit, sign * OUTLIER, f)
    if kind == "collapse":
        cell = torch.tensor([W // 2 + 0.3, H // 2 + 0.6], dtype=torch.float64).view(1, 2, 1, 1)
        return (cell - _grid(N, H, W)).float()
    assert kind == "gone", kind
    return _smooth(g, N, H, W) + torch.tensor([2.0 * W + 8, -2.0 * H - 8]).view(1, 2, 1, 1)


def image(case, problem=0):
    """fp32 [N,C,H,W], uniform in [-1, 1] on a grid of 2^-8."""
    g = _gen(case, 2, problem)
    return torch.randint(-256, 257, (case.N, case.C, case.H, case.W), generator=g).float() / 256


def metric(case, mode, problem=0):
    """The metric the mode takes: None for summation and average (and for softmax cases of kind None), a positive one for linear."""
    if mode in ("summation", "average"):
        return None
    kind = case.metric
    shape = (case.N, 1, case.H, case.W)
    g = _gen(case, 3, problem)
    if mode == "linear":
        if kind in (None, "unit"):
            return torch.randn(*shape, generator=g).abs() + 0.1
        if kind == "model":
            return 20 * torch.rand(*shape, generator=g) + 0.05
        if kind == "wide":
            return 30 * torch.rand(*shape, generator=g) + 0.05
        return torch.pow(2.0, 102 + 8 * torch.rand(*shape, generator=g))   # beyond
    if kind is None:
        return None
    if kind == "unit":
        return torch.randn(*shape, generator=g)
    if kind == "model":
        return -20 * torch.rand(*shape, generator=g)
    if kind == "wide":
        return _uniform(g, shape, 30.0)
    assert kind == "beyond", kind
    lo, hi = BEYOND_RANGE
    return lo + (hi - lo) * torch.rand(*shape, generator=g)


def problem(case, mode, k=0):
    """(img, flow, metric) of problem k of the case in the given mode."""
    return image(case, k), flow(case, k), metric(case, mode, k)


# ---- low-resolution fields of the table producers: (N, h, w, H, W) -----------------------------------------------------------
# ragged sizes, a non-integer ratio (75 -> 149), h or w of 1, W = 65, H not a multiple of 4, two samples (batch-strided slices).
# fldr_resize_bilinear_spk_bounds takes W < 4 w only (beyond, fldr_hip falls back to the two launches): the last three fields bring
# h = 1, w = 1 and W = 65 to that launch, which the ratios of 4 and more of the first list cannot.
LOWRES_CASES = [(1, 9, 15, 72, 120), (2, 13, 21, 26, 42), (1, 30, 75, 59, 149), (1, 1, 16, 8, 128), (1, 20, 1, 80, 4), (2, 7, 13, 35, 65),
                (1, 34, 40, 68, 80), (1, 1, 33, 2, 65), (1, 20, 1, 40, 2), (2, 18, 33, 35, 65)]
LOWRES_FUSED = [c for c in LOWRES_CASES if c[4] < 4 * c[2]]          # the fields the fused resize + bounds launch accepts
LOWRES_T = (0.0, 0.3, 1.0)
LOWRES_AMPLITUDE = 3.0


def lowres_flow(case, seed=0):
    """fp32 [N,4,h,w] level flow (channels 0-1 flow_10, 2-3 flow_01), uniform +-LOWRES_AMPLITUDE."""
    N, h, w, H, W = case
    g = torch.Generator().manual_seed(7001 + 31 * (N + 7 * h + 53 * w + 211 * H) + W + 100003 * seed)
    return _uniform(g, (N, 4, h, w), LOWRES_AMPLITUDE)


def all_metric_values():
    """Every softmax metric value of every case and problem, fp32: what exp is measured on."""
    vals = []
    for case in CASES:
        for k in range(2):
            m = metric(case, "softmax", k)
            if m is not None:
                vals.append(m.flatten())
    return torch.cat(vals)


_exp = []


def exp_distance():
    """The largest distance in ulps between torch's fp32 exp on the CPU and float64 exp over all_metric_values() (measured once per
    process, on the machine that runs the test: the figures in the docstring of tests/test_splat_ref_cpu.py are what one build gave,
    the bound follows whatever this measures, and the CPU test holds it under one ulp)."""
    if not _exp:
        import splat_float_ref
        m = all_metric_values()
        _exp.append(splat_float_ref.exp_ulp_distance(m.numpy(), torch.exp(m).numpy()))
    return _exp[0]


def exp_allowance():
    """The exp term of the bound: twice the measured distance, for another IEEE-class implementation on the device."""
    return 2 * exp_distance()


def tile_geometry(case):
    """(TW, TH, K): tile width, height and tiles per workgroup column of the case's configuration."""
    return (64, 24, 3) if case.config == "image" else (32, 8, 1)


assert all(c.H * c.W <= MAX_PIXELS for c in CASES)
