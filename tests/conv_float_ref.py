"""The float64 statement of the library's convolutions and the per-pixel bound a correct kernel stays within.

Statement (plain float64 torch, no library code): concatenate the sources along the channels, a nearest-x2 source read by index
(y // 2, x // 2); zero padding 1; F.conv2d in float64 (3x3 stride 1 or 4x4 stride 2); bias; ReLU; the residual AFTER the activation;
the first `cout_store` channels.

Bound.  u = 2^-24 (half an fp32 ulp of 1), n = cin k k products per output.  Per output pixel, in float64 and over real taps only (a
tap in the padding contributes nothing):
    S   = conv(|x|, |w|) + |b| + |residual|       the magnitude sum
    A_w = conv(1 inside the frame, |w|)           sum of |w| over the real taps
    A_x = conv(|x|, 1)                            sum of |x| over the real taps
The bound is derived from the arithmetic alone; nothing in it is a measurement of the kernels.

  Accumulation (every kernel).  The n products are summed in fp32 in an order the kernels do not promise (MFMA blocks, chunks of
  channels, tap pairs), then the bias and the residual are added: n + 1 additions.  The rounding of a partial sum INSIDE a matrix
  instruction is not documented, so every addition is charged 2 u instead of u, and the usual first-order sum bound (each of the n + 2
  terms passes through at most n + 2 roundings of relative size 2 u; the factor (1 + 2u)^(n+2) - 1 is within 1e-4 of 2 (n + 2) u for
  n <= 1600) gives
      E_acc = 2 (n + 2) u S.
  The weight scale is a power of two and is undone exactly.  ReLU and the channel slice do not increase an error.  The exact
  fp32 kernel (fldr_conv2d, precision "fp32": fp32 products are exact in the fp32 matrix instruction's wider product) has E_acc alone.

  Split representation (fldr_split_hl; three products hi hi + hi lo + lo hi).  Let 2^e <= |x| < 2^(e+1).  Activations: hi = x
  truncated to 11 significant bits, so the remainder r = x - hi is below 2^(e-10) <= 2^-10 |x| and its leading bit is at e - 11 or
  lower; lo = r rounded to fp16's 11 bits, spacing at most 2^(e-21): |x - (hi + lo)| <= 2^(e-22) <= 2^-22 |x| = 4 u |x| while lo is
  normal.  Weights (prepack: w' = w scale, hi = nearest fp16, lo = nearest fp16 of w' - hi): |r| <= 2^-11 |w'| and
  |w' - (hi + lo)| <= 2^-23 |w'|; the bound charges them 2^-22 as well.  The dropped product |lo_x lo_w| <= 2^-10 2^-11 |x w'|; the
  bound charges 2^-20.  Together
      E_rep = (4 + 4 + 16) u S = 24 u S,
  which covers the 14 u just derived and the second-order products of the three errors.
  Below |x| = 0.25 the remainder is below 2^-12 and lo approaches fp16's SUBNORMALS (multiples of 2^-24, from |r| < 2^-14 on): its
  rounding error is then up to 2^-25 whatever |x| is.  Below |x| = 2^-14 hi is subnormal too: the conversion rounds the fp32 truncation
  t to a multiple of 2^-24 (another 2^-25), and lo is formed from x - t, not from x - float(hi), so that error is not recovered.  An
  activation therefore carries an ABSOLUTE error of up to 2^-24, which reaches the output times |w_hi + w_lo| / scale <= (1 + 2^-9) |w|:
      E_abs = 2^-24 (1 + 2^-9) A_w  +  2^-24 (1 + 2^-9) / scale  A_x,       scale = 2^floor(log2(8192 / max|w|)),
  the second term being the same statement for the weights, whose halves live at w scale.  Without E_abs the relative part alone is
  exceeded several hundred-fold on data around 1e-4 (tests/test_conv_ref_cpu.py emulates the split and prints the ratios).

  precision "fp16" (3x3 stride 1 only: one product hi_x hi_w).  The code TRUNCATES the activation (the same hi as above: relative
  error below 2^-10) and ROUNDS the weight to nearest (prepack: below 2^-11).  (1 + 2^-10)(1 + 2^-11) - 1 < 2^-10 + 2^-11 + 2^-21:
      E_rep16 = (2^14 + 2^13 + 8) u S,   E_abs16 = 2^-25 (1 + 2^-10) (A_w + A_x / scale)
  (the conversions of a subnormal hi round to a multiple of 2^-24: 2^-25 each).  A stride-2 convolution has no one-product form:
  "fp16" runs its three-product kernel and is held to the split bound.

  Packed tensors.  A packed SOURCE or RESIDUAL is compared through the values it holds (hi + lo, exact in fp32): the statement is
  evaluated on those.  A packed OUTPUT is the split of the fp32 result y: by the activation figures above
      E_out = 2^-22 |y| + 2^-24,     |y| <= |ref| + E,
  E being the bound of the fp32 result."""
import copy

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
ACC = 2.0                     # charged per addition, in units of u
REP_SPLIT = 24.0              # units of u S
ABS_SPLIT = 2.0 ** -24 * (1 + 2.0 ** -9)
REP_FP16 = 2.0 ** 14 + 2.0 ** 13 + 8.0
ABS_FP16 = 2.0 ** -25 * (1 + 2.0 ** -10)
OUT_REL = 2.0 ** -22          # packed output: the split of the fp32 result
OUT_ABS = 2.0 ** -24


def cat(srcs, up2, parity=0, order=None):
    """The concatenated float64 input.  parity / order: mutants only (nearest-x2 index (i + parity) // 2; another source order)."""
    xs = []
    for s, u in zip(srcs, up2):
        s = s.double()
        if u:
            iy = ((torch.arange(2 * s.shape[2]) + parity) // 2).clamp(max=s.shape[2] - 1)
            ix = ((torch.arange(2 * s.shape[3]) + parity) // 2).clamp(max=s.shape[3] - 1)
            s = s[:, :, iy][:, :, :, ix]
        xs.append(s)
    if order is not None:
        xs = [xs[i] for i in order]
    return torch.cat(xs, 1)


def conv(x, w, stride, replicate=False):
    x = F.pad(x, (1, 1, 1, 1), mode="replicate" if replicate else "constant")
    return F.conv2d(x, w, None, stride=stride)


def finish(y, b, relu, res, store, res_first=False):
    """bias, ReLU, the residual after the activation, the stored channels.  res_first: the mutant that adds it before."""
    if b is not None:
        y = y + b.double().view(1, -1, 1, 1)
    if store:
        y = y[:, :store]
    if res is not None and res_first:
        y = y + res.double()
    if relu:
        y = F.relu(y)
    if res is not None and not res_first:
        y = y + res.double()
    return y


def statement(spec, srcs, w, b, res=None):
    return finish(conv(cat(srcs, spec.up2), w.double(), spec.stride), b, spec.relu, res, spec.store)


def prepack_scale(w):
    """The prepack's power-of-two weight scale, with its fp32 operations."""
    mx = np.float32(w.abs().max().item())
    if mx == 0:
        return 1.0
    return float(np.exp2(np.floor(np.log2(np.float32(8192.0) / mx))))


class Terms:
    """S (with |b| and |residual|), A_w, A_x of the stored channels, n and the prepack scale."""

    def __init__(self, spec, srcs, w, b, res=None):
        x = cat(srcs, spec.up2).abs()
        wa = w.double().abs()
        S = conv(x, wa, spec.stride)
        if b is not None:
            S = S + b.double().abs().view(1, -1, 1, 1)
        c = spec.store or spec.cout
        self.S = S[:, :c] + (res.double().abs() if res is not None else 0.0)
        self.A_w = conv(torch.ones_like(x[:, :1]).expand_as(x), wa, spec.stride)[:, :c]
        self.A_x = conv(x, torch.ones(1, x.shape[1], spec.k, spec.k, dtype=torch.float64), spec.stride)
        self.n = x.shape[1] * spec.k * spec.k
        self.scale = prepack_scale(w)

    def with_residual(self, res):
        """These terms for the same convolution with (another) residual added after the activation; built without one."""
        t = copy.copy(self)
        t.S = self.S + res.double().abs()
        return t

    def accumulation(self):
        return ACC * (self.n + 2) * U * self.S

    def representation(self, mode):
        if mode == "fp32":
            return torch.zeros_like(self.S)
        rel, ab = (REP_SPLIT, ABS_SPLIT) if mode == "split" else (REP_FP16, ABS_FP16)
        return rel * U * self.S + ab * (self.A_w + self.A_x / self.scale)

    def bound(self, mode, ref=None, packed_out=False):
        """mode: "fp32" (exact products), "split" (three fp16 products), "fp16" (one).  packed_out: for the values of a packed output
        (needs ref, the statement's result)."""
        assert mode in ("fp32", "split", "fp16"), mode
        e = self.accumulation() + self.representation(mode)
        if packed_out:
            e = e + OUT_REL * (ref.abs() + e) + OUT_ABS
        return e


# ---- emulation of the split operands (CPU tests) ------------------------------------------------------------------------------------
def split_activation(x):
    """fldr_split_hl on in-range values: hi = fp16(x & 0xFFFFE000), lo = fp16(x - that fp32 truncation); float64 tensors of the halves."""
    a = x.float().contiguous().numpy()
    t = (a.view(np.int32) & np.int32(-8192)).view(np.float32)           # 0xFFFFE000
    hi = t.astype(np.float16)
    lo = (a - t).astype(np.float16)
    return torch.from_numpy(hi.astype(np.float64)), torch.from_numpy(lo.astype(np.float64))


def split_weight(w, scale):
    """The prepack's halves of w scale: nearest fp16, and the nearest fp16 of what is left; float64 tensors."""
    a = (w.float().numpy() * np.float32(scale)).astype(np.float32)
    hi = a.astype(np.float16)
    lo = (a - hi.astype(np.float32)).astype(np.float16)
    return torch.from_numpy(hi.astype(np.float64)), torch.from_numpy(lo.astype(np.float64))


def emulated(spec, srcs, w, b, res=None, terms=3):
    """The convolution of the split operands with exact (float64) products and sums: what the matrix cores are given, without their
    accumulation rounding.  terms = 1: the one-product "fp16" form."""
    scale = prepack_scale(w)
    halves = [split_activation(s) for s in srcs]
    xh = cat([h for h, _ in halves], spec.up2)
    xl = cat([l for _, l in halves], spec.up2)
    wh, wl = split_weight(w, scale)
    y = conv(xh, wh, spec.stride)
    if terms == 3:
        y = y + conv(xh, wl, spec.stride) + conv(xl, wh, spec.stride)
    return finish(y / scale, b, spec.relu, res, spec.store)


# ---- the cases of tests/conv_cases.py, computed once per session and shared: read-only ------------------------------------------------
_cache = {}


def reference(case):
    """-> (inputs of conv_cases.make, the statement's result, Terms) of a case."""
    if case not in _cache:
        import conv_cases
        d = conv_cases.make(case)
        _cache[case] = (d, statement(case.spec, d["srcs"], d["w"], d["b"], d["res"]), Terms(case.spec, d["srcs"], d["w"], d["b"], d["res"]))
    return _cache[case]
