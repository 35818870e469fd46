"""The float64 statement of the synthesis half (dec2, dec3, softmax / T, blend; fLDRnet.py:638-643, 511-524), its rounded forms, and
the per-pixel bound a correct kernel stays within.

Statement (plain float64 torch, no library code; the two layers through conv_float_ref):
    d2     = ReLU(conv3x3(cat(nearest-x2(dec1), enc1)) + b2)
    logits = conv3x3(nearest-x2(d2)) + b3
    occ    = softmax(logits / T) over the six candidates
    w_k    = (1 - t) FORMED IN fp32 and then widened for even k, t for odd k (the reference multiplies its fp32 t tensor into float64)
    out    = sum_k w_k occ_k cand_k / sum_k w_k occ_k
    rounded forms: crop to Hc x Wc, rint(clip((out + 1) / 2, 0, 1) white), half to even, white = 255 or maxval.

Bound.  u = 2^-24 and v = 2^-53 (half an ulp of 1 in fp32 / fp64).  Nothing in it is a measurement of the kernels; one term (the fp32
exponential's own error) is measured on the CPU and stated below.

  Combining formula.  The quotient only sees W_k = w_k exp(l_k / T) up to a common factor; let p_k = W_k / sum W be the statement's
  normalised weights.  If a kernel's weights are W_k (1 + d_k) (times any common factor) with |d_k| <= eta_k, then exactly
      out' - out = sum_k p_k d_k (c_k - out) / (1 + sum_k p_k d_k),
      |out' - out| <= sum_k p_k eta_k |c_k - out| / (1 - sum_k p_k eta_k)                         (F)
  as long as sum p eta < 1.  Every kernel's weights are non-negative and those of the candidates with w_k = 0 are exactly 0, so out'
  also lies between the smallest and the largest candidate with w_k != 0: (F) is capped by that span, and replaced by it where
  sum p eta >= 1.

  eta_k has three parts.
  (a) Logit error.  With |l'_k - l_k| <= E_k and E = max_k E_k at the pixel, the weight relative to the (moved) maximum changes by
      at most expm1((E_k + E) / T).  E is 0 in the exact and bias-only regimes (the kernels' logits are then the statement's bit for
      bit: asserted on the GPU where a kernel returns them).  Generic regime:
          E = Terms(dec3).bound(mode) + 4 u S3 + conv(|w3|, nearest-x2(E_d2)),
      mode "fp32" for the vector kernel and "split" for the matrix-core ones; 4 u S3 for the phase weights (dec3 on a nearest-x2 source
      runs as four 2x2 convolutions whose weights are sums of up to four fp32 taps: three additions, charged four); E_d2 =
      Terms(dec2).bound("split", packed_out=True) for the fused kernel, whose dec2 values are split-packed, and 0 where d2 is an input.
  (b) The exponential.
      fp32-exp kernel (fldr_dec23_synth): y_k = (l_k - max) * sc2 in fp32 with sc2 = fp32(log2(e) / T): three roundings (the
      subtraction, sc2, the product), 3 u |y_k| on the argument (charged 3.01 for the second order), i.e. 3.01 u ln(2) |y_k| on
      exp2(y_k); the exponential's own error A 2^-23 with A = exp2_allowance() ulps (below); the conversion to fp64 is exact.  The
      maximum is the largest logit whose w_k != 0.  exp2 on the transcendental unit returns 0 below 2^-126 and the bound allows any
      weight below 2^-120 of the largest to be dropped entirely: eta_k = 1 where y_k (less the logit error) < -120.
      fp64-exp kernels (fldr_dec3_synth, fldr_dec3_synth_spk, fldr_synth_tail): s_k = l_k / T (or l_k * (1 / T): two roundings),
      x_k = s_k - max s, exp(x_k): (2 |s_k| + 2 |max s| + 2 |x_k|) v on the argument and EXP64_ULPS = 2 ulps (4 v) for the library
      exp (documented as 1 ulp).  The maximum is over all six.  eta_k = 1 where x_k < -700.
  (c) fp64 roundings of a weight after the exponential: exp / sum (or * (1 / sum)) and w_k * ...: charged 4 v.
  The blend itself: six products and five additions (or an fma chain) over the numerator, five additions over the divisor, the
  reciprocal (or division) and the last product: at most 14 roundings on terms bounded by sum_k p_k |c_k|, charged BLEND = 16:
      E_blend = 16 v sum_k p_k |c_k|.
  fp32 output form: + 2^-24 (|out| + bound) + 2^-149 (half an fp32 ulp of the result).

  Rounded forms.  With V = (out + 1) / 2 white and D = bound white / 2: a pixel is `ill` where V is within D (plus 2 v white for the
  three fp64 operations of the rounding itself) of a rounding tie k + 1/2 or of a clamp edge (0 or white).  Elsewhere the codes must
  be equal; at an ill pixel they may differ by one.  Condition: at most 1 % of every case's pixels are ill for the bound of its
  regime and kernel (asserted on the statement alone in tests/test_synth_ref_cpu.py).

  The fp32 exponential's allowance.  The accuracy of the hardware's exp2 is not documented here, so the allowance is, as
  splat_cases.exp_allowance does it, twice the largest ulp distance of torch's fp32 exp2 on the CPU from float64, over every exp2
  argument the cases produce (measured once per process; tests/test_synth_ref_cpu.py holds the distance under one ulp and records
  what one build gave)."""
import math

import numpy as np
import torch

import conv_float_ref as R
import synth_cases as SC

U = 2.0 ** -24
V = 2.0 ** -53
LOG2E = 1.4426950408889634074
PHASE = 4.0                 # phase-weight sums, units of u S3
ARG32 = 3.01                # fp32 roundings of the exp2 argument, units of u |y|
DROP32 = -120.0             # exp2 argument below which a weight may be dropped (fp32-exp kernel)
DROP64 = -700.0             # exp argument below which a weight may be dropped (fp64-exp kernels)
EXP64_ULPS = 2.0
WEIGHT64 = 4.0              # fp64 roundings of a weight after the exponential, units of v
BLEND = 16.0                # units of v sum p |c|
ILL_CAP = 0.01


# ---- statement ----------------------------------------------------------------------------------------------------------------------
def layers(d, parity=0, replicate=False, drop_lo=False):
    """-> (d2, logits) in float64.  d: dict with dec1, enc1, w2, b2 (or d2) and w3, b3.  parity / replicate / drop_lo: mutants only
    (nearest-x2 index shifted; replicate padding; dec2's values cut to the 11 bits of their `hi` half)."""
    if "d2" in d:
        d2 = d["d2"].double()
    else:
        d2 = R.finish(R.conv(R.cat([d["dec1"], d["enc1"]], SC.SPEC2.up2, parity=parity), d["w2"].double(), 1, replicate), d["b2"], True, None, None)
    if drop_lo:
        d2 = R.split_activation(d2.float())[0]
    logits = R.finish(R.conv(R.cat([d2], SC.SPEC3.up2, parity=parity), d["w3"].double(), 1, replicate), d["b3"], False, None, None)
    return d2, logits


def t_weights(t, f64_one_minus=False, swapped=False):
    """[N,6,1,1] float64: (1 - t) formed in fp32 for even k, t for odd k.  f64_one_minus / swapped: mutants."""
    t = t.float().reshape(-1)
    w1 = t.double()
    w0 = (1.0 - t.double()) if f64_one_minus else (torch.tensor(1.0, dtype=torch.float32) - t).double()
    if swapped:
        w0, w1 = w1, w0
    return torch.stack([w0, w1] * 3, 1).view(-1, 6, 1, 1)


def stack(cands):
    return torch.stack([c.double() for c in cands], 1)          # [N,6,3,H,W]


def tail(logits, cands, t, T=SC.T_PARAM, **mut):
    """The tail alone, from given logits (any float dtype): -> out [N,3,H,W] float64."""
    occ = torch.softmax(logits.double() / T, dim=1)
    W = t_weights(t, **mut) * occ
    return (W.unsqueeze(2) * stack(cands)).sum(1) / W.sum(1, keepdim=True)


def literal(logits, cands, t, T=SC.T_PARAM):
    """fLDRnet.py:511-524 operation by operation, in float64: the divisor from the first four terms, the frame from three pairs, the
    divisor completed, the quotient."""
    occ = torch.softmax(logits.double() / T, dim=1)
    tv = t.float().view(-1, 1, 1, 1)
    one_minus, c = (1 - tv), [x.double() for x in cands]
    o = lambda k: occ[:, k, :].unsqueeze(1)
    divisor = one_minus * o(0) + tv * o(1) + one_minus * o(2) + tv * o(3)
    out = one_minus * o(0) * c[0] + tv * o(1) * c[1]
    out = out + (one_minus * o(2) * c[2] + tv * o(3) * c[3])
    out = out + (one_minus * o(4) * c[4] + tv * o(5) * c[5])
    divisor = divisor + (one_minus * o(4) + tv * o(5))
    return out / divisor


def rounded(out, Hc, Wc, white, half_up=False, x0=0):
    """The cropped rounded frame as int64.  half_up / x0: mutants (round half up; the crop offset by x0 columns)."""
    v = ((out[:, :, :Hc, x0:x0 + Wc].double() + 1.0) / 2.0).clamp(0.0, 1.0) * float(white)
    return (torch.floor(v + 0.5) if half_up else torch.from_numpy(np.rint(v.numpy()))).long()


def ill_pixels(out, bound, Hc, Wc, white):
    """Pixels of the cropped frame within the bound of a rounding tie or a clamp edge."""
    v = (out[:, :, :Hc, :Wc] + 1.0) / 2.0 * float(white)
    b = bound[:, :, :Hc, :Wc]
    D = b * float(white) / 2.0 + 2 * V * float(white)
    tie = ((v - torch.floor(v)) - 0.5).abs() <= D
    return (tie | (v.abs() <= D) | ((v - float(white)).abs() <= D)) & (b > 0)        # (bound 0: the same frame, the same rounding)


def rounded_agree(codes, out, bound, Hc, Wc, white):
    """codes (integers, the cropped frame) against the rounded statement: equal outside the ill pixels, within one code at them.
    -> (number of pixels that break this, fraction of ill pixels)."""
    ref = rounded(out, Hc, Wc, white)
    ill = ill_pixels(out, bound, Hc, Wc, white)
    diff = (codes.long().cpu() - ref).abs()
    wrong = ((diff > 0) & ~ill) | (diff > 1)
    return int(wrong.sum()), ill.double().mean().item()


# ---- bound --------------------------------------------------------------------------------------------------------------------------
def logit_error(d, d2, kernel):
    """E of the docstring for the generic regime.  kernel: "vec" (fldr_dec3_synth), "spk" (fldr_dec3_synth_spk), "dec23"."""
    T3 = R.Terms(SC.SPEC3, [d2], d["w3"], d["b3"])
    E = T3.bound("fp32" if kernel == "vec" else "split") + PHASE * U * T3.S
    if kernel == "dec23":
        T2 = R.Terms(SC.SPEC2, [d["dec1"], d["enc1"]], d["w2"], d["b2"])
        E = E + R.conv(R.cat([T2.bound("split", d2, packed_out=True)], SC.SPEC3.up2), d["w3"].double().abs(), 1)
    return E


def tail_bound(logits, cands, t, exp32, E=None, T=SC.T_PARAM, out32=False, exp_ulps=None):
    """-> (out, bound), float64 [N,3,H,W]: the statement's tail on `logits` and the bound of the docstring for a kernel whose own
    logits are within E (None: 0) of them.  exp32: the fp32-exp kernel (maximum over the candidates with w_k != 0), else an fp64-exp
    kernel (maximum over all six)."""
    l = logits.double()
    w = t_weights(t)
    live = (w > 0).expand_as(l)
    s = l / T
    m_all = s.max(1, keepdim=True).values
    m_live = torch.where(live, s, torch.full_like(s, -math.inf)).max(1, keepdim=True).values
    W = w * torch.exp(s - m_live)                                  # (zero-weight candidates: 0 * finite)
    W = torch.where(live, W, torch.zeros_like(W))
    p = W / W.sum(1, keepdim=True)
    c = stack(cands)
    out = (p.unsqueeze(2) * c).sum(1)
    if E is None:
        E = torch.zeros_like(l)
    Epix = E.max(1, keepdim=True).values
    eta = torch.expm1((E + Epix) / T)
    if exp32:
        if exp_ulps is None:
            exp_ulps = exp2_allowance()
        y = (s - m_live) * LOG2E
        eta = eta + ARG32 * U * math.log(2.0) * y.abs() + exp_ulps * 2.0 ** -23 + WEIGHT64 * V
        eta = torch.where(y - (E + Epix) * LOG2E / T < DROP32, torch.ones_like(eta), eta)
    else:
        x = s - m_all
        eta = eta + (2 * s.abs() + 2 * m_all.abs() + 2 * x.abs()) * V + (2 * EXP64_ULPS + WEIGHT64) * V
        eta = torch.where(x - (E + Epix) / T < DROP64, torch.ones_like(eta), eta)
    eta = torch.where(live, eta, torch.zeros_like(eta))
    spe = (p * eta).sum(1, keepdim=True)
    dev = (p.unsqueeze(2) * eta.unsqueeze(2) * (c - out.unsqueeze(1)).abs()).sum(1)
    lv = live.unsqueeze(2).expand_as(c)
    span = torch.where(lv, c, torch.full_like(c, -math.inf)).max(1).values - torch.where(lv, c, torch.full_like(c, math.inf)).min(1).values
    F = torch.where(spe < 1.0, dev / (1.0 - spe).clamp(min=1e-300), span)
    bound = torch.minimum(F, span) + BLEND * V * (p.unsqueeze(2) * c.abs()).sum(1)
    if out32:
        bound = bound + U * (out.abs() + bound) + 2.0 ** -149
    return out, bound


# ---- the fp32 exponential's allowance -----------------------------------------------------------------------------------------------
def exp2_arguments(logits, t, T=SC.T_PARAM):
    """The fp32 exp2 arguments the fused kernel forms on fp32 logits: (l - max over the candidates with w_k != 0) * sc2, in fp32, of the
    candidates with w_k != 0."""
    l = logits.float()
    live = (t_weights(t) > 0).expand_as(l)
    mx = torch.where(live, l, torch.full_like(l, -math.inf)).max(1, keepdim=True).values
    sc2 = torch.tensor((1.0 / T) * LOG2E, dtype=torch.float64).float()
    return ((l - mx) * sc2)[live]


def ulp_distance32(x64, got32):
    """Largest |got - x| in fp32 ulps of x (x > 0, normal)."""
    x = np.asarray(x64, dtype=np.float64)
    ulp = np.exp2(np.floor(np.log2(x)) - 23)
    return float((np.abs(np.asarray(got32, dtype=np.float64) - x) / ulp).max())


_exp = []


def exp2_distance():
    """The largest distance in ulps between torch's fp32 exp2 on the CPU and float64 2^y, over every exp2 argument of every case that
    gives a normal result (measured once per process, on the machine that runs the test)."""
    if not _exp:
        ys = torch.cat([exp2_arguments(reference(c)["logits"], reference(c)["d"]["t"]) for c in SC.CASES])
        ys = ys[ys >= -126.0]
        _exp.append(ulp_distance32(np.exp2(ys.double().numpy()), torch.exp2(ys).numpy()))
    return _exp[0]


def exp2_allowance():
    """Twice the measured distance, for another implementation of the same class on the device."""
    return 2 * exp2_distance()


# ---- the cases of tests/synth_cases.py, computed once per process and shared: read-only ----------------------------------------------
_cache = {}


def build(case, d):
    """-> dict(d, d2, logits, out: the float64 statement on the inputs d; E: {kernel: logit error or None})."""
    d2, logits = layers(d)
    r = dict(d=d, d2=d2, logits=logits, out=tail(logits, d["cands"], d["t"]), E={})
    for kernel in (("vec", "spk") if case.fam == "dec3" else ("dec23",)):
        r["E"][kernel] = logit_error(d, d2, kernel) if case.regime == "generic" else None
    return r


def reference(case):
    if case not in _cache:
        _cache[case] = build(case, SC.make(case))
    return _cache[case]
