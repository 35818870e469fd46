"""The anchors of the backward-warp, splat-metric and resize tests, anchored themselves: oracle.bwarp (both mask forms) and fp32
F.interpolate against the float64 statement of the operations (tests/warp_float_ref.py: index arithmetic from the definitions, no
grid_sample, no interpolate) on every case of tests/warp_cases.py, the cases the GPU tests (tests/test_gpu_warp_ops.py) hold the
kernels to the oracle at.

The bound is derived, not tuned.  fp32 forms the sample position from numbers up to max(W, H) in a handful of roundings (add, scale,
divide, unnormalise: 8 eps32 max(W, H) px covers them), and a position error moves the interpolated value by at most the plane's
largest step between adjacent samples, D, per pixel; the four products and three sums of the taps add 4 eps32 R, R the plane's largest
magnitude:  bound = 8 eps32 max(W, H) D + 4 eps32 R.  The masked form is compared outside the positions whose mask value lies
within BWARP_BAND of the hard threshold (oracle.bwarp_mask_value): there fp32 and float64 may legitimately decide differently.
Measured on the CPU: the oracle stays at or under a ninth of the bound (1.3e-5 of 1.6e-4 at 9 x 83), fp32 F.interpolate under a
thirtieth (3.5e-5 of 1.2e-3 at the x4 case).

The same file asserts what keeps the GPU tests from being vacuous: the masked `aligned` cases keep at least half of their pixels
(with `zero` flows at H <= 2 or W = 1 the mask zeroes the whole frame), and in every masked case at most 1 % of the pixels are
ill-conditioned."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import warp_cases as WC
import warp_float_ref as R64

EPS32 = float(np.finfo(np.float32).eps)
BWARP_BAND = 1e-4                    # as tests/test_gpu_parity.py: |mask value - 0.999| below which the threshold is ill-conditioned
MIN_KEPT_ALIGNED = 0.5
MAX_ILL_SHARE = 0.01


def _steps(x):
    """(D, R) of planes [N,C,H,W]: the largest step between adjacent samples (0 along an axis of one sample) and the largest magnitude."""
    x = x.double()
    dx = (x[..., 1:] - x[..., :-1]).abs().max().item() if x.shape[3] > 1 else 0.0
    dy = (x[..., 1:, :] - x[..., :-1, :]).abs().max().item() if x.shape[2] > 1 else 0.0
    return max(dx, dy), x.abs().max().item()


def _bound(x, size, mul=1.0):
    D, R = _steps(x)
    return 8 * EPS32 * size * D * abs(mul) + 4 * EPS32 * R * abs(mul)


def _ill(oracle, shape, flo):
    return (oracle.bwarp_mask_value(shape, flo) - oracle.BWARP_MASK_THRESHOLD).abs() < BWARP_BAND


def _check_bwarp(oracle, x, flo, tag):
    """oracle.bwarp against the float64 statement, both mask forms -> (kept share, ill share)."""
    N, C, H, W = x.shape
    bound = _bound(x, max(W, H))
    ill = _ill(oracle, x.shape, flo)
    e_plain = (oracle.bwarp(x, flo, withmask=False).double() - torch.from_numpy(R64.bwarp(x.numpy(), flo.numpy(), False))).abs().max().item()
    err = (oracle.bwarp(x, flo, withmask=True).double() - torch.from_numpy(R64.bwarp(x.numpy(), flo.numpy(), True))).abs()
    well = ~ill.expand_as(err)
    e_mask = err[well].max().item() if well.any() else 0.0
    kept = float((R64.bwarp_mask_value(flo.numpy(), H, W) >= R64.MASK_THRESHOLD).mean())
    share = ill.float().mean().item()
    print("%-34s kept %5.1f %%  ill %d of %d  err plain %.2e masked %.2e  bound %.2e" % (tag, 100 * kept, int(ill.sum()), ill.numel(), e_plain, e_mask, bound))
    assert e_plain <= bound and e_mask <= bound, (tag, e_plain, e_mask, bound)
    assert share <= MAX_ILL_SHARE, (tag, share)
    return kept, share


@pytest.mark.parametrize("kind", WC.FLOW_KINDS)
def test_oracle_bwarp_matches_float64_statement(oracle, kind):
    """Unit-range planes, every shape, both mask forms; the `aligned` cases keep at least half of their pixels under the mask."""
    for shape in WC.SHAPES:
        flo, wild = WC.flow(kind, shape)
        kept, _ = _check_bwarp(oracle, WC.image(shape), flo, "bwarp %s %s" % (shape, kind))
        if kind == "aligned":
            assert kept >= MIN_KEPT_ALIGNED, (shape, kept)
        if kind == "wild":
            assert wild.any() or shape[2] * shape[3] < 3
            gone = wild.expand(shape)
            for m in (False, True):
                assert (oracle.bwarp(WC.image(shape), flo, withmask=m)[gone] == 0).all() and (R64.bwarp(WC.image(shape).numpy(), flo.numpy(), m)[gone.numpy()] == 0).all()


@pytest.mark.parametrize("kind", ["aligned", "noise14", "wild"])
def test_oracle_bwarp_of_scaled_flow_planes_matches_float64_statement(oracle, kind):
    """The inputs of the fldr_bwarp_tscaled test: +-7 px planes warped by t-scaled flows, the products formed in fp32."""
    for k, shape in enumerate(WC.SHAPES):
        flo, _ = WC.flow(kind, shape)
        t = WC.t_values(k, shape[0])
        x = WC.flow_planes(shape)
        for xm in WC.T_MODES:
            for fm in WC.T_MODES:
                _check_bwarp(oracle, WC.scaled(x, xm, t), WC.scaled(flo, fm, t), "tscaled %s %s x*%s f*%s" % (shape, kind, xm, fm))


@pytest.mark.parametrize("kind", ["zero", "aligned", "noise14"])
def test_splat_metric_of_the_oracle_matches_float64_statement(oracle, kind):
    """mean_c(alpha |I - bwarp(other, flow)|) from oracle.bwarp, as the model forms it, against the float64 statement: |alpha| times the
    warp's bound plus the rounding of the difference, the product and the mean (C + 2 roundings of at most |alpha| 2 R)."""
    alpha = -1.894
    for shape in WC.SHAPES:
        flo, _ = WC.flow(kind, shape)
        I, other = WC.image(shape, 1), WC.image(shape, 2)
        ref = torch.from_numpy(R64.zmetric(I.numpy(), other.numpy(), flo.numpy(), alpha))
        got = torch.mean(alpha * torch.abs(I - oracle.bwarp(other, flo)), dim=1, keepdim=True).double()
        ill = _ill(oracle, shape, flo)
        bound = abs(alpha) * (_bound(other, max(shape[2], shape[3])) + (shape[1] + 2) * EPS32 * 2.0)
        err = (got - ref).abs()
        e = err[~ill].max().item() if (~ill).any() else 0.0
        print("zmetric %s %s: ill %d of %d  err %.2e  bound %.2e" % (shape, kind, int(ill.sum()), ill.numel(), e, bound))
        assert e <= bound, (shape, kind, e, bound)


def test_torch_resize_matches_float64_statement():
    """fp32 F.interpolate(bilinear, align_corners=False) * mul against the float64 statement on every resize case; D and R are those of the
    source times mul, the size that of the source.  The same-size case is exact."""
    for case in WC.RESIZE_CASES:
        h, w, H, W, mul = case
        for nc in WC.RESIZE_NC:
            x = WC.resize_source(case, nc)
            got = F.interpolate(x, size=(H, W), mode="bilinear", align_corners=False) * mul
            ref = torch.from_numpy(R64.resize_bilinear(x.numpy(), H, W, mul))
            assert got.shape == ref.shape
            bound = _bound(x, max(w, h), mul)
            e = (got.double() - ref).abs().max().item()
            print("resize %sx%s -> %sx%s mul %s N C %s: err %.2e  bound %.2e" % (h, w, H, W, mul, nc, e, bound))
            assert e <= bound, (case, nc, e, bound)
            if (h, w) == (H, W):
                assert torch.equal(ref.float(), x * mul) and torch.equal(got, x * mul)


def test_case_generators_are_seeded_and_as_described():
    for shape in WC.SHAPES:
        N, C, H, W = shape
        assert H <= 45 and W <= 83
        for kind in WC.FLOW_KINDS:
            a, wa = WC.flow(kind, shape)
            b, wb = WC.flow(kind, shape)
            assert torch.equal(a, b) and torch.equal(wa, wb) and a.shape == (N, 2, H, W) and a.dtype == torch.float32
            assert torch.isfinite(a).all() and a.abs().max().item() <= WC.WILD
        f, wild = WC.flow("wild", shape)
        assert torch.equal((f.abs() == WC.WILD).any(1, keepdim=True), wild)
        assert (WC.flow("noise14", shape)[0].abs() <= 7).all() and (WC.flow("noise2", shape)[0].abs() <= 1).all()
        # aligned: the float64 position of pixel i is sample i, up to the +-0.4 px of the axes that carry noise (times S / (S - 1))
        f, _ = WC.flow("aligned", shape)
        sx, sy = R64._positions(f.numpy(), H, W)
        for s, S, idx in ((sx, W, np.arange(W)[None, None, :]), (sy, H, np.arange(H)[None, :, None])):
            slack = WC.ALIGNED_NOISE * S / (S - 1) if S >= 3 else 1e-6
            assert np.abs(s - idx).max() <= slack + 1e-6, (shape, S)
    ts = set()
    for k, shape in enumerate(WC.SHAPES):
        ts |= set(WC.t_values(k, shape[0]).flatten().tolist())
    assert ts == set(torch.tensor(WC.T_VALUES).tolist())
