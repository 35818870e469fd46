"""The unfused level-0 group alone, at the shapes where a sampling kernel goes wrong: fldr_bwarp, fldr_bwarp_tscaled, fldr_zmetric,
fldr_resize_bilinear and fldr_resize_bilinear_spk against the CPU oracle on every case of tests/warp_cases.py: one row, one column,
2 x 2, widths either side of the 64-pixel tile and heights either side of its 4 rows, a second sample, with and without the mask, flows
that land on the samples, noise, and flows 1e9 px out of the frame; resizes that shrink, keep the size or start from one row or
column.  The fused fldr_level0_prep and tools/stress_shapes.py are compared with THESE kernels bit for bit, and share their tap
arithmetic (csrc/common.h), so nothing else in the suite sees a fault the two have in common.  The oracle itself is held to a float64
statement of the operations on the same cases by tests/test_warp_ref_cpu.py, which also asserts that the masked cases below are not
vacuous (the `aligned` flows keep at least half of the pixels) and carry at most 1 % ill-conditioned pixels.

Tolerances are those of test_bwarp_matches_reference_golden / test_bwarp_tscaled_zmetric_resize (the shapes are no larger than
theirs): 1e-5 on unit-range planes, 4e-5 on +-7 px flow planes, differences beyond them only where the oracle's mask value lies
within BWARP_BAND of the hard threshold.  Every test prints one line per case."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import warp_cases as WC
import warp_float_ref as R64
from test_gpu_parity import BWARP_BAND, _bwarp_ill, _cmp, hip  # noqa: F401  (hip: the module-scoped library fixture)

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)


def _kept(oracle, shape, flo):
    return (oracle.bwarp_mask_value(shape, flo) >= oracle.BWARP_MASK_THRESHOLD).float().mean().item()


@pytest.mark.parametrize("kind", WC.FLOW_KINDS)
def test_bwarp_every_shape_and_mask_form_vs_oracle(hip, oracle, dev, kind):
    for shape in WC.SHAPES:
        x = WC.image(shape)
        flo, wild = WC.flow(kind, shape)
        ill = _bwarp_ill(oracle, shape, flo)
        for mask in (True, False):
            got = hip.bwarp(x.to(dev), flo.to(dev), mask)
            what = "bwarp %s %s mask %d" % (shape, kind, mask)
            e = _cmp(got, oracle.bwarp(x, flo, withmask=mask), atol=1e-5, ill=ill if mask else None, what=what)
            print("%s: kept %5.1f %%  ill %d of %d  max err %.2e" % (what, 100 * _kept(oracle, shape, flo), int(ill.sum()), ill.numel(), e))
            if kind == "wild":
                assert (got.cpu()[wild.expand(shape)] == 0).all(), what + ": a pixel 1e9 px out of the frame is not exactly 0"


@pytest.mark.parametrize("kind", ["aligned", "noise14", "wild"])
def test_bwarp_tscaled_all_nine_scale_pairs_vs_oracle(hip, oracle, dev, kind):
    """bwarp(sx x, sf flo) for sx, sf in {1, t, 1 - t} per sample, the products formed in fp32 as scaling the tensors first would
    (the x-scale path is a sampling loop of its own in bwarp_kernel); without scales bit-identical to fldr_bwarp."""
    for k, shape in enumerate(WC.SHAPES):
        x = WC.flow_planes(shape)
        flo, _ = WC.flow(kind, shape)
        t = WC.t_values(k, shape[0])
        xd, fd, td = x.to(dev), flo.to(dev), t.to(dev)
        for fm in WC.T_MODES:
            sflo = WC.scaled(flo, fm, t)
            ill = _bwarp_ill(oracle, shape, sflo)
            kept = _kept(oracle, shape, sflo)
            for xm in WC.T_MODES:
                for mask in (True, False):
                    got = hip.bwarp_tscaled(xd, fd, td, xm, fm, withmask=mask)
                    what = "bwarp_tscaled %s %s t %s x*%s flo*%s mask %d" % (shape, kind, [round(v, 3) for v in t.flatten().tolist()], xm, fm, mask)
                    e = _cmp(got, oracle.bwarp(WC.scaled(x, xm, t), sflo, withmask=mask), atol=4e-5, ill=ill if mask else None, what=what)
                    print("%s: kept %5.1f %%  ill %d of %d  max err %.2e" % (what, 100 * kept, int(ill.sum()), ill.numel(), e))
                    if xm is None and fm is None:
                        assert torch.equal(got, hip.bwarp(xd, fd, mask)), what + ": differs from fldr_bwarp"


@pytest.mark.parametrize("kind", ["zero", "aligned", "noise14"])
def test_zmetric_every_shape_vs_oracle(hip, oracle, dev, kind):
    alpha = -1.894
    for shape in WC.SHAPES:
        I, other = WC.image(shape, 1), WC.image(shape, 2)
        flo, _ = WC.flow(kind, shape)
        ill = _bwarp_ill(oracle, shape, flo)
        zref = torch.mean(alpha * torch.abs(I - oracle.bwarp(other, flo)), dim=1, keepdim=True)
        what = "zmetric %s %s" % (shape, kind)
        e = _cmp(hip.zmetric(I.to(dev), other.to(dev), flo.to(dev), alpha), zref, atol=1e-5, ill=ill, what=what)
        print("%s: kept %5.1f %%  ill %d of %d  max err %.2e" % (what, 100 * _kept(oracle, shape, flo), int(ill.sum()), ill.numel(), e))


def test_resize_bilinear_vs_float64_statement(hip, dev):
    """Against the float64 statement (tests/warp_float_ref.py), within max(2 E32, 2 eps32 |mul| max|in|): E32 is the distance of fp32
    CPU F.interpolate * mul from the same statement on the same input (the kernel and the CPU round independently by the same
    amount, hence the 2); the floor covers the cases where the CPU happens to be exact.  The same-size case is bit-equal to in * mul."""
    for case in WC.RESIZE_CASES:
        h, w, H, W, mul = case
        for nc in WC.RESIZE_NC:
            x = WC.resize_source(case, nc)
            ref = torch.from_numpy(R64.resize_bilinear(x.numpy(), H, W, mul))
            cpu = F.interpolate(x, size=(H, W), mode="bilinear", align_corners=False) * mul
            e32 = (cpu.double() - ref).abs().max().item()
            bound = max(2 * e32, 2 * EPS32 * abs(mul) * x.abs().max().item())
            got = hip.resize_bilinear(x.to(dev), H, W, mul=mul).cpu()
            assert got.shape == ref.shape and torch.isfinite(got).all()
            e64, ecpu = (got.double() - ref).abs().max().item(), (got - cpu).abs().max().item()
            print("resize %dx%d -> %dx%d mul %s N C %s: E32 %.2e  kernel to float64 %.2e (bound %.2e)  kernel to fp32 torch %.2e" % (h, w, H, W, mul, nc, e32, e64, bound, ecpu))
            assert e64 <= bound, (case, nc, e64, bound)
            if (h, w) == (H, W):
                assert torch.equal(got, x * mul), (case, nc)


def test_resize_bilinear_spk_bit_identical_and_packed_twin(hip, dev):
    """The C <= 8 resize that also writes its split-packed twin: the fp32 output is fldr_resize_bilinear's bit for bit, the twin is the
    split of that output, padding channels of the group included (zeros, never uninitialised memory); no range flag is raised."""
    hip.check_range()
    for case in WC.RESIZE_CASES:
        h, w, H, W, mul = case
        for nc in WC.RESIZE_NC + [(1, 8)]:
            x = WC.resize_source(case, nc).to(dev)
            out, sp = hip.resize_bilinear_spk(x, H, W, mul=mul)
            assert torch.equal(out, hip.resize_bilinear(x, H, W, mul=mul)), (case, nc)
            assert torch.equal(hip.spk_pack(out).buf, sp.buf), (case, nc)
            print("resize_spk %dx%d -> %dx%d mul %s N C %s: fp32 and packed twin bit-identical" % (h, w, H, W, mul, nc))
    hip.check_range()
