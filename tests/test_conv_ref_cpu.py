"""The float64 statement and bound of tests/conv_float_ref.py, checked without a GPU on every case of tests/conv_cases.py:
  * fp32 torch (the reference of test_conv_matches_torch_fp32, composed as there) lies within the exact-kernel bound of the statement;
  * an emulation of the split operands (fldr_split_hl's truncation mask, the prepack's scaled nearest-fp16 halves) convolved with
    exact products and sums lies within the REPRESENTATION part of the bound alone, for the three-product and the one-product form;
    without the absolute terms it does not (the floor of the split below |x| = 0.25);
  * non-vacuity: six wrong convolutions (a dropped border tap, replicated padding, nearest-x2 parity, swapped sources, the residual
    before the ReLU, the neighbouring channel's bias) each leave the bound at one pixel or more of EVERY case they apply to, for the
    loosest bound a test of the three-product kernels uses; so a kernel with one of these faults fails tests/test_gpu_conv_ops.py;
  * no case can raise the range flag: the magnitude sum S, which bounds every input and output, stays below fp16's 65504."""
import torch
import torch.nn.functional as F

import conv_cases as CC
import conv_float_ref as R

CASES = CC.cases()


def _worst(err, bound):
    return (err / bound.clamp(min=1e-300)).max().item()


def test_case_lists_cover_what_they_claim():
    assert len(CC.MODEL) == 12 and len(CASES) == sum(len(CC.shapes_of(s)) for s in CC.SPECS)
    assert {sum(s.parts) for s in CC.GENERIC} >= {1, 3, 7, 26, 100} and {s.cout for s in CC.GENERIC} >= {1, 6, 16, 17, 48, 96}
    for spec in CC.SPECS:
        mine = [c for c in CASES if c.spec == spec]
        assert {c.kind for c in mine} == set(CC.KINDS) and {c.wkind for c in mine} == {"plain", "spike"}, spec.name
        assert all(c.H % 2 == 0 and c.W % 2 == 0 for c in mine) or not any(spec.up2)
    assert sorted({(c.H, c.W) for c in CASES if c.N == 3}) == [(9, 33), (10, 34), (17, 65)]
    assert any(any(s.up2) and s.up2[0] for s in CC.GENERIC) and any(len(s.up2) > 1 and s.up2[1] for s in CC.GENERIC)
    assert any(len(s.parts) > 1 and s.parts[-1] % 8 for s in CC.SPECS if s.stride == 1)


def test_no_case_reaches_the_fp16_range():
    worst = 0.0
    for case in CASES:
        d, ref, T = R.reference(case)
        m = max(T.S.max().item(), max(s.abs().max().item() for s in d["srcs"]))
        worst = max(worst, m)
        assert m < 65504 / 2 and ref.abs().max().item() <= T.S.max().item(), (case, m)
    print("largest magnitude sum S over the cases: %.3g" % worst)


def test_fp32_torch_within_the_exact_kernel_bound():
    worst = {}
    for case in CASES:
        s = case.spec
        d, ref, T = R.reference(case)
        full = torch.cat([F.interpolate(x, scale_factor=2, mode="nearest") if u else x for x, u in zip(d["srcs"], s.up2)], 1)
        got = F.conv2d(full, d["w"], d["b"], stride=s.stride, padding=1)
        got = F.relu(got) if s.relu else got
        got = got[:, :s.store] if s.store else got
        got = got + d["res"] if s.residual else got
        assert got.shape == ref.shape, case
        r = _worst((got.double() - ref).abs(), T.bound("fp32"))
        worst[case.kind] = max(worst.get(case.kind, 0.0), r)
        assert r <= 1.0, (case, r)
    print("fp32 torch, worst error / exact-kernel bound per data kind:", {k: round(v, 4) for k, v in worst.items()})


def test_emulated_split_operands_within_the_representation_bound():
    worst3, worst1, rel_only = {}, {}, {}
    for case in CASES:
        s = case.spec
        d, ref, T = R.reference(case)
        e3 = (R.emulated(s, d["srcs"], d["w"], d["b"], d["res"]) - ref).abs()
        r3 = _worst(e3, T.representation("split"))
        worst3[case.kind] = max(worst3.get(case.kind, 0.0), r3)
        rel_only[case.kind] = max(rel_only.get(case.kind, 0.0), _worst(e3, R.REP_SPLIT * R.U * T.S))
        assert r3 <= 1.0, (case, r3)
        if s.stride == 1:
            r1 = _worst((R.emulated(s, d["srcs"], d["w"], d["b"], d["res"], terms=1) - ref).abs(), T.representation("fp16"))
            worst1[case.kind] = max(worst1.get(case.kind, 0.0), r1)
            assert r1 <= 1.0, (case, r1)
    print("split operands, exact sums: worst error / representation bound per data kind: three products %s, one product %s; "
          "against the relative part alone: %s" % tuple({k: round(v, 3) for k, v in w.items()} for w in (worst3, worst1, rel_only)))
    assert rel_only["dark"] > 1.0, "the absolute terms are not needed on these cases: the `dark` kind does not reach the subnormal halves"


# ---- mutants ----------------------------------------------------------------------------------------------------------------------------
def _mut_tap(case, d):
    """One product dropped at a border pixel: of the input values of sample 0 on the frame's border ring, the largest one's product is
    missing in every output channel of one output pixel that reads it: through the centre tap of a 3x3, through tap 1 (even position)
    or 2 (odd position) of a 4x4 stride 2, i.e. output index position // 2."""
    s = case.spec
    x = R.cat(d["srcs"], s.up2)
    H, W = x.shape[2:]
    Ho, Wo = CC.out_size(case)
    ok = torch.zeros(H, W, dtype=torch.bool)
    ok[0], ok[:, 0], ok[H - 1], ok[:, W - 1] = True, True, True, True
    ok[s.stride * Ho:], ok[:, s.stride * Wo:] = False, False                # (an odd stride-2 input: the last row / column is read by tap 3 only)
    i = int((x[0].abs() * ok).flatten().argmax())
    c, iy, ix = i // (H * W), (i // W) % H, i % W
    ky, kx = (1, 1) if s.stride == 1 else (1 + iy % 2, 1 + ix % 2)
    y = R.conv(x, d["w"].double(), s.stride)
    y[0, :, iy // s.stride, ix // s.stride] -= d["w"][:, c, ky, kx].double() * x[0, c, iy, ix]
    return R.finish(y, d["b"], s.relu, d["res"], s.store)


def _mut_replicate(case, d):
    s = case.spec
    return R.finish(R.conv(R.cat(d["srcs"], s.up2), d["w"].double(), s.stride, replicate=True), d["b"], s.relu, d["res"], s.store)


def _mut_parity(case, d):
    s = case.spec
    return R.finish(R.conv(R.cat(d["srcs"], s.up2, parity=1), d["w"].double(), s.stride), d["b"], s.relu, d["res"], s.store)


def _mut_swap(case, d):
    s = case.spec
    order = [1, 0] + list(range(2, len(s.parts)))
    return R.finish(R.conv(R.cat(d["srcs"], s.up2, order=order), d["w"].double(), s.stride), d["b"], s.relu, d["res"], s.store)


def _mut_res_first(case, d):
    s = case.spec
    return R.finish(R.conv(R.cat(d["srcs"], s.up2), d["w"].double(), s.stride), d["b"], s.relu, d["res"], s.store, res_first=True)


def _mut_bias(case, d):
    s = case.spec
    return R.finish(R.conv(R.cat(d["srcs"], s.up2), d["w"].double(), s.stride), torch.roll(d["b"], -1), s.relu, d["res"], s.store)


MUTANTS = [
    ("border tap dropped", _mut_tap, lambda c: True),
    ("padding replicated", _mut_replicate, lambda c: True),
    ("nearest-x2 parity", _mut_parity, lambda c: any(c.spec.up2) and (c.H, c.W) != (2, 2)),     # (a 1 x 1 source has one index only)
    ("sources swapped", _mut_swap, lambda c: len(c.spec.parts) > 1),
    ("residual before ReLU", _mut_res_first, lambda c: c.spec.relu and c.spec.residual),
    ("bias of channel c + 1", _mut_bias, lambda c: c.spec.bias and c.spec.cout > 1),
]


def test_every_mutant_leaves_the_bound_on_every_case_it_applies_to():
    """Against the loosest bound the GPU tests apply to a three-product kernel: the split bound of a packed output."""
    for name, mutant, applies in MUTANTS:
        n, weakest = 0, float("inf")
        for case in CASES:
            if not applies(case):
                continue
            d, ref, T = R.reference(case)
            r = _worst((mutant(case, d) - ref).abs(), T.bound("split", ref, packed_out=True))
            assert r > 1.0, "mutant `%s` stays inside the bound on %s (worst error / bound %.3g): change the case's data" % (name, case, r)
            n, weakest = n + 1, min(weakest, r)
        assert n > 0, name
        print("mutant `%s`: %d cases, smallest worst-pixel error / bound %.3g" % (name, n, weakest))
