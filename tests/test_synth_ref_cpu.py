"""The float64 statement and bound of tests/synth_float_ref.py, checked without a GPU on every case of tests/synth_cases.py:
  * the statement equals a literal transcription of fLDRnet.py:511-524 in float64 (to the 64 v of the two operation orders);
  * the exact regime is exact: fp32 torch convolutions in two channel orders and the emulated split operands (three products) give
    the statement's d2 and logits bit for bit, every magnitude sum stays below 2^24 units of its resolution, and more than a quarter
    of the dec2 values carry a non-zero `lo` half (so a kernel that drops it is caught: the mutant below);
  * an emulation of each kernel's arithmetic (fp32 convolutions; the fused kernel's fp32 exp2 tail with results below 2^-126 flushed
    to 0, the other kernels' fp64 exp tail) stays inside the bound on every case; the fused kernel's tail as it was before this
    suite (maximum over all six logits) is NOT finite on the (-85, +85) cases at t = 0 / t = 1, the statement is;
  * the comparison rejects eleven mutants, each on at least one case (most on every case they apply to);
  * at most 1 % of the pixels of every rounded form a GPU test runs are within the bound of a rounding tie or a clamp edge.

The fp32 exponential.  synth_float_ref.exp2_distance() measures torch's fp32 exp2 on the CPU against float64 over the 661 332 exp2
arguments of the cases that give a normal result: 0.8010 ulp on the x86-64 build this was written on, so an allowance of 1.6019 ulp
(test_exp2_allowance prints the figures).  The bound uses twice whatever the machine that runs the test measures, and this file holds
the distance under one ulp.  On an MI355X the fused kernel used 0.30 of its exact-regime bound: the hardware's exp2 is inside the
allowance."""
import math

import torch
import torch.nn.functional as F

import conv_float_ref as R
import synth_cases as SC
import synth_float_ref as SR

CASES = SC.CASES


def _ratio(err, bound):
    return (err / bound.clamp(min=1e-300)).max().item()


def _kernels(case):
    return ("vec", "spk", "tail") if case.fam == "dec3" else ("dec23",)


def _bound(case, kernel, out32=False, logits=None, E="case"):
    """The (statement, bound) a GPU test holds `kernel` to on the case."""
    r = SR.reference(case)
    if E == "case":
        E = r["E"].get(kernel)
    return SR.tail_bound(r["logits"] if logits is None else logits, r["d"]["cands"], r["d"]["t"], exp32=kernel == "dec23", E=E, out32=out32)


# ---- the case lists -------------------------------------------------------------------------------------------------------------------
def test_case_lists_cover_what_they_claim():
    assert CASES == SC._cases() and len(set(CASES)) == len(CASES)
    for fam, shapes in (("dec3", SC.DEC3_SHAPES), ("dec23", SC.DEC23_SHAPES)):
        mine = SC.cases(fam)
        assert {(c.h, c.w) for c in mine} == {(h, w) for _, h, w in shapes}
        assert {c.regime for c in mine} == {"exact", "bias", "generic"}
        assert {c.pattern for c in mine if c.regime == "bias"} == set(SC.BIAS_PATTERNS)
        assert {c.pattern for c in mine if c.regime == "generic"} == set(SC.GENERIC_PATTERNS) or fam == "dec23"
        assert {c.cand for c in mine} == set(SC.CAND_KINDS)
        assert any(c.pattern == "stripes" for c in mine)
        assert sum(1 for _, h, w in shapes if any(c.N == 3 and (c.h, c.w) == (h, w) for c in mine)) == 1
        for regime in ("exact", "bias", "generic"):
            ts = torch.cat([SC.t_values(c) for c in mine if c.regime == regime]).double().tolist()
            want = SC.T_EDGE
            assert set(torch.tensor(want, dtype=torch.float64).float().double().tolist()) <= set(ts), (fam, regime)
    assert all(c.h % 2 == 0 and c.w % 2 == 0 for c in SC.cases("dec23"))
    assert {SC.GENERIC_PATTERNS[i % 6] for i in range(len(SC.DEC23_SHAPES))} == set(SC.GENERIC_PATTERNS)
    assert SC.Case("dec23", "exact", "dyadic", *SC.MULTI_TILE_DEC23, "uniform")[:6] in [c[:6] for c in CASES]
    one = torch.tensor(1.0, dtype=torch.float32)
    for t in SC.T_EDGE:
        tf = torch.tensor(t, dtype=torch.float64).float()
        assert (one - tf).double().item() == 1.0 - tf.double().item()
    for t in SC.T_ROUNDED:
        tf = torch.tensor(t, dtype=torch.float64).float()
        assert (one - tf).double().item() != 1.0 - tf.double().item()
    for case in CASES:
        a, b = SC.make(case), SC.make(case)
        for k in a:
            if isinstance(a[k], torch.Tensor):
                assert torch.equal(a[k], b[k]), (case, k)
        c = torch.stack(a["cands"])
        assert c.abs().max() <= 1.2 * (1 + 0.05) and (case.cand in ("near",) or c.abs().max() > 1.0 or c.numel() < 200)
        if case.cand == "equal":
            assert all(x is a["cands"][0] for x in a["cands"])
        if case.cand == "pair":
            assert a["cands"][4].data_ptr() == a["pair"].data_ptr() and not a["cands"][5].is_contiguous()
        if case.regime == "bias":
            assert not a["w3"].any()
    for case in CASES:
        if case.pattern.startswith("alt85"):
            r = SR.reference(case)
            lg, w = r["logits"], SR.t_weights(r["d"]["t"])
            live = torch.where((w > 0).expand_as(lg), lg, torch.full_like(lg, -math.inf)).amax(1)
            assert {float(v) for v in (lg.amax(1) - live).unique()} == {0.0, 170.0}, case


def test_no_case_reaches_the_fp16_range():
    worst = 0.0
    for case in CASES:
        r = SR.reference(case)
        d = r["d"]
        T3 = R.Terms(SC.SPEC3, [r["d2"]], d["w3"], d["b3"])
        m = max(T3.S.max().item(), r["d2"].abs().max().item())
        if case.fam == "dec23":
            m = max(m, R.Terms(SC.SPEC2, [d["dec1"], d["enc1"]], d["w2"], d["b2"]).S.max().item(), d["dec1"].abs().max().item(), d["enc1"].abs().max().item())
        worst = max(worst, m)
        assert m < 65504 / 2, (case, m)
        assert torch.isfinite(r["out"]).all(), case
    print("largest magnitude over the cases: %.3g" % worst)


# ---- the statement --------------------------------------------------------------------------------------------------------------------
def test_statement_is_the_literal_transcription():
    worst = 0.0
    for case in CASES:
        r = SR.reference(case)
        lit = SR.literal(r["logits"], r["d"]["cands"], r["d"]["t"])
        scale = SR.stack(r["d"]["cands"]).abs().amax(1)
        e = ((lit - r["out"]).abs() / scale.clamp(min=1e-300)).max().item() / SR.V
        worst = max(worst, e)
        assert e <= 64, (case, e)
        # and the two layers are what F.conv2d on F.interpolate gives (another summation order: 1e-13 of the largest value)
        same = lambda a, b: (a - b).abs().max().item() <= 1e-13 * max(1.0, b.abs().max().item())
        if case.fam == "dec23":
            x = torch.cat([F.interpolate(r["d"]["dec1"].double(), scale_factor=2, mode="nearest"), r["d"]["enc1"].double()], 1)
            assert same(F.relu(F.conv2d(x, r["d"]["w2"].double(), r["d"]["b2"].double(), padding=1)), r["d2"]), case
        lg = F.conv2d(F.interpolate(r["d2"], scale_factor=2, mode="nearest"), r["d"]["w3"].double(), r["d"]["b3"].double(), padding=1)
        assert same(lg, r["logits"]), case
    print("statement against the literal order: worst difference %.1f v (of the largest candidate)" % worst)


def test_equal_candidates_give_that_candidate():
    n, worst = 0, 0.0
    for case in CASES:
        if case.cand == "equal":
            r = SR.reference(case)
            c = r["d"]["cands"][0].double()
            q = ((r["out"] - c).abs() / (SR.V * c.abs())).max().item()
            worst = max(worst, q)
            assert q <= SR.BLEND, case                                           # (the float64 sums and the quotient round too)
            n += 1
    print("equal candidates: the statement is that candidate to %.1f v" % worst)
    assert n >= 4


# ---- the exact regime -----------------------------------------------------------------------------------------------------------------
def _fp32_layers(d, flip=False):
    """Both layers as fp32 torch convolutions (flip: the input channels in reverse order) -> fp32 (d2, logits)."""
    def conv(x, w, b):
        if flip:
            x, w = x.flip(1), w.flip(1)
        return F.conv2d(x.contiguous(), w.contiguous(), b, padding=1)
    if "d2" in d:
        d2 = d["d2"]
    else:
        d2 = F.relu(conv(torch.cat([F.interpolate(d["dec1"], scale_factor=2, mode="nearest"), d["enc1"]], 1), d["w2"], d["b2"]))
    return d2, conv(F.interpolate(d2, scale_factor=2, mode="nearest"), d["w3"], d["b3"])


def test_exact_regime_is_exact():
    lo_n = lo_all = 0
    big2 = big3 = 0.0
    for case in SC.cases(regime="exact"):
        r = SR.reference(case)
        d = r["d"]
        # the resolution of the products: dyadic 2^-10 2^-2 (dec2) and 2^-12 2^-8 (dec3); stripes 2^-10 1 and 2^-10 2^-1
        res2, res3 = (2.0 ** -12, 2.0 ** -20) if case.pattern == "dyadic" else (2.0 ** -10, 2.0 ** -11)
        for flip in (False, True):
            d2, lg = _fp32_layers(d, flip)
            assert torch.equal(d2.double(), r["d2"]) and torch.equal(lg.double(), r["logits"]), (case, flip)
        if case.fam == "dec23":
            assert torch.equal(R.emulated(SC.SPEC2, [d["dec1"], d["enc1"]], d["w2"], d["b2"]), r["d2"]), case
            S2 = R.Terms(SC.SPEC2, [d["dec1"], d["enc1"]], d["w2"], d["b2"]).S.max().item() / res2
            big2 = max(big2, S2)
            assert S2 < 2.0 ** 24, case
            for x in (d["dec1"], d["enc1"]):
                hi, lo = R.split_activation(x)
                assert torch.equal(hi, x.double()) and not lo.any(), case
            for w in (d["w2"], d["w3"]):
                hi, lo = R.split_weight(w, R.prepack_scale(w))
                assert not lo.any() and torch.equal(hi / R.prepack_scale(w), w.double()), case
        assert torch.equal(R.emulated(SC.SPEC3, [r["d2"].float()], d["w3"], d["b3"]), r["logits"]), case
        hi, lo = R.split_activation(r["d2"].float())
        assert torch.equal(hi + lo, r["d2"]), case                                        # the split holds every dec2 value
        S3 = R.Terms(SC.SPEC3, [r["d2"]], d["w3"], d["b3"]).S.max().item() / res3
        big3 = max(big3, S3)
        assert S3 < 2.0 ** 24, case
        if case.pattern == "dyadic":
            assert r["logits"].abs().max() < 4.0, case
            lo_n, lo_all = lo_n + int((lo != 0).sum()), lo_all + lo.numel()
        else:
            top = r["logits"].amax(1)
            second = r["logits"].topk(2, dim=1).values[:, 1]
            assert ((top == 32.0) & (second == 0.0)).all() and set(r["logits"].argmax(1).unique().tolist()) == set(range(min(6, case.w))), case
    print("exact regime: largest magnitude sums 2^%.1f (dec2) and 2^%.1f (dec3) units; %.1f %% of the dec2 values have a non-zero lo" % (
        math.log2(big2), math.log2(big3), 100.0 * lo_n / lo_all))
    assert lo_n >= 0.25 * lo_all


# ---- the fp32 exponential's allowance --------------------------------------------------------------------------------------------------
def test_exp2_allowance():
    d = SR.exp2_distance()
    n = sum(int(SR.exp2_arguments(SR.reference(c)["logits"], SR.reference(c)["d"]["t"]).numel()) for c in CASES)
    print("torch fp32 exp2 on this CPU against float64 over %d arguments: %.4f ulp; allowance %.4f ulp" % (n, d, SR.exp2_allowance()))
    assert 0.0 < d < 1.0 and SR.exp2_allowance() == 2 * d


# ---- emulations of the kernels' arithmetic -------------------------------------------------------------------------------------------
def _emul_exp32(logits32, cands, t, live_max=True, T=SC.T_PARAM):
    """fldr_dec23_synth's tail: the maximum on the fp32 logits (live_max: over the candidates with a non-zero t weight, as the kernel
    takes it at t = 0 and t = 1; False: over all six, as it was), exp2((l - max) * sc2) in fp32 with results below 2^-126 flushed to
    0, everything after in fp64: an fma-free chain, the reciprocal of the divisor."""
    l = logits32.float()
    w = SR.t_weights(t)
    if live_max:
        l = torch.where((w > 0).expand_as(l), l, torch.full_like(l, -math.inf))
    mx = l.max(1, keepdim=True).values
    sc2 = torch.tensor((1.0 / T) * SR.LOG2E, dtype=torch.float64).float()
    e = torch.exp2((l - mx) * sc2)
    e = torch.where(e < 2.0 ** -126, torch.zeros_like(e), e)
    wo = w * e.double()
    c = SR.stack(cands)
    o = wo[:, 0:1] * c[:, 0]
    for k in range(1, 6):
        o = o + wo[:, k:k + 1] * c[:, k]
    div = ((wo[:, 0:1] + wo[:, 1:2]) + wo[:, 2:3]) + wo[:, 3:4]
    div = div + (wo[:, 4:5] + wo[:, 5:6])
    return o * (1.0 / div)


def _emul_exp64(logits32, cands, t, T=SC.T_PARAM):
    """dec3_synth_kernel's tail (fldr_synth_tail's differs by divisions in place of reciprocals)."""
    s = logits32.float().double() * (1.0 / T)
    e = torch.exp(s - s.max(1, keepdim=True).values)
    wo = SR.t_weights(t) * (e * (1.0 / e.sum(1, keepdim=True)))
    c = SR.stack(cands)
    v = [wo[:, k:k + 1] * c[:, k] for k in range(6)]
    o = (v[0] + v[1]) + (v[2] + v[3])
    o = o + (v[4] + v[5])
    div = ((wo[:, 0:1] + wo[:, 1:2]) + wo[:, 2:3]) + wo[:, 3:4]
    div = div + (wo[:, 4:5] + wo[:, 5:6])
    return o * (1.0 / div)


def test_emulated_kernels_within_the_bound():
    worst = {}
    for case in CASES:
        r = SR.reference(case)
        d = r["d"]
        d2, lg = _fp32_layers(d)
        if case.regime != "generic":
            assert torch.equal(lg.double(), r["logits"]), case                        # exact and bias-only: the logits bit for bit
        for kernel in _kernels(case):
            for out32 in (False, True):
                # (fldr_synth_tail is given the statement's logits, rounded to fp32, and held to the tail on those)
                lin = r["logits"].float() if kernel == "tail" else lg
                ref, bound = _bound(case, kernel, out32, logits=lin if kernel == "tail" else None)
                got = _emul_exp32(lin, d["cands"], d["t"]) if kernel == "dec23" else _emul_exp64(lin, d["cands"], d["t"])
                got = got.float().double() if out32 else got
                assert torch.isfinite(got).all(), (case, kernel)
                q = _ratio((got - ref).abs(), bound)
                key = (kernel, case.regime, "f32" if out32 else "f64")
                worst[key] = max(worst.get(key, 0.0), q)
                assert q <= 1.0, (case, kernel, out32, q)
    for key in sorted(worst):
        print("emulated %-5s %-7s %s: worst error / bound %.4f" % (key + (worst[key],)))
    bounds = {}
    for case in CASES:
        for kernel in _kernels(case):
            key = (kernel, case.regime)
            bounds[key] = max(bounds.get(key, 0.0), _bound(case, kernel)[1].max().item())
    for key in sorted(bounds):
        print("largest bound %-5s %-7s: %.3e" % (key + (bounds[key],)))
    assert all(v < 1e-12 for (k, rg), v in bounds.items() if k != "dec23" and rg != "generic")
    assert all(v < 1e-5 for (k, rg), v in bounds.items() if k == "dec23" and rg != "generic")


def test_maximum_over_all_six_logits_is_not_finite_at_t_0_and_1():
    """What the fused kernel's tail did before: the maximum over all six logits.  On the (-85, +85) cases the three candidates with a
    non-zero t weight are 170 below it, exp2 returns 0 for all of them and the quotient is 0 / 0; the statement is finite, and so is
    the tail that takes the maximum over those three."""
    n = 0
    for case in CASES:
        if case.fam == "dec23" and case.pattern.startswith("alt85"):
            r = SR.reference(case)
            d = r["d"]
            before = _emul_exp32(r["logits"], d["cands"], d["t"], live_max=False)
            bad = ~torch.isfinite(before).flatten(1).all(1)
            assert bad.tolist() == ([True, False] if case.pattern == "alt85a" else [False, True]), case
            assert torch.isfinite(_emul_exp32(r["logits"], d["cands"], d["t"])).all() and torch.isfinite(r["out"]).all()
            n += 1
    assert n >= 2


# ---- mutants --------------------------------------------------------------------------------------------------------------------------
def _mut_layers(**kw):
    return lambda case, r: SR.tail(SR.layers(r["d"], **kw)[1], r["d"]["cands"], r["d"]["t"])


def _mut_tail(**kw):
    return lambda case, r: SR.tail(r["logits"], r["d"]["cands"], r["d"]["t"], **kw)


def _mut_no45(case, r):
    occ = torch.softmax(r["logits"] / SC.T_PARAM, dim=1)
    W = SR.t_weights(r["d"]["t"]) * occ
    return (W.unsqueeze(2) * SR.stack(r["d"]["cands"])).sum(1) / W[:, :4].sum(1, keepdim=True)


def _mut_cands23(case, r):
    c = list(r["d"]["cands"])
    c[2], c[3] = c[3], c[2]
    return SR.tail(r["logits"], c, r["d"]["t"])


MUTANTS = [
    ("t weights swapped", _mut_tail(swapped=True), lambda c: True),
    ("1 - t formed in float64", _mut_tail(f64_one_minus=True), lambda c: c.regime != "generic"),
    ("T taken as 1", _mut_tail(T=1.0), lambda c: True),
    ("divisor without candidates 4 and 5", _mut_no45, lambda c: True),
    ("candidates 2 and 3 exchanged", _mut_cands23, lambda c: c.cand != "equal"),
    ("nearest-x2 parity shifted", _mut_layers(parity=1), lambda c: c.regime != "bias" and (c.h, c.w) != (1, 1)),
    ("replicate padding", _mut_layers(replicate=True), lambda c: c.regime != "bias"),
    ("dec2's lo dropped", _mut_layers(drop_lo=True), lambda c: c.regime == "exact"),
]


def test_every_mutant_leaves_the_bound():
    """Against the loosest bound a GPU test applies to the case: the fp32 output form of the kernel with the largest logit error."""
    for name, mutant, applies in MUTANTS:
        n = caught = 0
        for case in CASES:
            if not applies(case):
                continue
            r = SR.reference(case)
            ref, bound = _bound(case, "spk" if case.fam == "dec3" else "dec23", out32=True)
            q = _ratio((mutant(case, r) - ref).abs(), bound)
            n, caught = n + 1, caught + (q > 1.0)
        print("mutant `%s`: leaves the bound on %d of %d cases" % (name, caught, n))
        assert caught >= 1, name
        if name not in ("1 - t formed in float64", "dec2's lo dropped"):
            assert caught >= n // 2, (name, caught, n)


def test_rounding_mutants_are_rejected():
    """Half up instead of half to even: a tie is ill for any non-zero bound, so the two roundings can only be told apart where the
    bound is 0: the comparison is given a frame of exact ties (V = k + 1/2 for white levels 2, 6 and 1022; odd white levels have their
    only dyadic tie at out = 0, where both roundings agree) with a zero bound.  The crop offset by one column: on every dec23 case."""
    for white, outs in ((2, [-0.5, 0.5]), (6, [-0.5, 0.5]), (1022, [-0.5, 0.5])):
        frame = torch.tensor(outs, dtype=torch.float64).view(1, 1, 1, 2).expand(1, 3, 2, 2).contiguous()
        zero = torch.zeros_like(frame)
        assert SR.rounded_agree(SR.rounded(frame, 2, 2, white), frame, zero, 2, 2, white)[0] == 0
        assert SR.rounded_agree(SR.rounded(frame, 2, 2, white, half_up=True), frame, zero, 2, 2, white)[0] > 0, white
    n = 0
    for case in SC.cases("dec23"):
        if case.regime == "generic" or case.w < 3:
            continue
        r = SR.reference(case)
        ref, bound = _bound(case, "dec23")
        Hc, Wc = 2 * case.h, 2 * case.w - 2
        assert SR.rounded_agree(SR.rounded(ref, Hc, Wc, 255), ref, bound, Hc, Wc, 255)[0] == 0
        wrong = SR.rounded_agree(SR.rounded(ref, Hc, Wc, 255, x0=1), ref, bound, Hc, Wc, 255)[0]
        assert wrong > 0 or case.cand == "near", case
        n += wrong > 0
    assert n >= 10


# ---- the condition of the rounded forms -----------------------------------------------------------------------------------------------
def test_few_pixels_are_within_the_bound_of_a_tie_or_a_clamp_edge():
    worst = {}
    for case in SC.cases("dec23"):
        if case.regime == "generic":
            continue                    # (the chained bound is wider than a code: the rounded forms run in the other two regimes)
        ref, bound = _bound(case, "dec23")
        for white in SC.whites(case):
            Hc, Wc = SC.crops(case)[0]
            frac = SR.ill_pixels(ref, bound, Hc, Wc, white).double().mean().item()
            worst[white] = max(worst.get(white, 0.0), frac)
            assert frac <= SR.ILL_CAP, (case, white, frac)
    print("largest share of ill pixels per white level:", {k: "%.4f" % v for k, v in worst.items()})
    assert set(worst) == {255, 1023, 65535}
