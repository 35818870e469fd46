"""The anchor of the forward-splat tests, anchored itself: oracle.function_softsplat and oracle.splat_forward against the float64
statement of the operation (tests/splat_float_ref.py: plain numpy from the definition) on every case of tests/splat_cases.py, the
cases tests/test_gpu_splat_ops.py holds fldr_softsplat_acc64 to the same statement at.

The bound is derived, not tuned (splat_float_ref.py): the roundings of the fp32 products, the casts of the two fp64 sums, a quotient
within one ulp and the post-scale.  Its one measured ingredient is exp: the largest distance between torch's fp32 exp (the oracle's,
and so the reference's) and float64 exp over every metric value of the cases, in ulps.  Measured here: 0.5521 ulp over 1 644 756
values between -30 and 85; the allowance for another IEEE-class implementation on the device is twice that, 1.1042 ulp.  Measured
with it, largest share of the bound over the cases (printed per case): softmax 0.499, linear 0.962, average and summation 1.000 —
without a metric the bound is a handful of roundings, and the post-scale of a value just above a power of two attains its term.

The same file asserts what keeps the GPU tests from being vacuous: by the search model on the exact bounds every walk of the kernel
is reached (whole map, nothing, rectangle, block queue, rectangle by queue overflow, whole map by super-block overflow), no product of
any case lies below 2^-100, the `beyond` cases and only they have normalisers outside [2^-100, 2^100], every `graze` and `edge` case
has cells reached only by weights below 1e-4, and every case but `gone` and `collapse` (one footprint by definition) reaches at least
a tenth of its cells.  And it holds the comparison itself to account: the statement with one fault at a time, seven mutants, must be
rejected by the comparison the GPU test uses on at least one case each."""
import numpy as np
import pytest
import torch

import splat_cases as SC
import splat_float_ref as R64

MIN_REACHED = 0.1
SMALL_WEIGHT = 1e-4
LOW, HIGH = 2.0 ** -100, 2.0 ** 100

_cache = {}


def _statement(case, mode, k=0):
    key = (case, mode, k)
    if key not in _cache:
        img, flo, m = SC.problem(case, mode, k)
        args = (img.numpy(), flo.numpy(), None if m is None else m.numpy(), mode)
        _cache[key] = R64.splat(*args) + (R64.bound(*args, SC.exp_allowance()),)
    return _cache[key]


def _model(case, k=0):
    key = (case, "model", k)
    if key not in _cache:
        blk, sbt = R64.block_bounds(SC.flow(case, k).numpy())
        _cache[key] = R64.search_model(blk, sbt, case.H, case.W, *SC.tile_geometry(case))
    return _cache[key]


def test_exp_distance_measured_and_allowance():
    """torch's fp32 exp over the metric values of every case against float64 exp: the measured distance (printed) is that of an
    IEEE-class implementation, under one ulp, and the allowance of the bound is twice it."""
    d = SC.exp_distance()
    print("fp32 exp over %d metric values: %.4f ulp from float64 exp; allowance %.4f ulp" % (SC.all_metric_values().numel(), d, SC.exp_allowance()))
    assert 0.0 < d <= 1.0 and SC.exp_allowance() == 2 * d


@pytest.mark.parametrize("mode", SC.MODES)
@pytest.mark.parametrize("config", ["image", "feature"])
def test_oracle_matches_float64_statement(oracle, config, mode):
    """function_softsplat within the bound of the statement on every case, holes exact; splat_forward's empty cells are the statement's."""
    worst = 0.0
    for case in SC.CASES:
        if case.config != config:
            continue
        img, flo, m = SC.problem(case, mode)
        ref, norm, bnd = _statement(case, mode)
        got = oracle.function_softsplat(img, flo, m, mode).double().numpy()
        share = R64.share_of_bound(got, ref, bnd)
        worst = max(worst, share)
        print("%-44s %-9s err %.2e  bound %.2e  share %.3f  holes %d of %d" % (SC.case_id(case), mode, np.abs(got - ref).max(), bnd.max(), share,
                                                                              int((norm == 0).sum()), norm.size))
        assert R64.violations(got, ref, norm, bnd) == [], (SC.case_id(case), mode)
        if mode == "summation":                         # the raw operator's hole set: once per case
            ones = torch.ones(case.N, 1, case.H, case.W)
            assert np.array_equal(oracle.splat_forward(ones, flo).numpy() == 0, norm == 0), SC.case_id(case)
            assert np.array_equal(R64.reach(flo.numpy()) == -1.0, norm == 0)
    print("%s %s: largest share of the bound %.3f" % (config, mode, worst))


def test_search_model_reaches_every_walk():
    """By the restated search on the exact bounds: which case takes which walk (printed), every walk is taken, and the overflow and
    super-block shapes take the branch they were chosen for under `wild` and the normal path under `smooth`."""
    seen = set()
    for case in SC.CASES:
        model = _model(case)
        walks = R64.walks_of(model)
        seen |= walks
        cols = [c for n in model for c in n]
        print("%-44s columns %4d  super-blocks matched <= %3d  blocks matched <= %3d  walks %s" % (
            SC.case_id(case), len(cols), max(c["n_sb"] for c in cols), max(c["n_match"] for c in cols), " ".join(sorted(walks))))
        nsb = int(np.prod(R64.table_geometry(case.H, case.W)))
        if case.H * case.W <= R64.WHOLE_PIXELS:
            assert walks == {"whole"}, SC.case_id(case)
        if (case.H, case.W) in SC.OVERFLOW_IMAGE or (case.H, case.W) == (1040, 65):
            assert nsb == 17 and 520 > R64.Q_BLOCKS
            if case.flow == "wild":
                assert all(c["n_match"] > R64.Q_BLOCKS for c in cols) and walks == {"rect_overflow"}, SC.case_id(case)
            else:
                assert all(0 < c["n_match"] <= R64.Q_BLOCKS for c in cols) and walks <= {"rect", "queue"}, SC.case_id(case)
        if (case.H, case.W) in SC.SUPER_IMAGE:
            assert nsb == 65 > R64.Q_SUPER and 1 in R64.table_geometry(case.H, case.W)
            if case.flow == "wild":
                assert all(c["n_sb"] > R64.Q_SUPER for c in cols) and walks == {"whole_sb_overflow"}, SC.case_id(case)
            else:
                assert all(0 < c["n_sb"] <= R64.Q_SUPER for c in cols) and walks <= {"rect", "queue"}, SC.case_id(case)
    assert seen == set(R64.WALKS), sorted(set(R64.WALKS) - seen)
    # the other route of the threshold shapes: (36, 64) through tables, (37, 64) through the whole-map walk
    for case in SC.CASES:
        if (case.H, case.W) == (36, 64):
            blk, sbt = R64.block_bounds(SC.flow(case).numpy())
            forced = R64.walks_of(R64.search_model(blk, sbt, 36, 64, *SC.tile_geometry(case), whole=False))
            assert forced and "whole" not in forced, SC.case_id(case)


def test_cases_are_not_vacuous():
    """Products, normalisers, grazing weights and reach of every case and problem, in the modes that form them."""
    for case in SC.CASES:
        for k in range(2):
            flo = SC.flow(case, k).numpy()
            reached = float((R64.reach(flo) == 1.0).mean())
            if case.flow == "gone":
                assert reached == 0.0, SC.case_id(case)
            elif case.flow == "collapse":
                assert 0.0 < reached * case.H * case.W <= 4 * case.N, SC.case_id(case)
            else:
                assert reached >= MIN_REACHED, (SC.case_id(case), k, reached)
            if case.flow in ("graze", "edge"):
                best = R64.max_weight(flo)
                grazed = int(((best > 0) & (best < SMALL_WEIGHT)).sum())
                assert grazed > 0, (SC.case_id(case), k)
            else:
                grazed = -1
            lows = []
            for mode in ("linear", "softmax"):
                img, _, m = SC.problem(case, mode, k)
                mm = None if m is None else m.numpy()
                lows.append(R64.smallest_product(img.numpy(), flo, mm, mode))
                assert lows[-1] >= LOW, (SC.case_id(case), mode, k, lows[-1])
                _, norm = R64.splat(img.numpy(), flo, mm, mode)
                live = norm[norm != 0]
                if case.metric == "beyond":
                    assert live.size and (live > HIGH).all(), (SC.case_id(case), mode, k)
                else:
                    assert ((live >= LOW) & (live <= HIGH)).all(), (SC.case_id(case), mode, k, live.min(), live.max())
            if k == 0:
                print("%-44s reached %5.1f %%  cells grazed only %4d  smallest product 2^%.0f" % (SC.case_id(case), 100 * reached, grazed, np.log2(min(lows))))


# fault -> (flow kinds, modes) of the cases it is looked for on
_MUTANT_CASES = {"east_tile": (("graze", "edge", "random", "wild"), ("softmax",)), "column_w": (("edge",), ("average",)),
                 "trunc": (("edge",), ("average",)), "tiny": (("graze",), ("softmax",)), "norm_floor": (("graze",), ("average", "softmax")),
                 "queue_512": (("wild",), ("average",)), "nw_left": (("graze", "edge", "random", "wild"), ("softmax",))}


@pytest.mark.parametrize("fault", R64.FAULTS)
def test_the_comparison_rejects_the_mutant(fault):
    """The statement with one fault, rounded to fp32 as a kernel's output is, fails the comparison of the GPU test on at least one
    case (and the unmutated statement passes it on that case)."""
    kinds, modes = _MUTANT_CASES[fault]
    rejected = []
    for case in SC.CASES:
        if case.flow not in kinds or (fault == "queue_512" and (case.config, case.H, case.W) != ("image", 1040, 65)):
            continue
        for mode in modes:
            img, flo, m = SC.problem(case, mode)
            ref, norm, bnd = _statement(case, mode)
            out, _ = R64.splat(img.numpy(), flo.numpy(), None if m is None else m.numpy(), mode, fault=fault, geom=SC.tile_geometry(case))
            found = R64.violations(out.astype(np.float32), ref, norm, bnd)
            assert R64.violations(ref.astype(np.float32), ref, norm, bnd) == []
            if found:
                rejected.append(SC.case_id(case))
                print("%-12s rejected on %-44s %-9s: %s" % (fault, SC.case_id(case), mode, "; ".join(found)))
    assert rejected, fault


def test_block_bounds_layout_and_search_geometry():
    """block_bounds against a loop over the blocks of a ragged map; dead entries exactly outside the map; super-blocks are unions."""
    flo = SC.flow(SC.Case("image", 2, 1, 70, 300, "random", None)).numpy()
    blk, sbt = R64.block_bounds(flo)
    nsb_x, nsb_y = R64.table_geometry(70, 300)
    assert (nsb_x, nsb_y) == (2, 2) and blk.shape == (2, 4, 64, 4) and sbt.shape == (2, 4, 4)
    for n in range(2):
        for s in range(4):
            for b in range(64):
                x0, y0 = ((s % nsb_x) * 4 + b % 4) * 64, ((s // nsb_x) * 16 + b // 4) * 4
                px = flo[n, :, y0:y0 + 4, x0:x0 + 64]
                if px.size == 0:
                    assert np.array_equal(blk[n, s, b], np.array([np.inf, -np.inf, np.inf, -np.inf], np.float32))
                else:
                    assert np.array_equal(blk[n, s, b], np.array([px[0].min(), px[0].max(), px[1].min(), px[1].max()], np.float32))
            assert np.array_equal(sbt[n, s], np.array([blk[n, s, :, 0].min(), blk[n, s, :, 1].max(), blk[n, s, :, 2].min(), blk[n, s, :, 3].max()]))
    ws = R64.table_workspace(blk, sbt)
    b2, s2 = R64.split_workspace(ws, 2, 70, 300)
    assert np.array_equal(b2, blk) and np.array_equal(s2, sbt)


def test_case_generators_are_seeded_and_as_described():
    kinds = {"image": set(), "feature": set()}
    for case in SC.CASES:
        kinds[case.config].add(case.flow)
        assert (case.C <= 3) == (case.config == "image") and case.H * case.W <= SC.MAX_PIXELS
        for k in range(2):
            a, b = SC.flow(case, k), SC.flow(case, k)
            assert torch.equal(a, b) and a.shape == (case.N, 2, case.H, case.W) and a.dtype == torch.float32 and torch.isfinite(a).all()
            assert torch.equal(SC.image(case, k), SC.image(case, k)) and SC.image(case, k).abs().max() <= 1
            for mode in SC.MODES:
                m, m2 = SC.metric(case, mode, k), SC.metric(case, mode, k)
                assert (m is None and m2 is None) or torch.equal(m, m2)
                assert mode != "linear" or (m > 0).all()
                assert (m is None) == (mode in ("summation", "average") or (mode == "softmax" and case.metric is None))
        if case.H * case.W > 1 and case.flow not in ("zero", "collapse"):
            assert not torch.equal(SC.flow(case, 0), SC.flow(case, 1)), SC.case_id(case)
        if case.metric == "beyond":
            assert case.flow in ("integer", "zero", "half")
        f = SC.flow(case)
        if case.flow in ("integer", "zero"):
            assert torch.equal(f, f.round())
        if case.flow == "outliers" and case.H * case.W > 300:
            assert 0 < (f.abs() == SC.OUTLIER).any(1).float().mean() < 3 * SC.OUTLIER_SHARE
    for config in kinds:
        assert kinds[config] >= set(SC.FLOW_KINDS), (config, set(SC.FLOW_KINDS) - kinds[config])
    assert {c.C for c in SC.FEATURE_CASES} == set(SC.FEATURE_C) and {c.C for c in SC.IMAGE_CASES} == {1, 2, 3}
    assert {(c.H, c.W) for c in SC.CASES if c.N == 2} == {(25, 65), (9, 33)}
