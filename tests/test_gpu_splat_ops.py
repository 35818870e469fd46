"""fldr_softsplat_acc64 — the splat of every forward — and the producers of its bounds tables alone, at the shapes where they can go
wrong, against the float64 statement of the operation (tests/splat_float_ref.py) on every case of tests/splat_cases.py: degenerate
maps, either side of the 64 x 24 / 32 x 8 tiles, of the three-tile column and of the 2304-pixel table threshold, more than 512
matching blocks (queue overflow), more than 64 super-blocks (the super-block search) and more than 64 of them matching (its
overflow); whole-pixel flows, flows a hair off a whole pixel, landings on columns and rows -1, S - 1 and S, flows that throw 1 % of
the vectors 3e9 px out, that collapse the map into one cell or empty it; metrics that put the normalisers beyond 2^100; one and two
problems per launch, the second through the batch- and channel-strided views the model passes.

The tolerance is the derived bound of splat_float_ref.bound (the roundings of the fp32 products, the two casts, a quotient within
one ulp, the post-scale; exp within twice the distance measured for torch's fp32 exp on the CPU) and nothing else; holes are exact,
and the reach map is compared without any tolerance.  tests/test_splat_ref_cpu.py holds the oracle to the same statement, shows by
a model of the search that every walk of the kernel is reached by these cases, and shows that this comparison rejects seven
mutants.  Every test prints the largest error as a share of the bound."""
import numpy as np
import pytest
import torch

import splat_cases as SC
import splat_float_ref as R64
from test_gpu_parity import hip, hooks  # noqa: F401  (the module-scoped library fixture, the test-build fixture)

pytestmark = pytest.mark.gpu

_cache = {}


def _statement(case, mode, k):
    """(out, norm, bound) of problem k of the case: computed once, shared, never written to."""
    key = (case, mode, k)
    if key not in _cache:
        img, flo, m = SC.problem(case, mode, k)
        args = (img.numpy(), flo.numpy(), None if m is None else m.numpy(), mode)
        _cache[key] = R64.splat(*args) + (R64.bound(*args, SC.exp_allowance()),)
        for a in _cache[key]:
            a.setflags(write=False)
    return _cache[key]


def _device_problems(case, mode, nprob, dev, ones=False):
    """(imgs, flows, metrics) for hip.softsplat_acc64.  Two problems: the sources are channel-strided views of one [N,C,2,H,W]
    tensor (images: the frames) or batch-strided channel slices of one [N,2C,H,W] tensor (features), the flows slices of one
    [N,4,H,W] tensor, as the model passes them."""
    probs = [SC.problem(case, mode, k) for k in range(nprob)]
    if ones:
        probs = [(torch.ones_like(p[0]), p[1], p[2]) for p in probs]
    metrics = None if probs[0][2] is None else [p[2].to(dev) for p in probs]
    if nprob == 1:
        return [probs[0][0].to(dev)], [probs[0][1].to(dev)], metrics
    C = case.C
    if case.config == "image":
        fr = torch.stack([probs[0][0], probs[1][0]], 2).to(dev)
        imgs = [fr[:, :, 0], fr[:, :, 1]]
    else:
        fd = torch.cat([probs[1][0], probs[0][0]], 1).to(dev)
        imgs = [fd[:, C:], fd[:, :C]]
    ud = torch.cat([probs[0][1], probs[1][1]], 1).to(dev)
    return imgs, [ud[:, :2], ud[:, 2:]], metrics


def _check(got, case, mode, k, what):
    """The comparison (R64.violations: the one the mutants are rejected by) -> the error as a share of the bound."""
    ref, norm, bnd = _statement(case, mode, k)
    got = got.detach().cpu().double().numpy()
    found = R64.violations(got, ref, norm, bnd)
    assert not found, "%s %s %s problem %d: %s" % (what, SC.case_id(case), mode, k, "; ".join(found))
    return R64.share_of_bound(got, ref, bnd)


def _cases(config):
    return [c for c in SC.CASES if c.config == config]


@pytest.mark.parametrize("mode", SC.MODES)
@pytest.mark.parametrize("config", ["image", "feature"])
def test_acc64_every_case_within_the_bound_of_the_statement(hip, dev, config, mode):
    """One and two problems per launch; holes exactly -1.0; FunctionSoftsplat gives the direct call's bits; the feature
    configuration's packed twin is the split of its fp32 output."""
    import softSplat
    worst = 0.0
    hip.device_status(reset=True)                                       # (sticky: whatever an earlier test left)
    for case in _cases(config):
        spk = config == "feature"
        shares = []
        for nprob in (1, 2):
            imgs, flows, metrics = _device_problems(case, mode, nprob, dev)
            res = hip.softsplat_acc64(imgs, flows, metrics, mode, want_f32=True, want_spk=spk)
            for k in range(nprob):
                out = res[k][0] if spk else res[k]
                shares.append(_check(out, case, mode, k, "acc64, %d per launch" % nprob))
                if spk:
                    assert torch.equal(hip.spk_pack(out).buf, res[k][1].buf), (SC.case_id(case), mode, nprob, k, "packed twin")
            if nprob == 1:
                op = softSplat.FunctionSoftsplat(imgs[0], flows[0], None if metrics is None else metrics[0], mode)
                assert torch.equal(op, res[0][0] if spk else res[0]), (SC.case_id(case), mode, "FunctionSoftsplat")
        worst = max(worst, max(shares))
        print("%-44s %-9s share of the bound: alone %.3f, pair %.3f %.3f" % (SC.case_id(case), mode, shares[0], shares[1], shares[2]))
    print("%s %s: largest share of the bound %.3f" % (config, mode, worst))
    assert hip.device_status(reset=True) == 0, "a packed output left the range of the fp16 split"


@pytest.mark.parametrize("config", ["image", "feature"])
def test_acc64_reach_map_equals_the_statement(hip, dev, config):
    """Independent of any tolerance: the `average` splat of an all-ones image is +1 where a cell is reached and -1 where not, and
    must equal the statement's map bit for bit, in every channel, for both problems of a pair."""
    for case in _cases(config):
        for nprob in (1, 2):
            imgs, flows, _ = _device_problems(case, "average", nprob, dev, ones=True)
            res = hip.softsplat_acc64(imgs, flows, None, "average")
            for k in range(nprob):
                want = np.broadcast_to(R64.reach(SC.flow(case, k).numpy()), res[k].shape)
                got = res[k].cpu().numpy()
                assert np.array_equal(got, want), "%s problem %d of %d: %d cells of the reach map differ" % (SC.case_id(case), k, nprob, int((got != want).sum()))
        print("%-44s reach map exact (%5.1f %% reached)" % (SC.case_id(case), 100 * float((R64.reach(SC.flow(case).numpy()) == 1).mean())))


@pytest.mark.parametrize("config", ["image", "feature"])
def test_acc64_same_case_through_every_route_to_its_candidates(hip, dev, config):
    """The exact pre-pass (its table read back from a workspace of the caller's: bit-identical to block_bounds), the whole-map walk
    (flags bit 2) and a caller-filled table each stay within the bound: every case in softmax, the cases either side of the
    2304-pixel threshold in all four modes — (36, 64) through tables, (37, 64) through the whole-map walk as well."""
    for case in _cases(config):
        H, W = case.H, case.W
        modes = SC.MODES if (H, W) in SC.ROUTE_SHAPES else ("softmax",)
        blk, sbt = R64.block_bounds(SC.flow(case).numpy())
        table = torch.from_numpy(R64.table_workspace(blk, sbt)).to(dev)
        for mode in modes:
            imgs, flows, metrics = _device_problems(case, mode, 1, dev)
            shares = {}
            ws = torch.full((hip.lib().fldr_softsplat_tile_ws_floats(case.N, H, W),), float("nan"), device=dev)
            shares["pre-pass"] = _check(hip.softsplat_acc64(imgs, flows, metrics, mode, ws=[ws])[0], case, mode, 0, "exact pre-pass")
            if H * W > R64.WHOLE_PIXELS:
                b2, s2 = R64.split_workspace(ws.cpu().numpy(), case.N, H, W)
                assert np.array_equal(b2, blk) and np.array_equal(s2, sbt), (SC.case_id(case), "the exact pre-pass's table")
            else:
                assert bool(torch.isnan(ws).all()), (SC.case_id(case), "a map without tables wrote one")
            shares["whole"] = _check(hip.softsplat_acc64(imgs, flows, metrics, mode, whole=True)[0], case, mode, 0, "whole-map walk")
            shares["table"] = _check(hip.softsplat_acc64(imgs, flows, metrics, mode, bounds_ws=[table])[0], case, mode, 0, "caller-filled table")
            print("%-44s %-9s share of the bound: %s" % (SC.case_id(case), mode, "  ".join("%s %.3f" % kv for kv in shares.items())))


def _table_checks(ws, tables, flows, spans, what):
    """ws: a workspace of `tables` tables; flows[i]: the fp32 flow [2,H,W] table i is for; spans[i]: (x, y) value range of the scaled
    low-resolution field it was made from.  Every live entry brackets the exact bounds, dead entries sit exactly outside the map,
    super-blocks are the unions of their blocks, the slack stays within the field's range."""
    H, W = flows[0].shape[1:]
    blk, sbt = R64.split_workspace(ws.cpu().numpy(), tables, H, W)
    dead = np.array([np.inf, -np.inf, np.inf, -np.inf], np.float32)
    for i in range(tables):
        eb, es = R64.block_bounds(flows[i][None].cpu().numpy())
        eb, es = eb[0], es[0]
        live = np.isfinite(eb[..., 0])
        assert np.array_equal(blk[i][~live], np.broadcast_to(dead, blk[i][~live].shape)), (what, i, "dead entries")
        assert np.isfinite(blk[i][live]).all(), (what, i, "a live entry is not finite")
        t, e = blk[i][live], eb[live]
        assert (t[:, 0] <= e[:, 0]).all() and (t[:, 1] >= e[:, 1]).all() and (t[:, 2] <= e[:, 2]).all() and (t[:, 3] >= e[:, 3]).all(), (what, i, "a block interval is too tight")
        union = np.stack([blk[i][..., 0].min(1), blk[i][..., 1].max(1), blk[i][..., 2].min(1), blk[i][..., 3].max(1)], -1)
        assert np.array_equal(sbt[i], union), (what, i, "a super-block is not the union of its blocks")
        sx = max(float((e[:, 0] - t[:, 0]).max()), float((t[:, 1] - e[:, 1]).max()))
        sy = max(float((e[:, 2] - t[:, 2]).max()), float((t[:, 3] - e[:, 3]).max()))
        assert sx <= spans[i][0] + 1e-3 and sy <= spans[i][1] + 1e-3, (what, i, sx, sy, spans[i])


def _span(lo2, scale, mul):
    """(x, y) value range of scale * lo2 * mul for one sample's [2,h,w] field."""
    return tuple(float((lo2[c].max() - lo2[c].min()) * abs(scale) * mul) for c in range(2))


def _against_statement(got, img, flo, metric, what):
    args = (img.cpu().numpy(), flo.cpu().numpy(), None if metric is None else metric.cpu().numpy(), "softmax")
    ref, norm = R64.splat(*args)
    bnd = R64.bound(*args, SC.exp_allowance())
    got = got.cpu().double().numpy()
    found = R64.violations(got, ref, norm, bnd)
    assert not found, "%s: %s" % (what, "; ".join(found))
    return R64.share_of_bound(got, ref, bnd)


@pytest.mark.parametrize("tv", SC.LOWRES_T)
def test_image_tables_from_the_low_resolution_flow(hip, dev, tv):
    """fldr_splat_bounds_upsampled and the `images` form of fldr_splat_bounds_upsampled_pair against block_bounds of the flow_t0 /
    flow_t1 that fldr_level0_prep writes (the tensors the splats read); the splats on those tables against the statement.  The
    level-0 upsampling has one whole ratio for both axes, so the fields of a non-integer ratio are left to the feature tables."""
    for lc in SC.LOWRES_CASES:
        N, h, w, H, W = lc
        if H % h or W % w or H // h != W // w:
            continue
        up = H // h
        lo = SC.lowres_flow(lc).to(dev)
        fr = SC.image(SC.Case("image", N, 6, H, W, "zero", None)).view(N, 3, 2, H, W).to(dev)
        I0, I1 = fr[:, :, 0], fr[:, :, 1]
        ts = [tv if n == 0 else (0.3 if tv != 0.3 else 1.0) for n in range(N)]
        t4 = torch.tensor(ts).view(N, 1, 1, 1).to(dev)
        r = hip.level0_prep(lo, I0, I1, t4, H, W, -1.894, -1.8942, withmask=True, want_z=True)
        f0, f1 = r["flow_t0"], r["flow_t1"]
        b0 = hip.splat_bounds_upsampled(lo[:, 2:], t4, 1, float(up), H, W)
        b1 = hip.splat_bounds_upsampled(lo[:, :2], t4, 2, float(up), H, W)
        bw = hip.splat_bounds_upsampled_pair(lo, t4, "images", float(up), H, W)
        loc = lo.cpu()
        s0 = [_span(loc[n, 2:], ts[n], up) for n in range(N)]
        s1 = [_span(loc[n, :2], 1 - ts[n], up) for n in range(N)]
        _table_checks(b0, N, list(f0), s0, "upsampled t*flow_01 %s" % (lc,))
        _table_checks(b1, N, list(f1), s1, "upsampled (1-t)*flow_10 %s" % (lc,))
        _table_checks(bw, 2 * N, list(f0) + list(f1), s0 + s1, "pair images %s" % (lc,))
        shares = []
        for tables in ([b0, b1], bw):
            w0, w1 = hip.softsplat_acc64([I0, I1], [f0, f1], [r["z0"], r["z1"]], "softmax", bounds_ws=tables)
            shares.append(_against_statement(w0, I0, f0, r["z0"], "splat of I0 on the low-resolution tables %s" % (lc,)))
            shares.append(_against_statement(w1, I1, f1, r["z1"], "splat of I1 on the low-resolution tables %s" % (lc,)))
        print("image tables %s t %s: contained, unions exact, slack within the field's range; splats at %.3f of the bound" % (lc, ts, max(shares)))


def test_feature_tables_from_the_previous_level_flow(hip, dev):
    """fldr_splat_bounds_upsampled (unscaled), the `features` form of fldr_splat_bounds_upsampled_pair and the fused
    fldr_resize_bilinear_spk_bounds against block_bounds of the fldr_resize_bilinear_spk output (the tensor the feature splats
    read), ragged sizes and the non-integer ratio included; the feature splats on those tables against the statement.
    The fused launch takes W < 4 w only.  Its entry point is called directly on the fields of SC.LOWRES_FUSED — (2,13,21,26,42),
    (1,30,75,59,149), (1,34,40,68,80), (1,1,33,2,65), (1,20,1,40,2), (2,18,33,35,65): h = 1, w = 1 and W = 65 among them — and must
    refuse the others — (1,9,15,72,120), (1,1,16,8,128), (1,20,1,80,4), (2,7,13,35,65), ratios of 4 and more —, for which
    fldr_hip.resize_bilinear_spk_bounds falls back to the two launches: there the fourth table is the pair kernel's again."""
    C = 17
    assert hip.RESIZE_BOUNDS
    assert {1} <= {c[1] for c in SC.LOWRES_FUSED} and {1} <= {c[2] for c in SC.LOWRES_FUSED} and 65 in {c[4] for c in SC.LOWRES_FUSED}
    for lc in SC.LOWRES_CASES:
        N, h, w, H, W = lc
        prev = SC.lowres_flow(lc, 1).to(dev)
        mul = W / w
        up, _ = hip.resize_bilinear_spk(prev, H, W, mul=mul)
        up2 = torch.empty(N, 4, H, W, device=dev)
        sp2 = hip._spk_alloc(N, 4, H, W, dev)
        bw_fused = torch.full((2 * hip.lib().fldr_softsplat_tile_ws_floats(N, H, W),), float("nan"), device=dev)
        rc = hip.lib().fldr_resize_bilinear_spk_bounds(prev.data_ptr(), up2.data_ptr(), sp2.ptr, bw_fused.data_ptr(), N, h, w, H, W, float(mul), hip._stream())
        if lc in SC.LOWRES_FUSED:
            assert rc == 0 and W < 4 * w, (lc, rc)                      # the fused kernel itself ran
        else:
            assert rc != 0 and W >= 4 * w and bool(torch.isnan(bw_fused).all()), (lc, rc)
            up2, _, bw_fused = hip.resize_bilinear_spk_bounds(prev, H, W, mul=mul)        # the two launches
        assert torch.equal(up, up2)
        bw = hip.splat_bounds_upsampled_pair(prev, None, "features", mul, H, W)
        b0 = hip.splat_bounds_upsampled(prev[:, :2], None, 0, mul, H, W)
        b1 = hip.splat_bounds_upsampled(prev[:, 2:], None, 0, mul, H, W)
        pc = prev.cpu()
        s0 = [_span(pc[n, :2], 1.0, mul) for n in range(N)]
        s1 = [_span(pc[n, 2:], 1.0, mul) for n in range(N)]
        f0, f1 = up[:, :2], up[:, 2:]
        _table_checks(b0, N, list(f0), s0, "upsampled flow_10 %s" % (lc,))
        _table_checks(b1, N, list(f1), s1, "upsampled flow_01 %s" % (lc,))
        _table_checks(bw, 2 * N, list(f0) + list(f1), s0 + s1, "pair features %s" % (lc,))
        _table_checks(bw_fused, 2 * N, list(f0) + list(f1), s0 + s1, "fused resize + bounds %s" % (lc,))
        feat = SC.image(SC.Case("feature", N, 2 * C, H, W, "zero", None)).to(dev)
        shares = []
        for tables in ([b0, b1], bw, bw_fused):
            a0, a1 = hip.softsplat_acc64([feat[:, C:], feat[:, :C]], [f0, f1], None, "softmax", bounds_ws=tables)
            shares.append(_against_statement(a0, feat[:, C:], f0, None, "feature splat 0 on the low-resolution tables %s" % (lc,)))
            shares.append(_against_statement(a1, feat[:, :C], f1, None, "feature splat 1 on the low-resolution tables %s" % (lc,)))
        print("feature tables %s: contained, unions exact, slack within the field's range; splats at %.3f of the bound" % (lc, max(shares)))


# the folded walk takes effect from 512 tiles and two channel groups on: the overflow map as a pair, at C = 17
FOLD_CASES = [SC.Case("feature", 1, 17, 1040, 65, "wild", "model"), SC.Case("feature", 1, 17, 1040, 65, "smooth", "unit")]


@pytest.mark.parametrize("hook", ["quad", "group_fold"])
def test_acc64_test_build_walks_within_the_bound(hip, hooks, dev, hook):
    """Test build, tile-edge and overflow shapes only: the image walk by one pixel per item (fldr_debug_splat_quad(0)) and the
    feature walk with all channel groups of a tile in one workgroup (fldr_debug_splat_group_fold(1)) stay within the bound too.
    Only the cases on which the hook changes the walk run.  quad: the image cases of SC.HOOK_SHAPES with W % 4 == 0 — (24, 64),
    (72, 64), (73, 68), (1040, 68); the others take the one-pixel walk in the product already.  group_fold: the fold needs 512 tiles
    and two channel groups, which none of the feature cases has (the tile-edge maps have a handful of tiles, the overflow map runs
    at C = 16, one group), so it runs on FOLD_CASES alone: the overflow map at C = 17, 780 tiles as a pair."""
    if hook == "quad":
        cases = [c for c in _cases("image") if (c.H, c.W) in SC.HOOK_SHAPES and c.W % 4 == 0]
        assert {(c.H, c.W) for c in cases} == {(24, 64), (72, 64), (73, 68), (1040, 68)}
    else:
        cases = FOLD_CASES
        assert all(c.C > 16 and 2 * -(-c.W // 32) * -(-c.H // 8) >= 512 for c in cases)
    fn, on, off = (hooks.fldr_debug_splat_quad, 0, 1) if hook == "quad" else (hooks.fldr_debug_splat_group_fold, 1, 0)
    try:
        assert fn(on) == on
        for case in cases:
            for mode in SC.MODES:
                imgs, flows, metrics = _device_problems(case, mode, 2, dev)
                res = hip.softsplat_acc64(imgs, flows, metrics, mode)
                shares = [_check(res[k], case, mode, k, "test build, %s" % hook) for k in range(2)]
                print("%-44s %-9s %s: share of the bound %.3f %.3f" % (SC.case_id(case), mode, hook, shares[0], shares[1]))
    finally:
        fn(off)
    assert fn(-1) == off
