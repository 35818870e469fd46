"""The three kernel families that write frames — fldr_dec3_synth / fldr_dec3_synth_spk, fldr_synth_tail, and fldr_dec23_synth with its
_rows, _u16 and _u16_rows forms — against the float64 statement of tests/synth_float_ref.py, element by element within its derived
bound, on the cases of tests/synth_cases.py: one pixel, one row, one column, frames below, at and one past the 8 x 32 tile, three tiles
by three, N = 3; dyadic data whose logits every correct kernel reproduces bit for bit, bias-only logits (flat, one candidate ahead by
10 / 40 / 100, +-85 alternating at t = 0 and t = 1), generic data; candidates beyond [-1, 1], all equal, close together, strided
planes; t in {0, 1, 2^-24, 1 - 2^-24, 0.125, 0.5, 2^-25, 1/3}.

  * Logits held directly: fldr_dec3_synth[_spk](want_refine) within conv_float_ref's bound (plus the phase-weight sums), bit-equal in
    the exact and bias-only regimes.  The tail held tightly: the frame against the statement's tail on the logits the kernel returned.
  * The rounded forms (8 bit; 16 bit with white 1023 and 65535), crops and row limits against the ROUNDED STATEMENT, not against
    another kernel: equal codes except at pixels within the bound of a tie or a clamp edge (at most one code there).  In the generic
    regime the chained bound of two stacked layers is wider than a code (geometry and data ranges, not last bits): the codes are
    held to |code - V| <= bound white / 2 + 1/2 there.
  * Every output is finite wherever the statement is (every comparison asserts it).

The bound is derived, not measured (synth_float_ref's docstring); one line per case prints the worst error / bound of each form.
Packed sources are compared through the values they hold.  Every test leaves fldr_range_status and the ring's status clean."""
import pytest
import torch

import conv_float_ref as R
import synth_cases as SC
import synth_float_ref as SR
from test_gpu_parity import hip, hooks  # noqa: F401  (the module-scoped library fixture, the test-build fixture)

pytestmark = pytest.mark.gpu

T = SC.T_PARAM
NAN = float("nan")
_DEV = {}
IDS3 = dict(ids=lambda s: "N%d-%dx%d" % s)


def _inputs(case, dev):
    """The case's inputs on the device, uploaded once (the weight tensors carry the library's prepack caches); candidates 4 and 5 of a
    `pair` case are channel-strided views of the uploaded pair tensor, the six of an `equal` case one tensor."""
    if case not in _DEV:
        d = SR.reference(case)["d"]
        D = {k: v.to(dev) for k, v in d.items() if isinstance(v, torch.Tensor)}
        if case.cand == "equal":
            D["cands"] = [d["cands"][0].to(dev)] * 6
        else:
            D["cands"] = [c.contiguous().to(dev) for c in d["cands"]]
            if d["pair"] is not None:
                D["cands"][4:] = [D["pair"][:, :, 0], D["pair"][:, :, 1]]
                assert not D["cands"][5].is_contiguous()
        _DEV[case] = D
    return _DEV[case]


def _within(what, got, ref, bound):
    """Every element of `got` finite and within `bound` of `ref`; -> worst error / bound."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(ref).all()
    assert torch.isfinite(got).all(), what + ": non-finite values where the statement is finite"
    err = (got - ref).abs()
    ratio = err / bound.clamp(min=1e-300)
    if (err > bound).any():
        i = int(ratio.flatten().argmax())
        pytest.fail("%s: %d of %d elements outside the bound; worst at flat index %d: got %.17g, float64 %.17g, error %.3e, bound %.3e" % (
            what, int((err > bound).sum()), err.numel(), i, got.flatten()[i], ref.flatten()[i], err.flatten()[i], bound.flatten()[i]))
    return ratio.max().item()


def _codes(what, codes, ref, bound, Hc, Wc, white, chained=False):
    """A rounded form against the rounded statement -> share of ill pixels (chained: worst |code - V| / (D + 1/2))."""
    codes = codes.cpu()
    codes = codes.long() if codes.dtype == torch.uint8 else codes.view(torch.int16).long() & 0xFFFF
    assert tuple(codes.shape[2:]) == (Hc, Wc), (what, codes.shape)
    assert int(codes.max()) <= white, what
    if chained:
        v = ((ref[:, :, :Hc, :Wc] + 1.0) / 2.0).clamp(0.0, 1.0) * float(white)
        lim = bound[:, :, :Hc, :Wc] * float(white) / 2.0 + 2 * SR.V * float(white) + 0.5
        q = ((codes.double() - v).abs() / lim).max().item()
        assert q <= 1.0, "%s: a code is %.3f of its allowance from the statement's value" % (what, q)
        return q
    wrong, ill = SR.rounded_agree(codes, ref, bound, Hc, Wc, white)
    assert wrong == 0, "%s: %d codes differ from the rounded statement away from ties and clamp edges (or by more than one)" % (what, wrong)
    return ill                  # (its cap of 1 % is asserted on the statement alone, in tests/test_synth_ref_cpu.py)


def _show(case, fig):
    print("%s: %s" % (SC.label(case), "  ".join("%s %.3f" % kv for kv in fig.items())))


def _clean(hip):
    hip.check_range()


def _logit_bound(d, d2, mode):
    T3 = R.Terms(SC.SPEC3, [d2], d["w3"], d["b3"])
    return T3.bound(mode) + SR.PHASE * SR.U * T3.S


def _held(case, x, packed):
    """The values a packed tensor holds (the pack itself held to 2^-22 |x| + 2^-24; exact in the exact regime)."""
    v = packed.float().cpu()
    assert ((v.double() - x.double()).abs() <= R.OUT_REL * x.double().abs() + R.OUT_ABS).all(), (case, "fldr_spk_pack")
    if case.regime == "exact":
        assert torch.equal(v, x), (case, "fldr_spk_pack of values that hi + lo hold")
    return v


# ---- fldr_dec3_synth, fldr_dec3_synth_spk ---------------------------------------------------------------------------------------------
def _dec3_forms(hip, case, dev, forms=("vec", "spk")):
    """-> ({form: fp64 frame}, figures)."""
    r = SR.reference(case)
    d, D = r["d"], _inputs(case, dev)
    fig, frames = {}, {}
    for form in forms:
        if form == "vec":
            src, rr = D["d2"], r
        else:
            src = hip.spk_pack(D["d2"])
            held = _held(case, d["d2"], src)
            rr = r if case.regime != "generic" else SR.build(case, dict(d, d2=held))
        out, lg = hip.dec3_synth(src, D["w3"], D["b3"], D["cands"], D["t"], T, want_refine=True)
        lg = lg.cpu()
        what = "%s %s" % (SC.label(case), form)
        if case.regime == "generic":
            fig[form + " logits"] = _within(what + " logits", lg, rr["logits"], _logit_bound(d, rr["d2"], "fp32" if form == "vec" else "split"))
        else:
            assert torch.equal(lg.double(), rr["logits"]), what + ": logits differ from the statement's, which every operation order gives exactly"
        # the tail alone, on the logits the kernel returned
        fig[form + " tail"] = _within(what + " tail on its own logits", out, *SR.tail_bound(lg, d["cands"], d["t"], exp32=False))
        o32 = hip.dec3_synth(src, D["w3"], D["b3"], D["cands"], D["t"], T, out_dtype=torch.float32)
        assert o32.dtype == torch.float32
        fig[form + " tail f32"] = _within(what + " tail, fp32 output", o32, *SR.tail_bound(lg, d["cands"], d["t"], exp32=False, out32=True))
        # the whole operator against the statement
        fig[form] = _within(what + " frame", out, *SR.tail_bound(rr["logits"], d["cands"], d["t"], exp32=False, E=rr["E"][form]))
        frames[form] = out
    return frames, fig


@pytest.mark.parametrize("shape", SC.DEC3_SHAPES, **IDS3)
def test_dec3_synth_logits_and_tail_vs_float64(hip, dev, shape):
    hip.device_status(reset=True)
    mine = [c for c in SC.cases("dec3") if (c.h, c.w) == shape[1:]]
    assert mine
    for case in mine:
        _show(case, _dec3_forms(hip, case, dev)[1])
    _clean(hip)


@pytest.mark.parametrize("shape", SC.DEC3_SHAPES, **IDS3)
def test_synth_tail_vs_float64(hip, dev, shape):
    """fldr_synth_tail on the statement's logits rounded to fp32 (the bias-only patterns exactly), fp64 and fp32 output."""
    hip.device_status(reset=True)
    for case in [c for c in SC.cases("dec3") if (c.h, c.w) == shape[1:]]:
        r = SR.reference(case)
        d, D = r["d"], _inputs(case, dev)
        lg = r["logits"].float()
        cands = [c.contiguous() for c in D["cands"]]
        fig = {}
        for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
            out = hip.synth_tail(lg.to(dev), cands, D["t"], T, out_dtype=dt)
            assert out.dtype == dt
            fig[name] = _within("%s fldr_synth_tail %s" % (SC.label(case), name), out, *SR.tail_bound(lg, d["cands"], d["t"], exp32=False, out32=dt == torch.float32))
        _show(case, fig)
    _clean(hip)


# ---- fldr_dec23_synth -----------------------------------------------------------------------------------------------------------------
def _dec23_setup(hip, case, dev):
    """-> (positional arguments of hip.dec23_synth, the statement on the values the packed sources hold, its bound for the fp64 form)."""
    key = ("dec23", case)
    if key not in _DEV:
        r = SR.reference(case)
        d, D = r["d"], _inputs(case, dev)
        p1, pe = hip.spk_pack(D["dec1"]), hip.spk_pack(D["enc1"])
        h1, he = _held(case, d["dec1"], p1), _held(case, d["enc1"], pe)
        rr = r if case.regime != "generic" else SR.build(case, dict(d, dec1=h1, enc1=he))
        args = (p1, pe, D["w2"], D["b2"], D["w3"], D["b3"], D["cands"], D["t"], T)
        _DEV[key] = (args, rr)
    return _DEV[key]


def _dec23_bound(case, rr, out32=False):
    d = rr["d"]
    return SR.tail_bound(rr["logits"], d["cands"], d["t"], exp32=True, E=rr["E"]["dec23"], out32=out32)


def _dec23_forms(hip, case, dev, rounded=True):
    args, rr = _dec23_setup(hip, case, dev)
    H, W = 2 * case.h, 2 * case.w
    what = SC.label(case)
    ref, bound = _dec23_bound(case, rr)
    fig, outs = {}, {}
    out = hip.dec23_synth(*args)
    assert out.dtype == torch.float64 and tuple(out.shape) == (case.N, 3, H, W)
    fig["f64"] = _within(what + " fp64 frame", out, ref, bound)
    o32 = hip.dec23_synth(*args, out_dtype=torch.float32)
    assert o32.dtype == torch.float32
    fig["f32"] = _within(what + " fp32 frame", o32, *_dec23_bound(case, rr, out32=True))
    outs["f64"], outs["f32"] = out, o32
    if not rounded:
        return outs, fig
    chained = case.regime == "generic"
    worst = 0.0
    for Hc, Wc in (SC.crops(case) if not chained else SC.crops(case)[:2]):
        for white in SC.whites(case):
            if white == 255:
                codes = hip.dec23_synth(*args, u8_crop=(Hc, Wc))
                assert codes.dtype == torch.uint8
            else:
                codes = hip.dec23_synth(*args, u16_crop=(Hc, Wc), maxval=white)
                assert codes.dtype == torch.uint16
            outs[(Hc, Wc, white)] = codes
            worst = max(worst, _codes("%s crop %dx%d white %d" % (what, Hc, Wc, white), codes, ref, bound, Hc, Wc, white, chained))
    fig["codes" if chained else "ill"] = worst
    return outs, fig


@pytest.mark.parametrize("shape", SC.DEC23_SHAPES, **IDS3)
def test_dec23_synth_every_output_form_vs_float64(hip, dev, shape):
    """fp64, fp32, 8-bit and 16-bit (white 1023; 65535 where the bound stays below 1 % of a code) frames; the crop equal to the frame,
    cutting the last tile row and column, and 2 x 2."""
    hip.device_status(reset=True)
    mine = [c for c in SC.cases("dec23") if (c.h, c.w) == shape[1:]]
    assert mine
    for case in mine:
        _show(case, _dec23_forms(hip, case, dev)[1])
    _clean(hip)


@pytest.fixture
def nan_empty(monkeypatch):
    """Every tensor the library wrappers allocate with torch.empty starts as NaN (integers: all bits set), so an untouched output row is
    recognisable (as in tests/test_gpu_crop_rows.py)."""
    real = torch.empty

    def empty(*a, **k):
        t = real(*a, **k)
        if t.is_floating_point():
            t.fill_(NAN)
        elif t.dtype in (torch.uint8, torch.uint16):
            t.view(torch.uint8).fill_(255)
        return t
    monkeypatch.setattr(torch, "empty", empty)
    return empty


@pytest.mark.parametrize("shape", [s for s in SC.DEC23_SHAPES if 2 * s[1] > 16], **IDS3)
def test_dec23_row_limits_vs_float64(hip, dev, shape, nan_empty):
    """fldr_dec23_synth_rows / _u16_rows: one tile row (16 frame rows) and a tile boundary +- 1.  The rows below the limit rounded up to
    whole tile rows hold the statement (the rounded statement), the rows at or beyond it are untouched."""
    hip.device_status(reset=True)
    for case in [c for c in SC.cases("dec23") if (c.h, c.w) == shape[1:] and c.regime != "generic"]:
        args, rr = _dec23_setup(hip, case, dev)
        H, W = 2 * case.h, 2 * case.w
        ref, bound = _dec23_bound(case, rr)
        ref32, bound32 = _dec23_bound(case, rr, out32=True)
        Hc, Wc = SC.crops(case)[1]
        fig = {}
        for rows in SC.row_limits(case):
            written = min(H, -(-rows // 16) * 16)
            what = "%s row limit %d" % (SC.label(case), rows)
            for name, dt, rf, bd in (("f64", torch.float64, ref, bound), ("f32", torch.float32, ref32, bound32)):
                out = hip.dec23_synth(*args, out_dtype=dt, rows=rows).cpu()
                fig["%s r%d" % (name, rows)] = _within(what + " " + name, out[:, :, :written], rf[:, :, :written], bd[:, :, :written])
                assert torch.isnan(out[:, :, written:]).all(), what + ": wrote rows beyond the rounded-up limit"
            for white in SC.whites(case):
                kw = dict(u8_crop=(Hc, Wc)) if white == 255 else dict(u16_crop=(Hc, Wc), maxval=white)
                codes = hip.dec23_synth(*args, rows=rows, **kw).cpu()
                shown = min(Hc, written)
                _codes("%s white %d" % (what, white), codes[:, :, :shown], ref, bound, shown, Wc, white)
                assert bool((codes[:, :, shown:].contiguous().view(torch.uint8) == 255).all()), what + ": wrote codes beyond the rounded-up limit"
        _show(case, fig)
    _clean(hip)


# ---- t = 0 and t = 1 with the live candidates 170 below the others ----------------------------------------------------------------------
def test_alternating_85_logits_at_t_0_and_1_are_finite_in_every_family(hip, dev):
    """Logits (-85, +85, ...) and (+85, -85, ...) with t = (0, 1): on one sample of each the three candidates whose t weight is not zero
    are 170 below the other three.  The statement is finite and well conditioned there (the three live weights are equal: the frame is
    the mean of three candidates).  The fp32 exp2 of the fused kernel has 126 T / log2(e) = 136 of room below its maximum, so that
    maximum has to be the largest LIVE logit; the fp64 exp of the other two families has 745 T."""
    hip.device_status(reset=True)
    n = 0
    for case in SC.CASES:
        if not case.pattern.startswith("alt85"):
            continue
        r = SR.reference(case)
        d, D = r["d"], _inputs(case, dev)
        live = [0, 2, 4] if case.pattern == "alt85a" else [1, 3, 5]
        s = 0 if case.pattern == "alt85a" else 1                          # the sample whose live candidates are the low ones
        mean3 = sum(d["cands"][k][s].double() for k in live) / 3
        assert (r["out"][s] - mean3).abs().max() <= 1e-15
        if case.fam == "dec3":
            frames, fig = _dec3_forms(hip, case, dev)
            lg = r["logits"].float()
            frames["tail"] = hip.synth_tail(lg.to(dev), [c.contiguous() for c in D["cands"]], D["t"], T)
            fig["tail"] = _within(SC.label(case) + " fldr_synth_tail", frames["tail"], *SR.tail_bound(lg, d["cands"], d["t"], exp32=False))
        else:
            frames, fig = _dec23_forms(hip, case, dev)
        for name, f in frames.items():
            assert f.dtype in (torch.uint8, torch.uint16) or bool(torch.isfinite(f).all()), (case, name)
        _show(case, fig)
        n += 1
    assert n >= 4
    _clean(hip)


# ---- test build: the tile grids ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [s for s in SC.DEC3_SHAPES if s[1:] in SC.TILE_EDGE_DEC3], **IDS3)
def test_dec3_tile_grid_hooks_give_the_default_bits(hip, dev, shape, hooks):
    """fldr_debug_dec3_xshift 5 / 16 / 31 (the vector kernel's tile grid starts that many columns left of the frame) and
    fldr_debug_dec3_xcd 0 / 1 (row-major or XCD-contiguous tile ranges) only move tiles: the bits of the default, which is held to the
    float64 statement here as well."""
    L = hip.lib()
    hip.device_status(reset=True)
    try:
        for case in [c for c in SC.cases("dec3") if (c.h, c.w) == shape[1:]]:
            D = _inputs(case, dev)
            base, fig = _dec3_forms(hip, case, dev)
            srcs = {"vec": D["d2"], "spk": hip.spk_pack(D["d2"])}
            for xcd in (0, 1):
                assert L.fldr_debug_dec3_xcd(xcd) == xcd
                for xs in (-1, 5, 16, 31):
                    assert L.fldr_debug_dec3_xshift(xs) == xs
                    for form, src in srcs.items():
                        out = hip.dec3_synth(src, D["w3"], D["b3"], D["cands"], D["t"], T)
                        assert torch.equal(out, base[form]), (case, form, xcd, xs)
            L.fldr_debug_dec3_xcd(1)
            L.fldr_debug_dec3_xshift(-1)
            _show(case, fig)
    finally:
        L.fldr_debug_dec3_xcd(1)
        L.fldr_debug_dec3_xshift(-1)
    _clean(hip)


def test_dec23_one_workgroup_per_xcd_gives_the_default_bits(hip, dev, hooks):
    """fldr_debug_dec23_wgs_per_xcd(1) on 18 x 66 with N = 3: 27 tiles on 8 workgroups, three or four tiles each, against one tile per
    workgroup: the same bits in every output form, and the default is held to the float64 statement."""
    L = hip.lib()
    hip.device_status(reset=True)
    before = L.fldr_debug_dec23_wgs_per_xcd(0)
    try:
        mine = [c for c in SC.cases("dec23") if (c.N, c.h, c.w) == SC.MULTI_TILE_DEC23]
        assert mine
        for case in mine:
            args, _ = _dec23_setup(hip, case, dev)
            base, fig = _dec23_forms(hip, case, dev, rounded=case.regime != "generic")
            assert L.fldr_debug_dec23_wgs_per_xcd(1) == 1
            assert torch.equal(hip.dec23_synth(*args), base["f64"]), case
            assert torch.equal(hip.dec23_synth(*args, out_dtype=torch.float32), base["f32"]), case
            for key, codes in base.items():
                if isinstance(key, tuple):
                    Hc, Wc, white = key
                    kw = dict(u8_crop=(Hc, Wc)) if white == 255 else dict(u16_crop=(Hc, Wc), maxval=white)
                    got = hip.dec23_synth(*args, **kw)
                    assert torch.equal(got.view(torch.uint8), codes.view(torch.uint8)), (case, key)
            L.fldr_debug_dec23_wgs_per_xcd(before)
            _show(case, fig)
    finally:
        L.fldr_debug_dec23_wgs_per_xcd(before)
    _clean(hip)
