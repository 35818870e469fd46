"""Every convolution entry point against the float64 statement of tests/conv_float_ref.py, element by element within its derived bound,
on the cases of tests/conv_cases.py: one pixel, one row, one column, frames below, at and one past the 8 x 32 (and 8 x 16) tile, N = 3,
a nearest-x2 source of 1 x 1; the model's twelve layers and generic ones; unit, post-ReLU, mixed-magnitude and dark data; plain weights
and weights with one value 1e3 times the rest.  The split-packed kernels are otherwise held bit-identical to fldr_conv2d_split and to
each other, and share its split, tile walk and epilogue: a fault in the shared code passes those tests and fails these
(tests/test_conv_ref_cpu.py shows that six such faults leave the bound on every case).

The bound is derived, not measured (conv_float_ref's docstring); the printed figures, one line per case, are the worst error / bound
of each form.  Packed sources, residuals and outputs are compared through the values they hold.  Every test leaves
fldr_range_status and the ring's timeout count clean."""
import ctypes

import pytest
import torch

import conv_cases as CC
import conv_float_ref as R
from test_gpu_parity import hip, hooks  # noqa: F401  (the module-scoped library fixture, the test-build fixture)

pytestmark = pytest.mark.gpu

FLDR_E_SHAPE = -2
S1 = [s for s in CC.SPECS if s.stride == 1]
S2 = [s for s in CC.SPECS if s.stride == 2]
LEVELS = [s for s in S1 if len(s.parts) == 1 and not any(s.up2) and not s.store]
IDS = dict(ids=lambda s: s.name)

_DEV, _PACKED = {}, {}


def _inputs(case, dev):
    """The case's inputs on the device, uploaded once (the weight tensor carries the library's prepack cache)."""
    if case not in _DEV:
        d = R.reference(case)[0]
        _DEV[case] = dict(srcs=[s.to(dev) for s in d["srcs"]], w=d["w"].to(dev), b=None if d["b"] is None else d["b"].to(dev),
                          res=None if d["res"] is None else d["res"].to(dev))
    return _DEV[case]


def _within(what, got, ref, bound):
    """Every element of `got` within `bound` of `ref`; -> worst error / bound."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what + ": non-finite values"
    err = (got - ref).abs()
    ratio = err / bound.clamp(min=1e-300)
    if (err > bound).any():
        i = int(ratio.flatten().argmax())
        pytest.fail("%s: %d of %d elements outside the bound; worst at flat index %d: got %.9g, float64 %.9g, error %.3e, bound %.3e" % (
            what, int((err > bound).sum()), err.numel(), i, got.flatten()[i], ref.flatten()[i], err.flatten()[i], bound.flatten()[i]))
    return ratio.max().item()


def _label(case):
    return "%-16s N %d %2dx%-2d %-5s %-5s" % (case.spec.name, case.N, case.H, case.W, case.kind, case.wkind)


def _show(case, figures):
    print("%s: %s" % (_label(case), "  ".join("%s %.3f" % kv for kv in figures.items())))


def _clean(hip):
    assert hip.device_status(reset=True) == 0, "fldr_range_status / fldr_ring_status raised on in-range data"


def _packed(hip, case, dev):
    """The case's sources (and residual) split-packed by fldr_spk_pack, and the statement on the values the packed tensors hold:
    -> dict(srcs, res: Spk; act: the statement without residual; T: its terms; res_f32 / res_spk: the residual values).  The pack itself
    is held to 2^-22 |x| + 2^-24 here."""
    if case not in _PACKED:
        s = case.spec
        d = R.reference(case)[0]
        D = _inputs(case, dev)
        out = dict(srcs=[hip.spk_pack(x) for x in D["srcs"]], res=None, res_f32=d["res"], res_spk=None)
        vals = [p.float().cpu() for p in out["srcs"]]
        for v, x in zip(vals, d["srcs"]):
            assert ((v.double() - x.double()).abs() <= R.OUT_REL * x.double().abs() + R.OUT_ABS).all(), (case, "fldr_spk_pack")
        if s.residual:
            out["res"] = hip.spk_pack(D["res"])
            out["res_spk"] = out["res"].float().cpu()
            assert ((out["res_spk"].double() - d["res"].double()).abs() <= R.OUT_REL * d["res"].double().abs() + R.OUT_ABS).all(), (case, "fldr_spk_pack")
        out["act"] = R.statement(s, vals, d["w"], d["b"])
        out["T"] = R.Terms(s, vals, d["w"], d["b"])
        _PACKED[case] = out
    return _PACKED[case]


def _spk_forms(hip, case, dev, product_forms=True):
    """fldr_conv2d_spk in its forms -> {form: worst error / bound}.  With product_forms = False only the two forms the kernel-variant
    tests repeat per variant: packed sources to both outputs (fp32 residual), and to the packed output alone (no residual)."""
    s = case.spec
    d, ref, T = R.reference(case)
    D = _inputs(case, dev)
    P = _packed(hip, case, dev)
    kw = dict(relu=s.relu, cout_store=s.store, up2=list(s.up2))
    fig = {}
    refp = P["act"] + (P["res_f32"].double() if s.residual else 0.0)
    Tp = P["T"].with_residual(P["res_f32"]) if s.residual else P["T"]
    o32, osp = hip.conv2d_spk(P["srcs"], D["w"], D["b"], residual=D["res"], want_f32=True, want_spk=True, **kw)
    fig["spk>f32"] = _within(_label(case) + " packed sources, fp32 output", o32, refp, Tp.bound("split"))
    fig["spk>spk"] = _within(_label(case) + " packed sources, packed output", osp.float(), refp, Tp.bound("split", refp, packed_out=True))
    if not s.residual:
        only = hip.conv2d_spk(P["srcs"], D["w"], D["b"], want_f32=False, want_spk=True, **kw)
        fig["spk>spk only"] = _within(_label(case) + " packed sources, packed output alone", only.float(), refp, Tp.bound("split", refp, packed_out=True))
    if not product_forms:
        return fig
    got = hip.conv2d_spk(D["srcs"], D["w"], D["b"], residual=D["res"], **kw)
    fig["f32>f32"] = _within(_label(case) + " fp32 sources, fp32 output", got, ref, T.bound("split"))
    if s.residual:
        refq = P["act"] + P["res_spk"].double()
        Tq = P["T"].with_residual(P["res_spk"])
        o32, osp = hip.conv2d_spk(P["srcs"], D["w"], D["b"], residual=P["res"], want_f32=True, want_spk=True, **kw)
        fig["res spk>f32"] = _within(_label(case) + " packed residual, fp32 output", o32, refq, Tq.bound("split"))
        fig["res spk>spk"] = _within(_label(case) + " packed residual, packed output", osp.float(), refq, Tq.bound("split", refq, packed_out=True))
        only = hip.conv2d_spk(P["srcs"], D["w"], D["b"], residual=P["res"], want_f32=False, want_spk=True, **kw)
        fig["res spk>spk only"] = _within(_label(case) + " packed residual, packed output alone", only.float(), refq, Tq.bound("split", refq, packed_out=True))
    got = hip.conv2d_spk(P["srcs"], D["w"], D["b"], residual=D["res"], precision="fp16", **kw)
    fig["fp16"] = _within(_label(case) + " packed sources, one product", got, refp, Tp.bound("fp16"))
    return fig


# ---- product library ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", CC.SPECS, **IDS)
def test_conv2d_three_precisions_vs_float64(hip, dev, spec):
    """fldr_conv2d (exact), fldr_conv2d_split (three products, one product) and fldr_conv2d_s2_split through hip.conv2d."""
    hip.device_status(reset=True)
    for case in CC.cases([spec]):
        d, ref, T = R.reference(case)
        D = _inputs(case, dev)
        fig = {}
        for prec in ("fp32", "split", "fp16"):
            kw = dict(stride=spec.stride, relu=spec.relu, residual=D["res"], cout_store=spec.store, up2=list(spec.up2), precision=prec)
            if prec == "fp32" and spec.k == 4 and 32 < spec.cout <= 48:            # the exact 4x4 kernel has no 48-channel form: refused, not run
                with pytest.raises(hip.FldrError):
                    hip.conv2d(D["srcs"], D["w"], D["b"], **kw)
                continue
            mode = "split" if (prec == "fp16" and spec.stride == 2) else prec      # (stride 2 has no one-product kernel)
            fig[prec] = _within("%s precision %s" % (_label(case), prec), hip.conv2d(D["srcs"], D["w"], D["b"], **kw), ref, T.bound(mode))
        if spec.stride == 2:
            o32, osp = hip.conv2d(D["srcs"], D["w"], D["b"], stride=2, relu=spec.relu, cout_store=spec.store, precision="split", want_spk=True)
            fig["split>spk"] = _within(_label(case) + " packed twin", osp.float(), ref, T.bound("split", ref, packed_out=True))
        _show(case, fig)
    _clean(hip)


def test_conv2d_stride2_beyond_64_outputs_is_refused(hip, dev):
    case = CC.Case(CC.REFUSED_S2, 1, 16, 64, "unit", "plain")
    d = CC.make(case)
    for prec in ("fp32", "split"):
        with pytest.raises(hip.FldrError):
            hip.conv2d([s.to(dev) for s in d["srcs"]], d["w"].to(dev), d["b"].to(dev), stride=2, relu=True, precision=prec)


@pytest.mark.parametrize("spec", S1, **IDS)
def test_conv2d_spk_every_form_vs_float64(hip, dev, spec):
    """fldr_conv2d_spk from fp32 and from packed sources; fp32, packed or both outputs; fp32 and packed residual; nearest-x2 sources
    and cout_store as the spec has them; the one-product form."""
    hip.device_status(reset=True)
    for case in CC.cases([spec]):
        _show(case, _spk_forms(hip, case, dev))
    _clean(hip)


@pytest.mark.parametrize("spec", LEVELS, **IDS)
def test_conv2d_spk_levels_edge_shapes_as_levels(hip, dev, spec):
    """fldr_conv2d_spk_levels with the ten edge shapes as the levels of two launches (sample 0 of every case; the weights and bias of the
    spec's first case): fp32 sources to both outputs with fp32 residuals, packed sources to packed outputs with packed residuals."""
    hip.device_status(reset=True)
    cases = CC.cases([spec])
    d0 = R.reference(cases[0])[0]
    w, b = d0["w"], d0["b"]
    wd, bd = _inputs(cases[0], dev)["w"], _inputs(cases[0], dev)["b"]
    for group in (cases[:5], cases[5:]):
        xs = [R.reference(c)[0]["srcs"][0][:1] for c in group]
        rs = [R.reference(c)[0]["res"][:1] for c in group] if spec.residual else None
        xd, rd = [x.to(dev) for x in xs], ([r.to(dev) for r in rs] if rs else None)
        got = hip.conv2d_spk_levels(xd, wd, bd, relu=spec.relu, residuals=rd, want_f32=True, want_spk=True)
        xp, rp = [hip.spk_pack(x) for x in xd], ([hip.spk_pack(r) for r in rd] if rd else None)
        gotp = hip.conv2d_spk_levels(xp, wd, bd, relu=spec.relu, residuals=rp, want_f32=False, want_spk=True)
        for l, case in enumerate(group):
            res = rs[l] if rs else None
            ref, T = R.statement(spec, [xs[l]], w, b, res), R.Terms(spec, [xs[l]], w, b, res)
            fig = {"f32>f32": _within(_label(case) + " level, fp32 output", got[l][0], ref, T.bound("split")),
                   "f32>spk": _within(_label(case) + " level, packed output", got[l][1].float(), ref, T.bound("split", ref, packed_out=True))}
            xv, rv = xp[l].float().cpu(), (rp[l].float().cpu() if rp else None)
            ref, T = R.statement(spec, [xv], w, b, rv), R.Terms(spec, [xv], w, b, rv)
            fig["spk>spk"] = _within(_label(case) + " level, packed sources and residual", gotp[l].float(), ref, T.bound("split", ref, packed_out=True))
            _show(case, fig)
    _clean(hip)


def _s2_spk_specs(hip):
    return [s for s in S2 if len(s.parts) == 1 and s.parts[0] % 8 == 0 and s.parts[0] <= 64]


def _s2_spk_forms(hip, case, dev):
    """fldr_conv2d_s2_spk (both outputs, packed alone) and fldr_conv2d_s2_spk_pair on the packed source -> figures.  A layer of up to
    32 outputs is paired with itself, channels rolled by one; a wider one (enc3) runs as its two halves, which is what the pair form
    is for.  Each half has its own prepack scale, hence its own terms."""
    s = case.spec
    d = R.reference(case)[0]
    D = _inputs(case, dev)
    P = _packed(hip, case, dev)
    vals = [P["srcs"][0].float().cpu()]
    fig = {}
    if s.cout <= 32:
        assert hip.s2_spk_ok(D["w"]), s.name
        ref, T = P["act"], P["T"]
        o32, osp = hip.conv2d_s2_spk(P["srcs"][0], D["w"], D["b"], relu=s.relu, want_f32=True, want_spk=True)
        fig["s2spk>f32"] = _within(_label(case) + " s2 on packed source, fp32 output", o32, ref, T.bound("split"))
        fig["s2spk>spk"] = _within(_label(case) + " s2 on packed source, packed output", osp.float(), ref, T.bound("split", ref, packed_out=True))
        only = hip.conv2d_s2_spk(P["srcs"][0], D["w"], D["b"], relu=s.relu, want_f32=False, want_spk=True)
        fig["s2spk>spk only"] = _within(_label(case) + " s2 on packed source, packed output alone", only.float(), ref, T.bound("split", ref, packed_out=True))
        halves = [(d["w"], d["b"]), (torch.roll(d["w"], 1, 0), None if d["b"] is None else torch.roll(d["b"], 1, 0))]
    else:
        h = s.cout // 2
        halves = [(d["w"][:h].contiguous(), d["b"][:h].contiguous()), (d["w"][h:].contiguous(), d["b"][h:].contiguous())]
    key = ("pair", case)
    if key not in _DEV:
        _DEV[key] = [(w.to(dev), None if b is None else b.to(dev)) for w, b in halves]
    assert hip.s2_spk_ok(_DEV[key][0][0]), s.name
    outs = hip.conv2d_s2_spk_pair(P["srcs"][0], _DEV[key], relu=s.relu)
    for k, ((w, b), o) in enumerate(zip(halves, outs)):
        sh = s._replace(cout=w.shape[0])
        ref, T = R.statement(sh, vals, w, b), R.Terms(sh, vals, w, b)
        fig["pair%d" % k] = _within(_label(case) + " s2 pair, half %d" % k, o.float(), ref, T.bound("split", ref, packed_out=True))
    return fig


def test_conv2d_s2_spk_and_pair_vs_float64(hip, dev):
    hip.device_status(reset=True)
    specs = _s2_spk_specs(hip)
    assert {s.name for s in specs} >= {"enc2", "enc3", "s8->16", "s24->17", "s40->32"}
    for case in CC.cases(specs):
        _show(case, _s2_spk_forms(hip, case, dev))
    _clean(hip)


# ---- writes stay inside the output --------------------------------------------------------------------------------------------------------
GUARD = 4096
SENTINEL = -12345.678


@pytest.mark.parametrize("spec", [s for s in CC.SPECS if s.name in ("conv_flow_bottom.8", "g7->17", "g100->96", "dec2", "enc1", "s7->17", "s3+3+1->6/4", "s100->64")], **IDS)
def test_conv2d_writes_only_its_output_slab(hip, dev, spec):
    """hip.conv2d(out=) into a contiguous slab cut from a larger buffer of sentinels, at the shapes with partial tiles: the slab holds the
    convolution (so every element was written), the guard zones before and after it still hold the sentinel."""
    hip.device_status(reset=True)
    for case in CC.cases([spec]):
        Ho, Wo = CC.out_size(case)
        if Ho % 8 == 0 and Wo % 32 == 0:
            continue
        d, ref, T = R.reference(case)
        D = _inputs(case, dev)
        n = ref.numel()
        for prec in ("fp32", "split"):
            big = torch.full((GUARD + n + GUARD,), SENTINEL, device=dev)
            slab = big[GUARD:GUARD + n].view(ref.shape)
            out = hip.conv2d(D["srcs"], D["w"], D["b"], stride=spec.stride, relu=spec.relu, residual=D["res"], cout_store=spec.store,
                             up2=list(spec.up2), out=slab, precision=prec)
            assert out.data_ptr() == slab.data_ptr()
            r = _within("%s precision %s into a slab" % (_label(case), prec), slab, ref, T.bound(prec))
            assert (big[:GUARD] == SENTINEL).all() and (big[GUARD + n:] == SENTINEL).all(), "%s precision %s: wrote outside its output" % (_label(case), prec)
            print("%s precision %s: slab of %d floats, guards untouched, worst error / bound %.3f" % (_label(case), prec, n, r))
    _clean(hip)


# ---- stride-2 inputs with no output row or column -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", CC.DEGENERATE_S2, ids=lambda s: "%dx%d" % s)
def test_stride2_input_without_output_is_refused_before_any_launch(hip, dev, size):
    """Hin or Win below 2: (H + 2 - 4) // 2 + 1 = 0.  The binding sizes the output with that formula and every entry point refuses the
    empty output.  C's truncating division gives 1 instead, and a caller that sizes the output that way would have been launched:
    fldr_conv2d, fldr_conv2d_s2_split and fldr_conv2d_s2_spk[_pair] return FLDR_E_SHAPE for it and leave the output untouched."""
    Hin, Win = size
    cin, cout = 8, 16
    g = torch.Generator().manual_seed(5)
    x = torch.rand(1, cin, Hin, Win, generator=g).to(dev)
    w = (torch.randn(cout, cin, 4, 4, generator=g) / 11).to(dev)
    xp = hip.spk_pack(x)
    for prec in ("split", "fp32"):
        with pytest.raises(hip.FldrError):
            hip.conv2d([x], w, None, stride=2, precision=prec)
    with pytest.raises(hip.FldrError):
        hip.conv2d_s2_spk(xp, w, None)
    with pytest.raises(hip.FldrError):
        hip.conv2d_s2_spk_pair(xp, [(w, None), (w, None)])
    Ho, Wo = int((Hin + 2 - 4) / 2) + 1, int((Win + 2 - 4) / 2) + 1            # as C computes it: truncation towards zero
    assert Ho >= 1 and Wo >= 1
    out = torch.full((cout * Ho * Wo + 256,), SENTINEL, device=dev)
    L = hip.lib()
    for fn, wp, src in ((L.fldr_conv2d, hip.conv_prepack(w), x.data_ptr()), (L.fldr_conv2d_s2_split, hip.conv_s2_prepack(w), x.data_ptr()),
                        (L.fldr_conv2d_s2_spk, hip.conv_s2_prepack(w), xp.ptr)):
        d = hip.ConvDesc()
        d.src[0], d.src_c[0], d.n_src = src, cin, 1
        d.wpack, d.out = wp.data_ptr(), out.data_ptr()
        d.N, d.cin, d.cout, d.cout_store = 1, cin, cout, cout
        d.Hin, d.Win, d.Hout, d.Wout = Hin, Win, Ho, Wo
        d.ksize, d.stride = 4, 2
        assert fn(ctypes.byref(d), hip._stream()) == FLDR_E_SHAPE
        if fn is L.fldr_conv2d_s2_spk:
            assert L.fldr_conv2d_s2_spk_pair(ctypes.byref(d), ctypes.byref(d), hip._stream()) == FLDR_E_SHAPE
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()


# ---- test build: the kernel variants, on the tile-edge shapes -----------------------------------------------------------------------------
# (spk variant, ring consumers, ring tile width, resident weights, small-unit threshold): what test_spk_conv_bit_identical_to_split_conv
# switches between, and the 16-channel sub-group launches switched off
SPK_VARIANTS = [("barrier", 0, 8, 0, 0, 96), ("ring4", 1, 4, 0, 0, 96), ("ring8 w32", 1, 8, 32, 0, 96), ("ring8 w16", 1, 8, 16, 0, 96),
                ("resident8", 1, 8, 0, 1, 96), ("resident4", 1, 4, 0, 1, 96), ("whole groups", 1, 8, 0, 0, -1)]


def _spk_defaults(L):
    L.fldr_debug_spk_variant(1)
    L.fldr_debug_ring_consumers(8)
    L.fldr_debug_ring_tile_width(0)
    L.fldr_debug_ring_resident(0)
    L.fldr_debug_spk_small_units(96)
    L.fldr_debug_ring32(1)


@pytest.mark.parametrize("spec", S1, **IDS)
def test_spk_kernel_variants_at_tile_edges_vs_float64(hip, dev, spec, hooks):
    """The barrier pipeline, the ring with 4 and 8 consumers, 16- and 32-wide tiles, resident weights, whole 48-channel groups instead
    of 16-channel sub-groups, and ring32 forced (64 / 96 outputs, packed output alone): each against the float64 statement."""
    L = hip.lib()
    hip.device_status(reset=True)
    edge = [c for c in CC.cases([spec]) if CC.tile_edge(c)]
    assert edge
    try:
        for case in edge:
            fig = {}
            for name, variant, cons, tw, resident, small in SPK_VARIANTS:
                L.fldr_debug_spk_variant(variant)
                L.fldr_debug_ring_consumers(cons)
                L.fldr_debug_ring_tile_width(tw)
                L.fldr_debug_ring_resident(resident)
                L.fldr_debug_spk_small_units(small)
                fig[name] = max(_spk_forms(hip, case, dev, product_forms=False).values())
            _spk_defaults(L)
            if spec.cout in (64, 96) and not spec.residual and not spec.store:
                D, P = _inputs(case, dev), _packed(hip, case, dev)
                L.fldr_debug_spk_small_units(-1)
                assert L.fldr_debug_ring32(2) == 2
                got = hip.conv2d_spk(P["srcs"], D["w"], D["b"], relu=spec.relu, up2=list(spec.up2), want_f32=False, want_spk=True)
                fig["ring32"] = _within(_label(case) + " ring32", got.float(), P["act"], P["T"].bound("split", P["act"], packed_out=True))
                _spk_defaults(L)
            _show(case, fig)
    finally:
        _spk_defaults(L)
    assert L.fldr_debug_ring_timeouts() == 0
    _clean(hip)


# (persistent, tile-grid shift, 16-byte staging): what test_stride2_persistent_kernel_bit_identical_to_per_tile switches between
S2_VARIANTS = [("per tile", 0, -1, 1), ("persistent", 1, -1, 1), ("shift 15", 1, 15, 1), ("shift 15 no vec4", 1, 15, 0), ("shift 31", 1, 31, 1)]


@pytest.mark.parametrize("spec", S2, **IDS)
def test_stride2_kernel_variants_at_tile_edges_vs_float64(hip, dev, spec, hooks):
    """fldr_conv2d_s2_split per tile and persistent, with the tile grid shifted and the 16-byte staging off; fldr_conv2d_s2_spk and its
    pair form with and without the LDS-DMA kernel: each against the float64 statement."""
    L = hip.lib()
    hip.device_status(reset=True)
    edge = [c for c in CC.cases([spec]) if CC.tile_edge(c)]
    assert edge
    try:
        for case in edge:
            d, ref, T = R.reference(case)
            D = _inputs(case, dev)
            fig = {}
            for name, mode, shift, v4 in S2_VARIANTS:
                L.fldr_debug_s2_persistent(mode)
                L.fldr_debug_s2_xshift(shift)
                L.fldr_debug_s2_vec4(v4)
                o32, osp = hip.conv2d(D["srcs"], D["w"], D["b"], stride=2, relu=spec.relu, cout_store=spec.store, precision="split", want_spk=True)
                fig[name] = max(_within("%s %s" % (_label(case), name), o32, ref, T.bound("split")),
                                _within("%s %s, packed twin" % (_label(case), name), osp.float(), ref, T.bound("split", ref, packed_out=True)))
            L.fldr_debug_s2_persistent(1)
            L.fldr_debug_s2_xshift(-1)
            L.fldr_debug_s2_vec4(1)
            if spec in _s2_spk_specs(hip):
                for dma in (0, 1):
                    assert L.fldr_debug_s2_dma(dma) == dma
                    fig["dma %d" % dma] = max(_s2_spk_forms(hip, case, dev).values())
            _show(case, fig)
    finally:
        L.fldr_debug_s2_persistent(1)
        L.fldr_debug_s2_xshift(-1)
        L.fldr_debug_s2_vec4(1)
        L.fldr_debug_s2_dma(1)
    _clean(hip)


# ---- weight prepacks: the bytes of the recorded parent; the LDS limit across layer widths ------------------------------------------------
def _same_digests(got, prefix_is_ringrow):
    import prepack_cases as PC
    want = {k: v for k, v in PC.DIGESTS.items() if k.startswith("ringrow") == prefix_is_ringrow}
    assert set(got) == set(want)
    wrong = sorted(k for k in got if got[k] != want[k])
    assert not wrong, "packed bytes differ from the recorded ones: %s" % ", ".join(wrong)


def test_prepack_bytes_are_the_recorded_ones(hip, dev):
    """sha256 of every weight pack (header included) of fresh seeded weights — split, spk (with its R32 section), stride 2 (with and
    without its DMA section), dec23, both dec3 forms; plain, all-zero and spiked weights — against the digests tests/prepack_cases.py
    records from commit 80b93a2's product library, the last before the prepack kernels were merged."""
    import prepack_cases as PC
    _same_digests(PC.product_digests(hip, dev), False)


def test_ringrow_prepack_bytes_are_the_recorded_ones(hip, dev, hooks):
    """The same for the ringrow weight section, through its hook of the test build (digests: commit 80b93a2's test build)."""
    import prepack_cases as PC
    _same_digests(PC.ringrow_digests(hip, hooks, dev), True)


def test_lds_limit_follows_ascending_cin(dev, clean_launcher):
    """tests/conv_lds_child.py in a fresh process (started through the GPU-clean launcher, as every GPU child of this suite: a timeout,
    the exit status checked): the stride-2 kernels whose dynamic LDS grows with cin, narrow layer first, every result within the
    float64 bound.  The widths are the widest each kernel takes; 64 inputs, which none takes from a packed source, must be refused."""
    import os
    import sys
    r = clean_launcher([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_lds_child.py")], env=dict(os.environ), timeout=240)
    print(r["stdout"])
    assert r["rc"] == 0 and "lds limit child: ok" in r["stdout"], (r["rc"], r["stderr"][-3000:])
