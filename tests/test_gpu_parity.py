"""Parity tests proper: every operator and the whole frame-pair forward, through the C ABI (libfldr_hip.so via
fldr_hip.py and the reference-named host modules), against the CPU oracle and the committed golden vectors.

Tolerances (fp32 path; stated per test):
  * gather / resize / PCA / tail kernels follow the oracle's operation order -> 1e-6 .. 1e-5 absolute;
  * the default splat (fldr_softsplat_acc64) accumulates the reference kernel's fp32 corner products in fp64 LDS tiles: the
    sums are independent of the summation order to ~1e-16 relative, two runs of a forward give the same bits (asserted at
    4K); the reference's own fp32 atomicAdd order is non-deterministic -> 1e-5 relative to the accumulated
    magnitude against the oracle;
  * convolutions: exact fp32 products, fp32 accumulation in a different order than MKL-DNN -> 2e-5 * sqrt(K);
  * whole model: ~10x the errors measured on MI355X (7e-7 at 256x256, 1.9e-6 at 200x500, 1.3e-5 at 4K; 97-101 dB):
    max 2e-5 on the small golden cases, max 1e-4 / mean 1e-6 elsewhere, >= 90 dB PSNR between the rounded 8-bit
    frames.  A 10x numerical regression fails.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _cmp(got, ref, atol, rtol=0.0, max_outlier_frac=0.0, what="", ill=None, outlier_atol=None):
    """Every element within atol + rtol |ref|.  Exceptions are conditioning-derived only: `ill` (a boolean tensor broadcastable to
    the outputs) marks the positions the ORACLE reports as ill-conditioned (a hard threshold within rounding of its operand):
    elements beyond the tolerance must all lie there.  `max_outlier_frac` (with `outlier_atol`: the bound the outliers still
    meet) is for rounding-boundary cases only — a last-bit difference of a cast — never an unbounded allowance."""
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all(), what + ": non-finite values"
    err = (got - ref).abs()
    bad = err > (atol + rtol * ref.abs())
    if ill is not None:
        stray = bad & ~ill.expand_as(bad)
        assert not stray.any(), "%s: %d elements beyond tol outside the ill-conditioned positions (of %d beyond tol, %d ill-conditioned), max err there %.3e" % (
            what, int(stray.sum()), int(bad.sum()), int(ill.expand_as(bad).sum()), err[stray].max().item())
        return err[~ill.expand_as(bad)].max().item() if (~ill.expand_as(bad)).any() else 0.0
    frac = bad.double().mean().item()
    assert frac <= max_outlier_frac, "%s: %.3g of elements beyond tol, max err %.3e" % (what, frac, err.max().item())
    if max_outlier_frac > 0.0:
        assert outlier_atol is not None and err.max().item() <= outlier_atol, "%s: outlier of %.3e (allowed %s)" % (what, err.max().item(), outlier_atol)
    return err.max().item()


BWARP_BAND = 1e-4       # |mask value - 0.999| below which the backward warp's hard threshold (fLDRnet.py:573-574) is ill-conditioned


def _bwarp_ill(oracle, shape, flo):
    """Pixels whose backward-warp mask value (oracle.bwarp_mask_value: what fLDRnet.py:573 thresholds) lies within BWARP_BAND of the
    threshold: the only positions where the HIP kernel's mask may differ from the reference's."""
    return (oracle.bwarp_mask_value(shape, flo) - oracle.BWARP_MASK_THRESHOLD).abs() < BWARP_BAND


@pytest.fixture(scope="module")
def hip():
    import fldr_hip
    fldr_hip.lib()
    return fldr_hip


@pytest.fixture(scope="module")
def model(dev):
    import fldr_harness as Hn
    m, _, a = Hn.prepare_model(dev)
    return m, a


@pytest.fixture
def hooks(hip):
    """Tests that switch kernel variants / tuning values run on the TEST build (libfldr_hip_test.so: the product kernels + the
    fldr_debug_* hooks and the retired cross-check kernels); everything else runs on the product library."""
    with hip.test_hooks() as L:
        yield L


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------
# softmax splat
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 3, 64, 96), (2, 5, 37, 91), (1, 49, 18, 30), (1, 1, 1, 1)])
def test_splat_raw_matches_oracle(hip, oracle, dev, shape):
    N, C, H, W = shape
    g = _gen(1)
    x = torch.rand(N, C, H, W, generator=g) * 2 - 1
    flow = (torch.rand(N, 2, H, W, generator=g) - 0.5) * 12
    flow[:, :, :2] *= 40                                         # far out-of-range rows
    import softSplat
    out = softSplat._FunctionSoftsplat.apply(x.to(dev), flow.to(dev))
    _cmp(out, oracle.splat_forward(x, flow), atol=2e-5, rtol=1e-5, what="splat raw")


@pytest.mark.parametrize("mode", ["summation", "average", "linear", "softmax"])
def test_function_softsplat_modes(hip, oracle, dev, mode):
    import softSplat
    g = _gen(2)
    x = torch.rand(2, 4, 33, 70, generator=g) * 2 - 1
    flow = (torch.rand(2, 2, 33, 70, generator=g) - 0.5) * 9
    z = torch.randn(2, 1, 33, 70, generator=g) if mode in ("linear", "softmax") else None
    if mode == "linear":
        z = z.abs() + 0.1
    out = softSplat.FunctionSoftsplat(x.to(dev), flow.to(dev), None if z is None else z.to(dev), mode)
    _cmp(out, oracle.function_softsplat(x, flow, z, mode), atol=3e-5, rtol=1e-5, what=mode)
    if mode == "softmax":
        out = softSplat.Softsplat()(x.to(dev), flow.to(dev))
        _cmp(out, oracle.function_softsplat(x, flow, None, mode), atol=3e-5, what="softmax no metric")


@pytest.mark.parametrize("shape", [(1, 9, 15, 8, 0.5), (2, 12, 20, 8, 0.125), (1, 36, 60, 4, 0.875), (1, 11, 14, 3, 0.3), (1, 7, 9, 2, 0.6), (1, 10, 6, 16, 0.5)])
def test_level0_prep_bit_identical_to_unfused(hip, dev, shape):
    """fldr_level0_prep (one pass) against the kernels it fuses: resize_bilinear, zmetric, bwarp_tscaled, bwarp."""
    N, h, w, up, tv = shape
    H, W = h * up, w * up
    g = _gen(31)
    flow_lo = ((torch.rand(N, 4, h, w, generator=g) - 0.5) * 6).to(dev)
    x = (torch.rand(N, 3, 2, H, W, generator=g) * 2 - 1).to(dev)
    I0, I1 = x[:, :, 0].contiguous(), x[:, :, 1].contiguous()
    t4 = torch.full((N, 1, 1, 1), tv).to(dev)
    za0, za1 = -1.894, -1.8942
    r = hip.level0_prep(flow_lo, I0, I1, t4, H, W, za0, za1, withmask=True, want_z=True)
    both = hip.resize_bilinear(flow_lo, H, W, mul=float(up))
    f10, f01 = both[:, :2], both[:, 2:]
    assert torch.equal(r["z0"], hip.zmetric(I0, I1, f01, za0)) and torch.equal(r["z1"], hip.zmetric(I1, I0, f10, za1))
    tl = hip.resize_bilinear(torch.cat([t4 * flow_lo[:, 2:], (1 - t4) * flow_lo[:, :2]], 1), H, W, mul=float(up))
    assert torch.equal(r["flow_t0"], tl[:, 0:2]) and torch.equal(r["flow_t1"], tl[:, 2:4])
    fb0 = hip.bwarp_tscaled(f10, f01, t4, "t", "1-t", withmask=True)
    fb1 = hip.bwarp_tscaled(f01, f10, t4, "1-t", "t", withmask=True)
    assert torch.equal(r["flowback_0"], fb0) and torch.equal(r["flowback_1"], fb1)
    assert torch.equal(r["im0_tot"], hip.bwarp(I0, fb0, True)) and torch.equal(r["im1_tot"], hip.bwarp(I1, fb1, True))


@pytest.mark.parametrize("shape", [(1, 20, 70, 8, 0.5, 1.0, "shift"), (2, 9, 33, 8, 0.125, 6.0, "noise"), (1, 6, 40, 16, 0.75, 3.0, "noise"), (1, 37, 45, 8, 0.3, 400.0, "noise"),
                                   (1, 24, 32, 8, 0.5, 0.2, "zoom"), (1, 11, 14, 3, 0.3, 2.0, "noise"), (1, 20, 21, 4, 0.6, 30.0, "edge")])
def test_level0_prep_flow_fields_bit_identical_to_unfused(hip, dev, shape):
    """fldr_level0_prep against the unfused kernels (resize_bilinear, zmetric, bwarp_tscaled, bwarp) on the flow fields that stress its
    taps: rigid shifts, smooth zoom, noise and 400 px wild flows (taps far outside the frame: clamped corners, masked weights), a motion
    edge; x3 / x4 / x8 / x16 upsampling (the integer source-index arithmetic of the power-of-two scales and the general path); frames read
    in place as channel-strided views, from a copy, at a 4-byte offset; the two-phase call; without masks / metrics.  Every plane
    bit-identical."""
    N, h, w, up, tv, amp, kind = shape
    H, W = h * up, w * up
    g = _gen(77)
    if kind == "shift":
        flow_lo = (torch.tensor([-0.75, -0.5, 0.75, 0.5]).view(1, 4, 1, 1) + (torch.rand(N, 4, h, w, generator=g) - 0.5) * 0.02 * amp)
    elif kind == "zoom":
        ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
        fx, fy = (xs - w / 2) * 0.03 * amp, (ys - h / 2) * 0.03 * amp
        flow_lo = torch.stack([fx, fy, -fx, -fy], 0).unsqueeze(0).repeat(N, 1, 1, 1)
    elif kind == "edge":
        flow_lo = torch.zeros(N, 4, h, w)
        flow_lo[:, :, :, w // 2:] = torch.tensor([amp / up, 1.0, -amp / up, -1.0]).view(1, 4, 1, 1)
    else:
        flow_lo = (torch.rand(N, 4, h, w, generator=g) - 0.5) * amp
    flow_lo = flow_lo.to(dev)
    x = (torch.rand(N, 3, 2, H, W, generator=g) * 2 - 1).to(dev)
    t4 = torch.full((N, 1, 1, 1), tv).to(dev)
    keys = ("z0", "z1", "flow_t0", "flow_t1", "flowback_0", "flowback_1", "im0_tot", "im1_tot")
    I0, I1 = x[:, :, 0], x[:, :, 1]                                       # strided views: read in place
    za0, za1 = -1.894, -1.8942
    r = hip.level0_prep(flow_lo, I0, I1, t4, H, W, za0, za1, withmask=True, want_z=True)
    # the unfused chain
    I0c, I1c = I0.contiguous(), I1.contiguous()
    both = hip.resize_bilinear(flow_lo, H, W, mul=float(up))
    f10, f01 = both[:, :2], both[:, 2:]
    tl = hip.resize_bilinear(torch.cat([t4 * flow_lo[:, 2:], (1 - t4) * flow_lo[:, :2]], 1), H, W, mul=float(up))
    fb0 = hip.bwarp_tscaled(f10, f01, t4, "t", "1-t", withmask=True)
    fb1 = hip.bwarp_tscaled(f01, f10, t4, "1-t", "t", withmask=True)
    ref = {"z0": hip.zmetric(I0c, I1c, f01, za0), "z1": hip.zmetric(I1c, I0c, f10, za1), "flow_t0": tl[:, 0:2], "flow_t1": tl[:, 2:4],
           "flowback_0": fb0, "flowback_1": fb1, "im0_tot": hip.bwarp(I0c, fb0, True), "im1_tot": hip.bwarp(I1c, fb1, True)}
    rc = hip.level0_prep(flow_lo, I0c, I1c, t4, H, W, za0, za1, withmask=True, want_z=True)
    st = hip.level0_prep(flow_lo, I0, I1, t4, H, W, za0, za1, withmask=True, want_z=True, phase=1)
    st = hip.level0_prep(None, None, None, None, H, W, 0, 0, state=st)
    for k in keys:
        assert torch.equal(r[k], ref[k]), k
        assert torch.equal(rc[k], ref[k]) and torch.equal(st[k], ref[k]), k
    nz = hip.level0_prep(flow_lo, I0, I1, t4, H, W, za0, za1, withmask=False, want_z=False)
    fb0n = hip.bwarp_tscaled(f10, f01, t4, "t", "1-t", withmask=False)
    assert torch.equal(nz["flowback_0"], fb0n) and torch.equal(nz["im0_tot"], hip.bwarp(I0c, fb0n, False)) and torch.equal(nz["flow_t1"], ref["flow_t1"])
    # frames at a 4-byte offset
    buf = torch.empty(x.numel() + 1, device=dev)
    buf[1:] = x.reshape(-1)
    xo = buf[1:].view_as(x)
    ro = hip.level0_prep(flow_lo, xo[:, :, 0], xo[:, :, 1], t4, H, W, za0, za1, withmask=True, want_z=True)
    for k in keys:
        assert torch.equal(ro[k], ref[k]), ("misaligned", k)


@pytest.mark.parametrize("shape", [(1, 27, 60, 8, 0.5, 6.0), (2, 13, 21, 8, 0.25, 40.0), (1, 9, 15, 4, 1.0, 2.0), (1, 34, 40, 8, 0.0, 10.0)])
def test_splat_bounds_from_low_resolution_flow(hip, oracle, dev, shape, hooks):
    """fldr_splat_bounds_upsampled (the bounds table of the level-0 image splats from the LOW-resolution flow): every block /
    super-block interval must contain the exact interval of the full-resolution flow_t that fldr_level0_prep writes, and the
    splat run on that table must equal the exact-bounds splat up to summation order and the oracle.  (Test build: the exact table is
    read back from the retired band splat fldr_softsplat_tile, which only that build has.)"""
    import ctypes
    N, h, w, up, tv, amp = shape
    H, W = h * up, w * up
    g = _gen(101)
    flow_lo = ((torch.rand(N, 4, h, w, generator=g) - 0.5) * amp).to(dev)
    x = (torch.rand(N, 3, 2, H, W, generator=g) * 2 - 1).to(dev)
    I0, I1 = x[:, :, 0], x[:, :, 1]
    t4 = torch.full((N, 1, 1, 1), tv).to(dev)
    r = hip.level0_prep(flow_lo, I0, I1, t4, H, W, -1.894, -1.8942, withmask=True, want_z=True)
    L = hip.lib()
    for img, flow, z, lo, smode in ((I0, r["flow_t0"], r["z0"], flow_lo[:, 2:], 1), (I1, r["flow_t1"], r["z1"], flow_lo[:, :2], 2)):
        ws_lo = hip.splat_bounds_upsampled(lo, t4, smode, float(up), H, W)
        exact = hip.softsplat_fused(img, flow, z, "softmax", kernel="tile")
        # the exact table: run the exact-bounds entry on a workspace of our own and read it back
        ws_ex = torch.empty_like(ws_lo)
        imgc = img.contiguous()
        out = torch.empty(N, 3, H, W, device=dev)
        assert L.fldr_softsplat_tile(ctypes.c_void_p(imgc.data_ptr()), ctypes.c_void_p(flow.data_ptr()), ctypes.c_void_p(z.data_ptr()),
                                     ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ws_ex.data_ptr()), N, 3, H, W, 3, None) == 0
        torch.cuda.synchronize()
        a, b = ws_lo.view(-1, 4).cpu(), ws_ex.view(-1, 4).cpu()
        live = torch.isfinite(b[:, 0])
        assert torch.equal(live, torch.isfinite(a[:, 0]))                      # the same blocks are inside the image
        a, b = a[live], b[live]
        assert bool((a[:, 0] <= b[:, 0]).all() and (a[:, 1] >= b[:, 1]).all() and (a[:, 2] <= b[:, 2]).all() and (a[:, 3] >= b[:, 3]).all())
        slack = torch.max((b[:, 0] - a[:, 0]).max(), (a[:, 1] - b[:, 1]).max())
        assert float(slack) <= amp * up * max(tv, 1 - tv) + 1e-3                # never wider than the value range of the field
        got = hip.softsplat_fused(img, flow, z, "softmax", bounds_ws=ws_lo)
        assert (got - exact).abs().max().item() <= 2e-6
        _cmp(got, oracle.function_softsplat(img.contiguous().cpu(), flow.cpu(), z.cpu(), "softmax"), atol=3e-5, what="splat on low-res bounds")


def test_channel_strided_frames_read_in_place(hip, dev):
    """I0 / I1 are the views x[:, :, 0] / x[:, :, 1] of the [B,3,2,H,W] input (fLDRnet.py:130-131): level0_prep, the
    splat, the stride-2 encoder and dec3_synth read them through batch + channel strides and must give exactly what
    they give on contiguous copies."""
    N, h, w, up = 2, 12, 20, 8
    H, W = h * up, w * up
    g = _gen(77)
    x = (torch.rand(N, 3, 2, H, W, generator=g) * 2 - 1).to(dev)
    flow_lo = ((torch.rand(N, 4, h, w, generator=g) - 0.5) * 6).to(dev)
    t4 = torch.tensor([0.25, 0.75]).view(N, 1, 1, 1).to(dev)
    views = (x[:, :, 0], x[:, :, 1])
    copies = (views[0].contiguous(), views[1].contiguous())
    assert not views[0][0].is_contiguous()
    res = []
    r = hip.level0_prep(flow_lo, copies[0], copies[1], t4, H, W, -1.9, -1.8, withmask=True, want_z=True)
    w0 = hip.softsplat_fused(copies[0], r["flow_t0"], r["z0"], "softmax")
    w1 = hip.softsplat_fused(copies[1], r["flow_t1"], r["z1"], "softmax")
    for I0, I1 in (views, copies):
        r = hip.level0_prep(flow_lo, I0, I1, t4, H, W, -1.9, -1.8, withmask=True, want_z=True)
        wt = (torch.rand(16, 10, 4, 4, generator=_gen(3)) - 0.5).to(dev)
        b = (torch.rand(16, generator=_gen(4)) - 0.5).to(dev)
        e = hip.conv2d([I0, I1, r["flow_t0"], r["flow_t1"]], wt, b, stride=2, relu=True, precision="split")
        d2 = torch.rand(N, 16, H // 2, W // 2, generator=_gen(5)).to(dev)
        w3 = (torch.rand(6, 16, 3, 3, generator=_gen(6)) - 0.5).to(dev)
        b3 = (torch.rand(6, generator=_gen(7)) - 0.5).to(dev)
        o = hip.dec3_synth(d2, w3, b3, [w0, w1, r["im0_tot"], r["im1_tot"], I0, I1], t4, 1.56)
        res.append([r[k] for k in ("z0", "z1", "flowback_0", "im0_tot", "im1_tot")] + [e, o])
    for a, b in zip(*res):
        assert torch.equal(a, b)
    # the default splat (fp64 LDS-atomic tiles) reads the strided views in place too: the same bits
    assert torch.equal(hip.softsplat_fused(views[0], r["flow_t0"], r["z0"], "softmax"), w0)
    assert torch.equal(hip.softsplat_fused(views[1], r["flow_t1"], r["z1"], "softmax"), w1)


def test_model_fused_synthesis_matches_the_two_kernel_form(hip, dev, model):
    """The model's default synthesis (fldr_dec23_synth: dec2 + dec3 + blend in one kernel) against its two-kernel form (conv2d_spk for dec2,
    then dec3_synth — what FLDR_DEC23=0 selects and what sizes that are not multiples of 4 at half resolution fall back to): same frame to
    fp32 accumulation rounding of dec2 + fp64 rounding of the tail."""
    import fldr_harness as Hn
    m, a = model
    for (H, W, seed) in ((256, 384, 11), (200, 330, 12)):
        f = Hn.frames_from_uint8(Hn.synthetic_pair(H, W, seed=seed)).to(dev)
        t = torch.tensor([[0.375]], device=dev)
        was = hip.DEC23_FUSED                                               # (False when the suite runs under FLDR_DEC23=0)
        try:
            hip.DEC23_FUSED = True
            fused = Hn.interpolate(m, a, f, t)
            hip.DEC23_FUSED = False
            two = Hn.interpolate(m, a, f, t)
        finally:
            hip.DEC23_FUSED = was
        assert fused.dtype == two.dtype == torch.float64 and fused.shape == two.shape == (1, 3, H, W)
        _cmp(fused, two, atol=3e-6, what="fused synthesis vs dec2 + dec3 kernels %dx%d" % (H, W))
    hip.check_range()


def test_graphed_interpolator_replays_the_eager_forward(hip, dev, model):
    """fldr_harness.GraphedInterpolator (the opt-in hipGraph replay of the harness; bench.py's steps are its replays): captured on one
    pair, fed two other pairs of the same shape — every replay == the eager forward of that pair, bit for bit; a prebuilt pyramid as the
    captured input works the same way; with the pair cache on it refuses."""
    import fldr_harness as Hn
    m, a = model
    pairs = [Hn.frames_from_uint8(Hn.synthetic_pair(200, 328, seed=s)).to(dev) for s in (3, 4, 5)]
    t = torch.tensor([[0.5]], device=dev)
    g = Hn.GraphedInterpolator(m, a, pairs[0], t)
    for f, tv in ((pairs[1], 0.5), (pairs[2], 0.25), (pairs[0], 0.875)):
        tt = torch.tensor([[tv]], device=dev)
        out = g(f, tt).clone()                       # (the caller's stream waits for the replay)
        ref = Hn.interpolate(m, a, f, tt)
        torch.cuda.synchronize()
        assert out.shape == (1, 3, 200, 328) and torch.equal(out, ref), tv
    pyr = Hn.build_pyramid(Hn.pad_frames(pairs[1], a), a)
    gp = Hn.GraphedInterpolator(m, a, pairs[1], t, pyramid=pyr)
    out = gp.replay(join=True).clone()
    assert torch.equal(out, Hn.interpolate(m, a, pairs[1], t))
    with pytest.raises(RuntimeError):
        gp(pairs[2], t)
    m.pair_cache = True
    try:
        with pytest.raises(RuntimeError):
            Hn.GraphedInterpolator(m, a, pairs[0], t)
    finally:
        m.pair_cache = False
    hip.check_range()


def test_pca_stream_equals_two_pass(hip, dev, model):
    """One-pass projection (raw fp64 parked, streaming rescale) == two-pass kernel bit for bit; its split-packed twin ==
    fldr_spk_pack of the fp32 output."""
    m, _ = model
    g = _gen(5)
    pl = (torch.rand(12, 72, 136, generator=g) * 2 - 1).to(dev)
    o32, o64, mm = hip.pca_project(pl, m.EV8.detach(), m.Mean8.detach(), m.meanVec8.detach(), want_f64=True)
    s32, s64, smm, spk = hip.pca_project_stream(pl, m.EV8.detach(), m.Mean8.detach(), m.meanVec8.detach(), want_spk=True)
    assert torch.equal(o32, s32) and torch.equal(o64, s64) and torch.equal(mm, smm)
    assert torch.equal(hip.spk_pack(o32.view(1, 192, 9, 17)).buf, spk.buf)


@pytest.mark.parametrize("K", [16, 8, 4])
def test_pca_pyramid_bit_identical_to_per_level(hip, dev, model, K, hooks):
    """fldr_pca_project_pyramid, vector kernel (all levels in two launches, pixel-major table, Markstein quotients, no fp64
    intermediate) against the per-level one-pass kernels of fldr_pca_project_stream: fp32 output, split-packed twin and
    min / max are the same bits at every level, including levels of a few blocks and an odd number of planes."""
    m, _ = model
    g = _gen(31)
    ev, mean, mv = m.EV8.detach()[:K].contiguous(), m.Mean8.detach(), m.meanVec8.detach()[:K].contiguous()
    P = 6 if K != 4 else 5
    levels = [(64, 96), (32, 48), (16, 24), (8, 8), (40, 520)]
    planes = [(torch.rand(P, h, w, generator=g) * 2 - 1).to(dev) for (h, w) in levels]
    assert hip.lib().fldr_debug_pca_variant(-1) == 0
    o32, osp, mm = hip.pca_project_pyramid(planes, ev, mean, mv, want_f32=True, want_spk=True)
    for i, pl in enumerate(planes):
        s32, s64, smm, spk = hip.pca_project_stream(pl, ev, mean, mv, want_spk=True)
        assert torch.equal(smm, mm[i]), (i, smm, mm[i])
        assert torch.equal(s32, o32[i]), (i, (s32 - o32[i]).abs().max().item())
        assert torch.equal(spk.buf, osp[i].buf), i
    only_spk = hip.pca_project_pyramid(planes, ev, mean, mv, want_f32=False, want_spk=True)[1]
    assert all(torch.equal(a.buf, b.buf) for a, b in zip(only_spk, osp))
    # one read of the frames: the first pass parks the un-normalised projections of the big levels as fp64 and a streaming launch
    # rescales them (every level / the levels above a size / none): the same bits
    for raw_min in (0, P * (32 // 8) * (48 // 8) * K * 8 + 1, 1 << 40):
        r32, rsp, rmm = hip.pca_project_pyramid(planes, ev, mean, mv, want_f32=True, want_spk=True, raw_min_bytes=raw_min)
        assert torch.equal(rmm, mm)
        assert all(torch.equal(a, b) for a, b in zip(r32, o32)) and all(torch.equal(a.buf, b.buf) for a, b in zip(rsp, osp)), raw_min


def test_pca_pyramid_matrix_core_kernel(hip, oracle, dev, model, hooks):
    """The opt-in K = 16 pyramid kernel on the fp64 matrix cores (v_mfma_f64_16x16x4_f64; pixels summed in the matrix instruction's order) against the
    per-level vector kernels and the oracle: min / max to 1e-13 relative, the fp32 casts equal except where an fp64 rounding
    difference crosses an fp32 rounding boundary (<= 1 ulp of 1.0, < 0.1 % of the elements), the packed twin = the pack of
    its own fp32 output.  Levels: many rows of 16-block tiles, rows that are no multiple of 16 blocks (tiles wrap), fewer
    than 32 blocks (dead lanes), a level of one block per plane."""
    m, _ = model
    g = _gen(33)
    ev, mean, mv = m.EV8.detach(), m.Mean8.detach(), m.meanVec8.detach()
    levels = [(64, 1024), (72, 136), (32, 48), (16, 24), (8, 8), (40, 520)]
    planes = [(torch.rand(6, h, w, generator=g) * 2 - 1).to(dev) for (h, w) in levels]
    L = hip.lib()
    try:
        assert L.fldr_debug_pca_variant(1) == 1
        o32, osp, mm = hip.pca_project_pyramid(planes, ev, mean, mv, want_f32=True, want_spk=True)
        for i, pl in enumerate(planes):
            s32, s64, smm, spk = hip.pca_project_stream(pl, ev, mean, mv, want_spk=True)
            assert torch.allclose(smm, mm[i], rtol=1e-13, atol=0.0), (i, smm, mm[i])
            d = (s32 - o32[i]).abs()
            assert d.max().item() <= 1.2e-7 and (d > 0).float().mean().item() < 1e-3, (i, d.max().item(), (d > 0).float().mean().item())
            P, H, W = pl.shape
            assert torch.equal(hip.spk_pack(o32[i].reshape(1, P * 16, H // 8, W // 8)).buf, osp[i].buf), i
            ref = oracle.to_pca_diff(pl.double().cpu(), mean.cpu(), ev.cpu(), mv.cpu())
            _cmp(o32[i].reshape(ref.shape), ref, atol=2e-7, what="matrix-core PCA vs oracle, level %d" % i)
        only_spk = hip.pca_project_pyramid(planes, ev, mean, mv, want_f32=False, want_spk=True)[1]
        assert all(torch.equal(a.buf, b.buf) for a, b in zip(only_spk, osp))
    finally:
        L.fldr_debug_pca_variant(0)


@pytest.mark.parametrize("shape", [(1, [96], [0], 96, None, 9, 15, True, True), (2, [96], [0], 48, None, 20, 37, True, False),
                                   (1, [48, 48, 4], [0, 0, 0], 96, None, 36, 60, True, False), (1, [48], [0], 6, 4, 9, 15, False, False),
                                   (1, [64, 32], [1, 0], 32, None, 24, 40, True, False), (1, [32, 16], [1, 0], 16, None, 48, 80, True, False),
                                   (1, [96], [0], 96, None, 72, 120, True, True), (1, [96], [0], 96, None, 136, 240, True, False),
                                   (2, [96], [0], 48, None, 136, 240, True, False), (1, [48, 48, 4], [0, 0, 0], 96, None, 136, 250, True, True),
                                   # 16-output-channel launches of <= 4 input chunks: the resident-weight ring (5 slots, two fills in flight)
                                   (1, [32, 16], [1, 0], 16, None, 272, 480, True, False), (1, [48], [0], 4, None, 136, 250, True, True),
                                   (2, [64], [0], 16, None, 70, 100, False, False), (1, [16], [0], 16, None, 40, 64, True, False),
                                   (1, [16], [0], 12, None, 8, 20, True, True)])
def test_spk_conv_bit_identical_to_split_conv(hip, dev, shape, hooks):
    """The persistent split-packed convolution (fldr_conv2d_spk) against the register-staged split convolution
    (fldr_conv2d_split): same hi/lo split, same MFMA order => bit-identical fp32 output; its packed output equals
    fldr_spk_pack of that output; a chain through the packed tensor equals the chain through fp32."""
    N, cs, ups, cout, cst, H, W, relu, res = shape
    g = _gen(21)
    srcs = [torch.randn(N, c, H // (2 if u else 1), W // (2 if u else 1), generator=g).to(dev) for c, u in zip(cs, ups)]
    wt = (torch.randn(cout, sum(cs), 3, 3, generator=g) / 20).to(dev)
    b = torch.randn(cout, generator=g).to(dev)
    rs = torch.randn(N, cst or cout, H, W, generator=g).to(dev) if res else None
    up2 = [bool(u) for u in ups]
    ref = hip.conv2d(srcs, wt, b, relu=relu, residual=rs, cout_store=cst, up2=up2, precision="split")
    L = hip.lib()
    try:
        # every pipeline of fldr_conv2d_spk: barrier pipeline; loader/consumer ring with 4 consumer waves, with 8 (default) on
        # 8x32 and on 8x16 tiles, and with the tile width picked per launch (the default)
        # (last column: the resident-weight ring of the test build where it applies — 16 output channels, <= 4 input chunks)
        for variant, cons, tw, resident in ((0, 8, 0, 1), (1, 4, 0, 1), (1, 8, 32, 1), (1, 8, 16, 1), (1, 8, 0, 1), (1, 8, 0, 0), (1, 4, 0, 0)):
            L.fldr_debug_spk_variant(variant)
            L.fldr_debug_ring_consumers(cons)
            L.fldr_debug_ring_tile_width(tw)
            L.fldr_debug_ring_resident(resident)
            got, gp = hip.conv2d_spk(srcs, wt, b, relu=relu, residual=rs, cout_store=cst, up2=up2, want_f32=True, want_spk=True)
            assert torch.equal(ref, got), (variant, cons, tw, resident)
            assert torch.equal(hip.spk_pack(ref).buf, gp.buf), (variant, cons, tw, resident)
    finally:
        L.fldr_debug_spk_variant(1)
        L.fldr_debug_ring_consumers(8)
        L.fldr_debug_ring_tile_width(0)
        L.fldr_debug_ring_resident(0)
    assert L.fldr_debug_ring_timeouts() == 0
    if len(cs) == 1 and cst is None and cout % 8 == 0:
        w2 = (torch.randn(48, cout, 3, 3, generator=g) / 20).to(dev)
        assert torch.equal(hip.conv2d([ref], w2, None, precision="split"), hip.conv2d_spk([gp], w2, None))
        half = cout // 2
        if half % 8 == 0:                                  # channel views of a packed tensor (feat[:, :48] / feat[:, 48:])
            w3 = (torch.randn(16, half, 3, 3, generator=g) / 20).to(dev)
            assert torch.equal(hip.conv2d([ref[:, half:]], w3, None, precision="split"), hip.conv2d_spk([gp.narrow(half, half)], w3, None))


@pytest.mark.parametrize("shape", [(16, 32, 50, 70, 2), (8, 16, 34, 130, 1), (32, 16, 18, 66, 1), (16, 32, 144, 240, 1), (24, 16, 20, 36, 1),
                                   (32, 32, 68, 120, 1), (32, 32, 272, 96, 2), (40, 24, 30, 44, 1)])
def test_stride2_conv_on_packed_source(hip, dev, shape):
    """fldr_conv2d_s2_spk (enc2 reading enc1's packed output): the bits of the fp32-source stride-2 kernel on the values the
    packed tensor holds — fp32 and packed outputs, odd sizes, batch of 2, several workgroup rounds."""
    cin, cout, H, W, N = shape
    g = _gen(88)
    x = F.relu(torch.randn(N, cin, H, W, generator=g)).to(dev) * 3
    wt = (torch.randn(cout, cin, 4, 4, generator=g) / (cin * 16) ** 0.5).to(dev)
    b = torch.randn(cout, generator=g).to(dev)
    xp = hip.spk_pack(x)
    xv = xp.float()                                         # hi + lo: what the packed tensor holds
    assert hip.s2_spk_ok(wt)
    got32, gotp = hip.conv2d_s2_spk(xp, wt, b, relu=True, want_f32=True, want_spk=True)
    ref32, refp = hip.conv2d([xv], wt, b, stride=2, relu=True, want_spk=True)
    # the fp32-source kernel splits xv again: hi / lo of (hi + lo) are hi / lo themselves except where lo's own rounding moved a bit
    _cmp(got32, ref32, atol=2e-6 * float(ref32.abs().max()) + 1e-7, what="s2 on packed source")
    assert torch.equal(hip.spk_pack(got32).buf, gotp.buf)
    only = hip.conv2d_s2_spk(xp, wt, b, relu=True, want_f32=False, want_spk=True)
    assert torch.equal(only.buf, gotp.buf)
    # two convolutions of the same packed source in one launch (enc3's halves): the bits of the two separate calls
    wt2 = (torch.rand(*wt.shape, generator=_gen(8)) - 0.5).to(dev) * 0.1
    b2 = (torch.rand(wt.shape[0], generator=_gen(9)) - 0.5).to(dev)
    pa, pb = hip.conv2d_s2_spk_pair(xp, [(wt, b), (wt2, b2)], relu=True)
    assert torch.equal(pa.buf, gotp.buf) and torch.equal(pb.buf, hip.conv2d_s2_spk(xp, wt2, b2, relu=True, want_f32=False, want_spk=True).buf)
    ref = F.relu(F.conv2d(xv.double().cpu(), wt.double().cpu(), b.double().cpu(), stride=2, padding=1))
    a32 = hip.conv2d([xv], wt, b, stride=2, relu=True, precision="fp32").double().cpu()
    e32, esp = (a32 - ref).abs().mean().item(), (got32.double().cpu() - ref).abs().mean().item()
    assert esp <= 1.5 * e32 + 1e-8, (esp, e32)


@pytest.mark.parametrize("shape", [(1, [96], [0], 96, 72, 120, True), (1, [48, 48, 4], [0, 0, 0], 96, 36, 60, True), (2, [96], [0], 96, 50, 70, False),
                                   (1, [32, 32], [0, 0], 64, 144, 240, True), (1, [64, 32], [1, 0], 64, 48, 80, True), (1, [96], [0], 96, 288, 480, True),
                                   (1, [16], [0], 64, 9, 15, False), (3, [40], [0], 96, 17, 33, True)])
def test_ring32_conv_matches_the_16x16x32_kernels(hip, dev, shape, hooks):
    """conv3x3_ring32_kernel (v_mfma_f32_32x32x16_f16 tiles, 4-slot ring, no pad tap; 64 / 96 output channels, packed output) against the
    16x16x32 ring kernel: another summation order (tap by tap instead of tap pairs, term-major), so equal to fp32 accumulation rounding,
    and not less accurate against fp64 than the exact-fp32-product kernel; multi-source, nearest-x2 source, partial tiles, batches,
    several rounds of persistent workgroups, launches too small to fill the chip."""
    N, cs, ups, cout, H, W, relu = shape
    g = _gen(52)
    srcs = [torch.randn(N, c, H // (2 if u else 1), W // (2 if u else 1), generator=g).to(dev) for c, u in zip(cs, ups)]
    wt = (torch.randn(cout, sum(cs), 3, 3, generator=g) / (sum(cs) * 9) ** 0.5).to(dev)
    b = torch.randn(cout, generator=g).to(dev)
    up2 = [bool(u) for u in ups]
    packed = [hip.spk_pack(x) for x in srcs]
    L = hip.lib()
    res = {}
    try:
        L.fldr_debug_spk_small_units(-1)                    # (keep the small launches on the kernels under test)
        for r32 in (0, 2):                                  # never / wherever it applies (1 = by its cost model)
            assert L.fldr_debug_ring32(r32) == r32
            res[min(r32, 1)] = hip.conv2d_spk(packed, wt, b, relu=relu, up2=up2, want_f32=False, want_spk=True).float()
    finally:
        L.fldr_debug_ring32(1)
        L.fldr_debug_spk_small_units(96)
    assert L.fldr_debug_ring_timeouts() == 0
    scale = float(res[0].abs().max())
    _cmp(res[1], res[0], atol=3e-6 * scale + 1e-7, what="ring32 vs 16x16x32 ring")
    xs = [p_.float().double().cpu() for p_ in packed]
    xs = [F.interpolate(x, scale_factor=2, mode="nearest") if u else x for x, u in zip(xs, ups)]
    ref = F.conv2d(torch.cat(xs, 1), wt.double().cpu(), b.double().cpu(), padding=1)
    ref = F.relu(ref) if relu else ref
    e32 = (hip.conv2d(srcs, wt, b, relu=relu, up2=up2, precision="fp32").double().cpu() - F.conv2d(torch.cat([F.interpolate(x.double().cpu(), scale_factor=2, mode="nearest") if u else x.double().cpu() for x, u in zip(srcs, ups)], 1), wt.double().cpu(), b.double().cpu(), padding=1).clamp(min=0 if relu else -1e30)).abs().mean().item()
    e_r32 = (res[1].double().cpu() - ref).abs().mean().item()
    # the packed output itself rounds to 22 bits: allow that on top of the exact-fp32 kernel's accumulation error
    assert e_r32 <= 1.5 * e32 + 2.0 ** -22 * float(ref.abs().mean()) + 1e-9, (e_r32, e32)


@pytest.mark.parametrize("shape", [(16, 32, 50, 70, 2), (16, 32, 144, 240, 1), (32, 32, 68, 120, 1), (32, 32, 272, 96, 2), (40, 24, 30, 44, 1), (8, 20, 18, 34, 1),
                                   (24, 32, 40, 72, 1), (32, 32, 576, 960, 1)])
def test_stride2_lds_dma_kernel(hip, dev, shape, hooks):
    """The LDS-DMA packed-source stride-2 kernel (records straight into LDS, taps outer / channels inner; 17..32 output channels: enc2,
    enc3's halves) against the register-staged kernel it replaces and against fp64: equal to fp32 accumulation rounding (other summation
    order), not less accurate; fp32 and packed outputs, single and pair launches, partial tiles, one group (cin 8) up to five (cin 40),
    many rounds of workgroups, batch of 2."""
    cin, cout, H, W, N = shape
    g = _gen(91)
    x = F.relu(torch.randn(N, cin, H, W, generator=g)).to(dev) * 3
    wt = (torch.randn(cout, cin, 4, 4, generator=g) / (cin * 16) ** 0.5).to(dev)
    wt2 = (torch.randn(cout, cin, 4, 4, generator=g) / (cin * 16) ** 0.5).to(dev)
    b, b2 = torch.randn(cout, generator=g).to(dev), torch.randn(cout, generator=g).to(dev)
    xp = hip.spk_pack(x)
    L = hip.lib()
    res = {}
    try:
        for dma in (0, 1):
            assert L.fldr_debug_s2_dma(dma) == dma
            o32, op = hip.conv2d_s2_spk(xp, wt, b, relu=True, want_f32=True, want_spk=True)
            pa, pb = hip.conv2d_s2_spk_pair(xp, [(wt, b), (wt2, b2)], relu=False)
            only = hip.conv2d_s2_spk(xp, wt, b, relu=True, want_f32=False, want_spk=True)
            assert torch.equal(hip.spk_pack(o32).buf, op.buf) and torch.equal(only.buf, op.buf)
            res[dma] = (o32, pa.float(), pb.float())
    finally:
        L.fldr_debug_s2_dma(1)
    for a_, b_ in zip(res[0], res[1]):
        _cmp(b_, a_, atol=2e-6 * float(a_.abs().max()) + 1e-7, what="LDS-DMA kernel vs register-staged kernel")
    xv = xp.float().double().cpu()
    ref = F.relu(F.conv2d(xv, wt.double().cpu(), b.double().cpu(), stride=2, padding=1))
    e0, e1 = (res[0][0].double().cpu() - ref).abs().mean().item(), (res[1][0].double().cpu() - ref).abs().mean().item()
    assert e1 <= 1.25 * e0 + 1e-9, (e1, e0)
    ref2 = F.conv2d(xv, wt2.double().cpu(), b2.double().cpu(), stride=2, padding=1)
    assert (res[1][2].double().cpu() - ref2).abs().max().item() <= 3e-6 * float(ref2.abs().max()) + 1e-7


@pytest.mark.parametrize("case", [(96, 96, True, True), (96, 96, True, False), (48, 16, False, False), (64, 40, True, True)])
def test_multi_level_conv_launch(hip, dev, case):
    """fldr_conv2d_spk_levels (rec_ctx_ds over the pyramid levels in one launch, fLDRnet.py:148-162): the bits of the per-level
    launches — fp32 and packed outputs, with and without the residual — for level sizes from one partial tile to several rounds
    of workgroups, not multiples of the 8 x 32 tile."""
    cin, cout, relu, res = case
    g = _gen(77)
    sizes = [(72, 120), (36, 60), (18, 30), (9, 15), (5, 33), (1, 1)]
    xs = [torch.randn(1, cin, h, w, generator=g).to(dev) for h, w in sizes]
    wt = (torch.randn(cout, cin, 3, 3, generator=g) / 20).to(dev)
    b = torch.randn(cout, generator=g).to(dev)
    rs = [torch.randn(1, cout, h, w, generator=g).to(dev) for h, w in sizes] if res else None
    got = hip.conv2d_spk_levels(xs, wt, b, relu=relu, residuals=rs, want_f32=True, want_spk=True)
    for l, x in enumerate(xs):
        r32, rsp = hip.conv2d_spk([x], wt, b, relu=relu, residual=rs[l] if res else None, want_f32=True, want_spk=True)
        assert torch.equal(got[l][0], r32), (l, sizes[l])
        assert torch.equal(got[l][1].buf, rsp.buf), (l, sizes[l])
    only = hip.conv2d_spk_levels([o[1] for o in got], wt[:, :cout] if cout <= cin else (torch.randn(cout, cout, 3, 3, generator=g) / 20).to(dev), None,
                                 want_f32=False, want_spk=True) if cout % 8 == 0 else None      # chained through the packed outputs
    if only is not None:
        assert all(o.shape == (1, cout, h, w) for o, (h, w) in zip(only, sizes))


@pytest.mark.parametrize("case", [(96, 96, (72, 120)), (48, 40, (19, 45)), (32, 16, (8, 32))])
def test_conv_split_packed_residual(hip, dev, case):
    """Round 4: the residual of fldr_conv2d_spk[_levels] given as a split-packed tensor (rec_ctx_ds.2 adds the PCA features, which
    then exist packed only).  The kernel adds hi + lo: (1) with an fp32 residual that IS hi + lo (unpack(pack(x))) the outputs are the
    bits of the fp32-residual call, single launch and multi-level launch; (2) with an arbitrary fp32 x in [-1, 1] the result differs
    from the fp32-residual one by at most 2^-22 |x| + the output's own rounding (asserted: 2.4e-7 + 1 ulp)."""
    cin, cout, (h, w) = case
    g = _gen(91)
    sizes = [(h, w), (max(h // 2, 1), max(w // 2, 1)), (3, 5)]
    xs = [torch.randn(1, cin, a, b, generator=g).to(dev) for a, b in sizes]
    wt = (torch.randn(cout, cin, 3, 3, generator=g) / 20).to(dev)
    bias = torch.randn(cout, generator=g).to(dev)
    raw = [(torch.rand(1, cout, a, b, generator=g) * 2 - 1).to(dev) for a, b in sizes]
    packed = [hip.spk_pack(r) for r in raw]
    exact = [p.float() for p in packed]                                     # hi + lo as fp32: exactly what the kernel adds
    for l, x in enumerate(xs):
        assert (exact[l] - raw[l]).abs().max().item() <= 2.4e-7
        a32, asp = hip.conv2d_spk([x], wt, bias, relu=True, residual=exact[l], want_f32=True, want_spk=True)
        b32, bsp = hip.conv2d_spk([x], wt, bias, relu=True, residual=packed[l], want_f32=True, want_spk=True)
        assert torch.equal(a32, b32) and torch.equal(asp.buf, bsp.buf), l
        only = hip.conv2d_spk([x], wt, bias, relu=True, residual=packed[l], want_f32=False, want_spk=True)   # no fp32 output needed
        assert torch.equal(only.buf, bsp.buf)
        c32, _ = hip.conv2d_spk([x], wt, bias, relu=True, residual=raw[l], want_f32=True, want_spk=True)
        assert (c32 - b32).abs().max().item() <= 2.4e-7 + 1.2e-7 * float(c32.abs().max())
    lv_a = hip.conv2d_spk_levels(xs, wt, bias, relu=True, residuals=exact, want_f32=True, want_spk=True)
    lv_b = hip.conv2d_spk_levels(xs, wt, bias, relu=True, residuals=packed, want_f32=True, want_spk=True)
    for (a32, asp), (b32, bsp) in zip(lv_a, lv_b):
        assert torch.equal(a32, b32) and torch.equal(asp.buf, bsp.buf)


@pytest.mark.parametrize("shape", [([3, 3, 2, 5], 16, 40, 72, 1), ([16], 32, 34, 70, 2), ([32], 64, 48, 64, 1), ([26], 16, 50, 38, 1)])
def test_stride2_split_conv_is_fp32_equivalent(hip, dev, shape):
    """The 3 x fp16-split stride-2 4x4 convolution (UNet encoders) against an fp64 reference: error at the level of the exact
    fp32-MFMA kernel; its split-packed twin equals fldr_spk_pack of its fp32 output."""
    parts, cout, H, W, N = shape
    g = _gen(51)
    srcs = [torch.randn(N, c, H, W, generator=g) for c in parts]
    cin = sum(parts)
    wt = torch.randn(cout, cin, 4, 4, generator=g) / (cin * 16) ** 0.5
    bs = torch.randn(cout, generator=g)
    ref = F.relu(F.conv2d(torch.cat(srcs, 1).double(), wt.double(), bs.double(), stride=2, padding=1))
    dsrc = [s.to(dev) for s in srcs]
    a32 = hip.conv2d(dsrc, wt.to(dev), bs.to(dev), stride=2, relu=True, precision="fp32").double().cpu()
    sp, spk = hip.conv2d(dsrc, wt.to(dev), bs.to(dev), stride=2, relu=True, precision="split", want_spk=True)
    assert torch.equal(hip.spk_pack(sp).buf, spk.buf)
    e32, esp = (a32 - ref).abs(), (sp.double().cpu() - ref).abs()
    print("cin %3d cout %2d: mean|err| fp32-MFMA %.2e split %.2e ; max %.2e / %.2e" % (cin, cout, e32.mean(), esp.mean(), e32.max(), esp.max()))
    assert esp.mean() <= 1.5 * e32.mean() + 1e-8 and esp.max() <= 2.0 * e32.max() + 1e-7


@pytest.mark.parametrize("shape", [([3, 3, 2, 5], 16, 40, 72, 1), ([16], 32, 34, 70, 2), ([26], 16, 50, 38, 3), ([5], 16, 18, 66, 1),
                                   ([4], 1, 34, 64, 1), ([1, 3], 17, 10, 66, 2), ([2, 1], 5, 130, 6, 1), ([3, 2], 16, 20, 600, 1)])
def test_stride2_persistent_kernel_bit_identical_to_per_tile(hip, dev, shape, hooks):
    """The persistent stride-2 kernel (weights resident in LDS, inputs requested two iterations ahead) against the per-tile
    kernel it replaces for enc1 / enc2: same operand layout and MFMA order => identical fp32 and split-packed outputs;
    partial tiles, several samples, multi-source concatenation."""
    parts, cout, H, W, N = shape
    g = _gen(23)
    srcs = [(torch.rand(N, c, H, W, generator=g) * 2 - 1).to(dev) for c in parts]
    wt = ((torch.rand(cout, sum(parts), 4, 4, generator=g) - 0.5) / 4).to(dev)
    b = (torch.rand(cout, generator=g) - 0.5).to(dev)
    outs = []
    try:
        # per-tile kernel; persistent with the automatic / forced tile-grid shifts, 16-byte staging loads (odd shifts, widths that
        # are multiples of 4) and the 4-byte path
        for mode, shift, v4 in ((0, -1, 1), (1, -1, 1), (1, 0, 1), (1, 15, 1), (1, 31, 1), (1, 15, 0), (1, 3, 1)):
            hip.lib().fldr_debug_s2_persistent(mode)
            hip.lib().fldr_debug_s2_xshift(shift)
            hip.lib().fldr_debug_s2_vec4(v4)
            o, sp = hip.conv2d(srcs, wt, b, stride=2, relu=True, precision="split", want_spk=True)
            outs.append((o.clone(), sp.buf.clone()))
    finally:
        hip.lib().fldr_debug_s2_persistent(1)
        hip.lib().fldr_debug_s2_xshift(-1)
        hip.lib().fldr_debug_s2_vec4(1)
    for k in range(1, len(outs)):
        assert torch.equal(outs[0][0], outs[k][0]) and torch.equal(outs[0][1], outs[k][1]), k
    # the packed twin is the split of the fp32 output, padding channels of the last group included (zeros, never
    # uninitialised memory: a later convolution multiplies them by zero weights, and NaN * 0 is NaN)
    assert torch.equal(hip.spk_pack(outs[1][0]).buf, outs[1][1])


def test_splat_and_correlation_backward(hip, oracle, dev):
    """fldr_softsplat_bwd / fldr_correlation_bwd against the oracle's restatement of the reference's backward kernels, and
    autograd through FunctionSoftsplat / FunctionCorrelation (the training-side use of the operators)."""
    import softSplat
    from OpticalFlow import correlation
    g = _gen(41)
    x = torch.rand(2, 5, 37, 70, generator=g) * 2 - 1
    flow = (torch.rand(2, 2, 37, 70, generator=g) - 0.5) * 12
    go = torch.randn(2, 5, 37, 70, generator=g)
    gi, gf = hip.softsplat_bwd(x.to(dev), flow.to(dev), go.to(dev))
    ri, rf = oracle.splat_backward(x, flow, go)
    _cmp(gi, ri, atol=2e-6, rtol=1e-5, what="splat gradInput")
    _cmp(gf, rf, atol=3e-5, rtol=1e-5, what="splat gradFlow")
    # autograd through the composed softmax splat == autograd through the oracle's forward restatement
    xd, fd = x.to(dev).requires_grad_(True), flow.to(dev).requires_grad_(True)
    zd = torch.randn(2, 1, 37, 70, generator=g)
    zg = zd.to(dev).requires_grad_(True)
    out = softSplat.FunctionSoftsplat(xd, fd, zg, "softmax")
    w = torch.randn(out.shape, generator=g)
    (out * w.to(dev)).sum().backward()
    xc, fc, zc = x.clone().requires_grad_(True), flow.clone().requires_grad_(True), zd.clone().requires_grad_(True)
    (oracle.function_softsplat(xc, fc, zc, "softmax") * w).sum().backward()
    _cmp(xd.grad, xc.grad, atol=3e-5, rtol=1e-4, what="d softsplat / d input")
    _cmp(zg.grad, zc.grad, atol=3e-5, rtol=1e-4, what="d softsplat / d metric")
    _cmp(fd.grad, fc.grad, atol=2e-3, rtol=2e-3, what="d softsplat / d flow")     # fp32 chain through the normalisation; the oracle sums in fp64
    a = torch.randn(2, 7, 21, 33, generator=g)
    b = torch.randn(2, 7, 21, 33, generator=g)
    gc = torch.randn(2, 81, 21, 33, generator=g)
    ga, gb = hip.correlation_bwd(a.to(dev), b.to(dev), gc.to(dev))
    ra, rb = oracle.correlation_backward(a, b, gc)
    _cmp(ga, ra, atol=3e-6, rtol=1e-5, what="correlation gradFirst")
    _cmp(gb, rb, atol=3e-6, rtol=1e-5, what="correlation gradSecond")
    ad, bd = a.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    (correlation.FunctionCorrelation(ad, bd) * gc.to(dev)).sum().backward()
    _cmp(ad.grad, ra, atol=3e-6, rtol=1e-5, what="autograd correlation first")
    _cmp(bd.grad, rb, atol=3e-6, rtol=1e-5, what="autograd correlation second")


@pytest.mark.parametrize("mode", ["summation", "average", "linear", "softmax"])
@pytest.mark.parametrize("shape", [(2, 4, 33, 70, 9.0), (1, 3, 70, 300, 40.0), (1, 13, 40, 130, 600.0)])
def test_tile_softsplat_matches_oracle(hip, oracle, dev, mode, shape, hooks):
    """The destination-owned (LDS tile) splat, opt-in via FLDR_SPLAT=tile: the same operator without global atomics.
    Flows range from coherent to wild (600 px: every tile falls back to the full block scan or the queue path)."""
    N, C, H, W, amp = shape
    g = _gen(11)
    x = torch.rand(N, C, H, W, generator=g) * 2 - 1
    flow = (torch.rand(N, 2, H, W, generator=g) - 0.5) * amp
    z = torch.randn(N, 1, H, W, generator=g) if mode in ("linear", "softmax") else None
    if mode == "linear":
        z = z.abs() + 0.1
    out = hip.softsplat_fused(x.to(dev), flow.to(dev), None if z is None else z.to(dev), mode, kernel="tile")
    _cmp(out, oracle.function_softsplat(x, flow, z, mode), atol=3e-5, rtol=1e-5, what="tile " + mode)


@pytest.mark.parametrize("mode", ["summation", "average", "linear", "softmax"])
@pytest.mark.parametrize("shape", [(2, 48, 33, 70, 3.0, "smooth"), (1, 48, 36, 60, 9.0, "random"), (1, 13, 40, 130, 80.0, "random"),
                                   (1, 3, 17, 16, 600.0, "random"), (1, 48, 72, 120, 30.0, "smooth")])
def test_gather_softsplat_matches_oracle(hip, oracle, dev, mode, shape):
    """fldr_softsplat_gather (deterministic gather formulation used for the warped features, fLDRnet.py:386-387) against
    the oracle: two (image, flow) problems per call, sources as channel slices of a larger tensor, smooth flows of
    several pixels (the video case), random flows up to far beyond the map (every tile reaches every tile), all four
    modes with and without a metric; fp32 and split-packed outputs; bitwise run-to-run determinism."""
    N, C, H, W, amp, kind = shape
    g = _gen(17)
    feat = torch.rand(N, 2 * C, H, W, generator=g) * 2 - 1
    if kind == "smooth":
        lo = (torch.rand(N, 4, max(H // 8, 2), max(W // 8, 2), generator=g) - 0.5) * amp + torch.tensor([amp, -amp / 2, -amp, amp / 3]).view(1, 4, 1, 1)
        up = F.interpolate(lo, size=(H, W), mode="bilinear", align_corners=False)
    else:
        up = (torch.rand(N, 4, H, W, generator=g) - 0.5) * amp
    z = None
    if mode in ("linear", "softmax"):
        z = [torch.randn(N, 1, H, W, generator=g) for _ in range(2)]
        if mode == "linear":
            z = [t.abs() + 0.1 for t in z]
    fd, ud = feat.to(dev), up.to(dev)
    imgs, flows = [fd[:, C:], fd[:, :C]], [ud[:, :2], ud[:, 2:]]
    zs = None if z is None else [t.to(dev) for t in z]
    res = hip.softsplat_gather(imgs, flows, zs, mode, want_f32=True, want_spk=True)
    res2 = hip.softsplat_gather(imgs, flows, zs, mode, want_f32=True, want_spk=True)
    for k in range(2):
        ref = oracle.function_softsplat(feat[:, C:] if k == 0 else feat[:, :C], up[:, :2] if k == 0 else up[:, 2:],
                                        None if z is None else z[k], mode)
        _cmp(res[k][0], ref, atol=3e-5, rtol=1e-5, what="gather %s dir %d" % (mode, k))
        assert torch.equal(res[k][0], res2[k][0]) and torch.equal(res[k][1].buf, res2[k][1].buf)      # deterministic
        assert torch.equal(hip.spk_pack(res[k][0]).buf, res[k][1].buf)                                 # packed twin
    if mode == "softmax" and z is not None:                      # metric None = weight 1 (the feature splats of the model)
        one = hip.softsplat_gather(imgs[:1], flows[:1], None, mode, want_f32=True, want_spk=False)[0]
        _cmp(one, oracle.function_softsplat(feat[:, C:], up[:, :2], None, mode), atol=3e-5, rtol=1e-5, what="gather softmax, no metric")


@pytest.mark.parametrize("mode", ["summation", "average", "linear", "softmax"])
@pytest.mark.parametrize("shape", [(2, 4, 33, 70, 9.0), (1, 3, 70, 300, 40.0), (1, 13, 40, 130, 600.0), (2, 3, 130, 190, 3.0), (1, 48, 36, 60, 9.0)])
def test_acc64_softsplat_matches_oracle(hip, oracle, dev, mode, shape):
    """fldr_softsplat_acc64 (destination-owned tiles, fp64 LDS atomics: the default splat since round 3) against the oracle:
    image (<= 3 channels) and 16-channel-group configurations, coherent to wild flows (600 px: every block of these maps matches
    every tile; they have at most 99 blocks, so the 512-entry queue does not overflow here — tests/test_gpu_splat_ops.py reaches
    the overflow walks), all four modes; run-to-run identical."""
    N, C, H, W, amp = shape
    g = _gen(12)
    x = torch.rand(N, C, H, W, generator=g) * 2 - 1
    flow = (torch.rand(N, 2, H, W, generator=g) - 0.5) * amp
    z = torch.randn(N, 1, H, W, generator=g) if mode in ("linear", "softmax") else None
    if mode == "linear":
        z = z.abs() + 0.1
    zs = None if z is None else [z.to(dev)]
    out = hip.softsplat_acc64([x.to(dev)], [flow.to(dev)], zs, mode)[0]
    _cmp(out, oracle.function_softsplat(x, flow, z, mode), atol=3e-5, rtol=1e-5, what="acc64 " + mode)
    assert torch.equal(out, hip.softsplat_acc64([x.to(dev)], [flow.to(dev)], zs, mode)[0])
    # the public operator takes the same path
    import softSplat
    _cmp(softSplat.FunctionSoftsplat(x.to(dev), flow.to(dev), None if z is None else z.to(dev), mode), out, atol=0.0, what="FunctionSoftsplat == acc64")


@pytest.mark.parametrize("mode", ["summation", "average", "linear", "softmax"])
@pytest.mark.parametrize("case", [(2, 3, 96, 200, 5.0, "smooth"), (1, 3, 70, 132, 3.0, "random"), (1, 2, 150, 260, 600.0, "random"),
                                  (1, 3, 40, 48, 2.0, "smooth"), (1, 3, 130, 256, 40.0, "outliers")])
def test_acc64_image_walk_of_pixel_runs(hip, hooks, oracle, dev, mode, case):
    """The image configuration's walk by runs of four adjacent source pixels (16-byte loads, neighbouring pixels' shared corners
    summed in registers, de-interleaved accumulator rows) against the oracle and against the one-pixel-per-item walk: smooth flows
    (every hand-off taken), random ones (almost none), 600 px (every one of the map's 190 blocks matches every tile: the rectangle
    walk over the whole map, no queue overflow — that needs more than 512 blocks, tests/test_gpu_splat_ops.py), maps small enough
    for the table-free walk, and a smooth field with 1 % of the vectors thrown to +-3e9 px (block-queue walk)."""
    N, C, H, W, amp, kind = case
    g = _gen(77)
    x = torch.rand(N, C, H, W, generator=g) * 2 - 1
    if kind == "random":
        flow = (torch.rand(N, 2, H, W, generator=g) - 0.5) * amp
    else:
        lo = (torch.rand(N, 2, max(H // 8, 2), max(W // 8, 2), generator=g) - 0.5) * amp + torch.tensor([amp, -amp / 2]).view(1, 2, 1, 1)
        flow = F.interpolate(lo, size=(H, W), mode="bilinear", align_corners=False)
        if kind == "outliers":
            m = torch.rand(N, 1, H, W, generator=g) < 0.01
            flow = torch.where(m, torch.where(torch.rand(N, 2, H, W, generator=g) < 0.5, torch.tensor(3.0e9), torch.tensor(-3.0e9)), flow)
    z = torch.randn(N, 1, H, W, generator=g) if mode in ("linear", "softmax") else None
    if mode == "linear":
        z = z.abs() + 0.1
    zs = None if z is None else [z.to(dev)]
    ref = oracle.function_softsplat(x, flow, z, mode)
    outs = {}
    try:
        for q in (1, 0):
            hooks.fldr_debug_splat_quad(q)
            outs[q] = hip.softsplat_acc64([x.to(dev)], [flow.to(dev)], zs, mode)[0]
            _cmp(outs[q], ref, atol=3e-5, rtol=1e-5, what="acc64 %s, runs of four: %d" % (mode, q))
    finally:
        hooks.fldr_debug_splat_quad(1)
    # the two walks sum the same fp32 products in fp64: equal up to a rounding boundary of the fp32 output (one ulp, rarely)
    d = (outs[0] - outs[1]).abs()
    assert float(d.max()) <= (2.5e-7 if mode != "summation" else 1e-5) and float((d > 0).float().mean()) < 1e-3
    # views with batch / channel strides (the frames of the model), two problems in one launch
    if C == 3:
        fr = torch.stack([x, x.flip(1)], 2).to(dev)                       # [N,3,2,H,W]
        fl2 = [flow.to(dev), (-flow).to(dev)]
        zz = None if z is None else [z.to(dev), z.to(dev)]
        a0, a1 = hip.softsplat_acc64([fr[:, :, 0], fr[:, :, 1]], fl2, zz, mode)
        assert float((a0 - outs[1]).abs().max()) <= (2.5e-7 if mode != "summation" else 1e-5)
        _cmp(a1, oracle.function_softsplat(x.flip(1), -flow, z, mode), atol=3e-5, rtol=1e-5, what="acc64 strided pair, second problem")


@pytest.mark.parametrize("mode", ["summation", "average", "softmax"])
@pytest.mark.parametrize("shape", [(2, 48, 33, 70, 3.0, "smooth"), (1, 48, 36, 60, 9.0, "random"), (1, 13, 40, 130, 80.0, "random"),
                                   (1, 48, 72, 120, 30.0, "smooth"), (1, 48, 9, 15, 2.0, "smooth")])
def test_acc64_softsplat_pair(hip, oracle, dev, mode, shape):
    """Two problems per launch, the way the model calls it (fLDRnet.py:386-387 / :449-450): sources as channel slices of one
    tensor, flows as channel slices of the [N,4,H,W] level flow, fp32 and packed outputs (packed == pack(fp32)), and the
    one-batch-of-two packed form the batched conv_flow1 consumes."""
    N, C, H, W, amp, kind = shape
    g = _gen(19)
    feat = torch.rand(N, 2 * C, H, W, generator=g) * 2 - 1
    if kind == "smooth":
        lo = (torch.rand(N, 4, max(H // 8, 2), max(W // 8, 2), generator=g) - 0.5) * amp + torch.tensor([amp, -amp / 2, -amp, amp / 3]).view(1, 4, 1, 1)
        up = F.interpolate(lo, size=(H, W), mode="bilinear", align_corners=False)
    else:
        up = (torch.rand(N, 4, H, W, generator=g) - 0.5) * amp
    z = [torch.randn(N, 1, H, W, generator=g) for _ in range(2)] if mode == "softmax" else None
    fd, ud = feat.to(dev), up.to(dev)
    imgs, flows = [fd[:, C:], fd[:, :C]], [ud[:, :2], ud[:, 2:]]
    zs = None if z is None else [t.to(dev) for t in z]
    res = hip.softsplat_acc64(imgs, flows, zs, mode, want_f32=True, want_spk=True)
    for k in range(2):
        ref = oracle.function_softsplat(feat[:, C:] if k == 0 else feat[:, :C], up[:, :2] if k == 0 else up[:, 2:],
                                        None if z is None else z[k], mode)
        _cmp(res[k][0], ref, atol=3e-5, rtol=1e-5, what="acc64 pair %s dir %d" % (mode, k))
        assert torch.equal(hip.spk_pack(res[k][0]).buf, res[k][1].buf)                                 # packed twin
    if N == 1:
        pair = hip.softsplat_acc64(imgs, flows, zs, mode, want_f32=False, want_spk=True, spk_batch=True)
        assert pair.shape == (2, C, H, W)
        assert torch.equal(pair.buf.view(torch.int16), torch.cat([res[0][1].buf.view(torch.int16), res[1][1].buf.view(torch.int16)]))


def test_acc64_softsplat_frames_in_place_and_low_res_bounds(hip, oracle, dev):
    """The level-0 call of the model: both image splats in one launch, frames read in place as channel-strided views of the
    [B,3,2,H,W] tensor, metrics given, bounds tables from the low-resolution flows."""
    g = _gen(23)
    B, H, W, up = 2, 128, 192, 8
    frames = (torch.rand(B, 3, 2, H, W, generator=g) * 2 - 1).to(dev)
    lo = (torch.randn(B, 4, H // up, W // up, generator=g) * 1.5).to(dev)
    t4 = torch.tensor([0.5, 0.125]).view(B, 1, 1, 1).to(dev)
    I0, I1 = frames[:, :, 0], frames[:, :, 1]
    ft0 = F.interpolate(t4 * lo[:, 2:], scale_factor=up, mode="bilinear", align_corners=False) * up
    ft1 = F.interpolate((1 - t4) * lo[:, :2], scale_factor=up, mode="bilinear", align_corners=False) * up
    z0 = -torch.rand(B, 1, H, W, generator=g).to(dev) * 3
    z1 = -torch.rand(B, 1, H, W, generator=g).to(dev) * 3
    b0 = hip.splat_bounds_upsampled(lo[:, 2:], t4, 1, up, H, W)
    b1 = hip.splat_bounds_upsampled(lo[:, :2], t4, 2, up, H, W)
    w0, w1 = hip.softsplat_acc64([I0, I1], [ft0, ft1], [z0, z1], "softmax", bounds_ws=[b0, b1])
    _cmp(w0, oracle.function_softsplat(I0.contiguous().cpu(), ft0.cpu(), z0.cpu(), "softmax"), atol=3e-5, what="acc64 I0")
    _cmp(w1, oracle.function_softsplat(I1.contiguous().cpu(), ft1.cpu(), z1.cpu(), "softmax"), atol=3e-5, what="acc64 I1")
    e0, e1 = hip.softsplat_acc64([I0.contiguous(), I1.contiguous()], [ft0, ft1], [z0, z1], "softmax")      # exact bounds pre-pass
    assert torch.equal(e0, w0) and torch.equal(e1, w1)
    bw = hip.splat_bounds_upsampled_pair(lo, t4, "images", up, H, W)                                       # both tables, one launch
    p0, p1 = hip.softsplat_acc64([I0, I1], [ft0, ft1], [z0, z1], "softmax", bounds_ws=bw)
    assert torch.equal(p0, w0) and torch.equal(p1, w1)
    # the feature pair of a level: flow = the x2 upsampling of the previous level's flow (fLDRnet.py:384-387)
    C, h, w = 48, 23, 37
    feat = (torch.rand(1, 2 * C, 2 * h, 2 * w, generator=g) * 2 - 1).to(dev)
    prev = (torch.randn(1, 4, h, w, generator=g) * 2).to(dev)
    upf = hip.resize_bilinear(prev, 2 * h, 2 * w, mul=2.0)
    bwf = hip.splat_bounds_upsampled_pair(prev, None, "features", 2.0, 2 * h, 2 * w)
    a = hip.softsplat_acc64([feat[:, C:], feat[:, :C]], [upf[:, :2], upf[:, 2:]], None, "softmax", bounds_ws=bwf)
    b = hip.softsplat_acc64([feat[:, C:], feat[:, :C]], [upf[:, :2], upf[:, 2:]], None, "softmax")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    _cmp(a[0], oracle.function_softsplat(feat[:, C:].cpu(), upf[:, :2].cpu(), None, "softmax"), atol=3e-5, what="feature pair, low-res bounds")


@pytest.mark.parametrize("shape", [(1, 23, 37, 46, 74), (2, 40, 68, 80, 136), (1, 135, 256, 270, 512), (1, 30, 50, 75, 149)])
def test_fused_resize_and_feature_bounds_bit_identical(hip, dev, shape):
    """fldr_resize_bilinear_spk_bounds (the level flow's upsampling and the tables of the two feature splats in one launch) against the
    two separate launches: fp32 flow, packed twin and both tables bit for bit; ragged sizes and a non-integer ratio included."""
    N, h, w, H, W = shape
    g = _gen(97)
    prev = (torch.randn(N, 4, h, w, generator=g) * 3).to(dev)
    mul = W / w
    up0, sp0 = hip.resize_bilinear_spk(prev, H, W, mul=mul)
    bw0 = hip.splat_bounds_upsampled_pair(prev, None, "features", mul, H, W)
    assert hip.RESIZE_BOUNDS
    up1, sp1, bw1 = hip.resize_bilinear_spk_bounds(prev, H, W, mul=mul)
    assert torch.equal(up0, up1)
    assert torch.equal(sp0.buf.view(torch.int16), sp1.buf.view(torch.int16))
    assert torch.equal(bw0.view(torch.int32), bw1.view(torch.int32))
    with pytest.raises(hip.FldrError):                                  # x4 and beyond: the two entry points
        ws = torch.empty(2 * hip.lib().fldr_softsplat_tile_ws_floats(N, 4 * h, 4 * w), device=dev)
        o = torch.empty(N, 4, 4 * h, 4 * w, device=dev)
        sp = hip._spk_alloc(N, 4, 4 * h, 4 * w, dev)
        hip._check(hip.lib().fldr_resize_bilinear_spk_bounds(prev.data_ptr(), o.data_ptr(), sp.ptr, ws.data_ptr(), N, h, w, 4 * h, 4 * w, 4.0, None),
                   "fldr_resize_bilinear_spk_bounds")


def test_tile_softsplat_extreme_and_smooth_flows(hip, oracle, dev, hooks):
    """Band splat corner cases: a smooth flow field (trimmed candidate walk) with 1 % of the vectors thrown out to
    +-3e9 px (bounds far beyond int range: the block walk takes over where they occur) and a pure sub-pixel shift."""
    g = _gen(41)
    N, C, H, W = 1, 3, 150, 400
    x = torch.rand(N, C, H, W, generator=g) * 2 - 1
    lo = torch.randn(N, 2, 5, 9, generator=g) * 4
    flow = torch.nn.functional.interpolate(lo, size=(H, W), mode="bilinear", align_corners=False) + 7.3
    z = torch.randn(N, 1, H, W, generator=g)
    out = hip.softsplat_fused(x.to(dev), flow.to(dev), z.to(dev), "softmax", kernel="tile")
    _cmp(out, oracle.function_softsplat(x, flow, z, "softmax"), atol=3e-5, rtol=1e-5, what="smooth flow")
    wild = flow.clone()
    m = torch.rand(N, 1, H, W, generator=g) < 0.01
    wild = torch.where(m, torch.where(torch.rand(N, 2, H, W, generator=g) < 0.5, torch.tensor(3.0e9), torch.tensor(-3.0e9)), wild)
    out = hip.softsplat_fused(x.to(dev), wild.to(dev), z.to(dev), "softmax", kernel="tile")
    _cmp(out, oracle.function_softsplat(x, wild, z, "softmax"), atol=3e-5, rtol=1e-5, what="smooth flow with outliers")
    shift = torch.zeros(N, 2, H, W); shift[:, 0] = 0.25; shift[:, 1] = -0.5
    out = hip.softsplat_fused(x.to(dev), shift.to(dev), None, "average", kernel="tile")
    _cmp(out, oracle.function_softsplat(x, shift, None, "average"), atol=3e-5, rtol=1e-5, what="sub-pixel shift")


def test_splat_known_answers(hip, dev):
    import softSplat
    sp = softSplat.Softsplat()
    x = (torch.rand(1, 3, 9, 11, generator=_gen(3)) * 2 - 1).to(dev)
    _cmp(sp(x, torch.zeros(1, 2, 9, 11, device=dev)), x, atol=1e-6, what="zero flow identity")
    flow = torch.zeros(1, 2, 9, 11, device=dev)
    flow[:, 0], flow[:, 1] = 2.0, -1.0
    out = sp(x, flow)
    _cmp(out[..., :8, 2:], x[..., 1:, :9], atol=1e-6, what="integer shift")
    assert (out[..., :, :2] == -1).all() and (out[..., 8, :] == -1).all()            # holes -> -1
    img = torch.zeros(1, 1, 1, 4, device=dev)
    img[0, 0, 0, 0], img[0, 0, 0, 2] = -1.0, 1.0
    fl = torch.zeros(1, 2, 1, 4, device=dev)
    fl[0, 0, 0, 0], fl[0, 0, 0, 2], fl[0, 0, 0, 1] = 1.0, -1.0, 2.0
    z = torch.zeros(1, 1, 1, 4, device=dev)
    z[0, 0, 0, 2] = math.log(3.0)
    assert abs(sp(img, fl, z)[0, 0, 0, 1].item() - 0.5) < 1e-6                       # 1:3 softmax mix


# ---------------------------------------------------------------------------------------------------
# cost volume
# ---------------------------------------------------------------------------------------------------
_CORR_SHAPES = [(2, 16, 20, 28), (1, 81, 13, 45), (2, 196, 9, 15), (1, 3, 64, 96), (1, 37, 40, 100)]


@pytest.mark.parametrize("shape", _CORR_SHAPES)
def test_correlation_matches_oracle(hip, oracle, dev, shape):
    """The cost volume of the PRODUCT library (what ships; no hooks fixture) against the oracle and the known answers."""
    from OpticalFlow import correlation
    assert hip.lib() is not None and not hasattr(hip.lib(), "fldr_debug_corr_variant")      # the product build has no hooks
    g = _gen(4)
    a = torch.randn(*shape, generator=g)
    b = torch.randn(*shape, generator=g)
    out = correlation.FunctionCorrelation(a.to(dev), b.to(dev))
    _cmp(out, oracle.correlation(a, b), atol=2e-6 * math.sqrt(shape[1]) + 1e-6, rtol=1e-5, what="correlation")
    out2 = correlation.ModuleCorrelation()(a.to(dev), a.to(dev))
    _cmp(out2[:, 40], (a * a).mean(1), atol=1e-5, what="centre channel = mean square")
    assert out2[0, 0, 0, 0].item() == 0.0                                           # zero padding


@pytest.mark.parametrize("shape", _CORR_SHAPES)
def test_correlation_stagings_bit_identical(hip, dev, shape, hooks):
    """Test build only: the three stagings (LDS-DMA double buffer with 8- / 16-channel chunks where W % 4 == 0; synchronous
    otherwise) give the same bits — and the same bits as the product library's call."""
    g = _gen(4)
    a = torch.randn(*shape, generator=g).to(dev)
    b = torch.randn(*shape, generator=g).to(dev)
    L = hip.lib()
    try:
        outs = []
        for variant, cc in ((0, 8), (1, 8), (1, 16)):
            L.fldr_debug_corr_variant(variant)
            L.fldr_debug_corr_chunk(cc)
            outs.append(hip.correlation_fwd(a, b))
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    finally:
        L.fldr_debug_corr_variant(1)
        L.fldr_debug_corr_chunk(8)
    prev, hip._lib = hip._lib, hip._load(hip.LIB_PATH, want_hooks=False)             # the product library for one call
    try:
        prod = hip.correlation_fwd(a, b)
    finally:
        hip._lib = prev
    assert torch.equal(prod, outs[1])


# ---------------------------------------------------------------------------------------------------
# PCA projection
# ---------------------------------------------------------------------------------------------------
def test_pca_matches_reference_golden_and_oracle(hip, oracle, weights, golden, dev, model):
    import pca_comp
    m, a = model
    g = golden("ops")
    pl = torch.from_numpy(g["pca_in"])
    out64 = pca_comp.to_pca_diff(pl.to(dev), m.params[0], a, m.Mean8, m.EV8, m.meanVec8)
    assert out64.dtype == torch.float64 and out64.shape == (96, 4, 6)
    _cmp(out64, torch.from_numpy(g["pca_out"]), atol=1e-12, what="to_pca_diff vs reference")
    assert out64.min().item() == -1.0 and out64.max().item() == 1.0
    big = torch.rand(12, 72, 136, generator=_gen(5)) * 2 - 1        # B=2: one global min/max over the batch
    ref = oracle.to_pca_diff(big, weights["Mean8"], weights["EV8"], weights["meanVec8"])
    _cmp(pca_comp.to_pca_diff(big.to(dev), m.params[0], a, m.Mean8, m.EV8, m.meanVec8), ref, atol=1e-12, what="pca f64")
    _cmp(pca_comp.to_pca_diff_f32(big.to(dev), m.params[0], a, m.Mean8, m.EV8, m.meanVec8), ref.float(), atol=0.0,
         what="pca f32 (bit exact after the cast)", max_outlier_frac=1e-4, outlier_atol=2.0 ** -24)   # (at most the last bit of the cast, values in [-1, 1])
    with pytest.raises(Exception, match="not padded right"):
        pca_comp.to_pca_diff(torch.zeros(6, 20, 16, device=dev), m.params[0], a, m.Mean8, m.EV8, m.meanVec8)


# ---------------------------------------------------------------------------------------------------
# backward warp, splat metric, resize
# ---------------------------------------------------------------------------------------------------
def test_bwarp_matches_reference_golden(hip, oracle, golden, dev, model):
    m, _ = model
    g = golden("ops")
    x, flo = torch.from_numpy(g["bwarp_x"]).to(dev), torch.from_numpy(g["bwarp_flo"]).to(dev)
    ill = _bwarp_ill(oracle, x.shape, torch.from_numpy(g["bwarp_flo"]))
    print("bwarp golden: %d of %d pixels within %.0e of the mask threshold" % (int(ill.sum()), ill.numel(), BWARP_BAND))
    _cmp(m.vfinet.bwarp(x, flo, withmask=True), torch.from_numpy(g["bwarp_out"]), atol=1e-5, ill=ill, what="bwarp mask")
    _cmp(m.vfinet.bwarp(x, flo, withmask=False), torch.from_numpy(g["bwarp_out_nomask"]), atol=1e-5, what="bwarp nomask")


def test_bwarp_tscaled_zmetric_resize(hip, oracle, dev):
    g = _gen(6)
    N, H, W = 2, 45, 83
    I0 = torch.rand(N, 3, H, W, generator=g) * 2 - 1
    I1 = torch.rand(N, 3, H, W, generator=g) * 2 - 1
    f10 = (torch.rand(N, 2, H, W, generator=g) - 0.5) * 14
    f01 = (torch.rand(N, 2, H, W, generator=g) - 0.5) * 14
    t = torch.tensor([0.125, 0.7]).view(N, 1, 1, 1)
    # differences beyond the tolerance only where the oracle's mask value sits on the hard threshold (fLDRnet.py:573-574)
    ref = oracle.bwarp(f10 * t, (1 - t) * f01)
    got = hip.bwarp_tscaled(f10.to(dev), f01.to(dev), t.to(dev), "t", "1-t")
    ills = [_bwarp_ill(oracle, f10.shape, (1 - t) * f01), _bwarp_ill(oracle, f01.shape, t * f10), _bwarp_ill(oracle, I1.shape, f01)]
    print("pixels within %.0e of the mask threshold: %s of %d" % (BWARP_BAND, [int(i.sum()) for i in ills], ills[0].numel()))
    # (the warped planes are FLOWS of +-7 px that change by up to 14 between neighbours: 4e-5 is 3e-6 of their range, a sample-position
    # rounding of 1e-6 px times that gradient — the 1e-5 of the unit-range image planes below scaled to the data)
    _cmp(got, ref, atol=4e-5, ill=ills[0], what="flowback_0")
    ref = oracle.bwarp(f01 * (1 - t), t * f10)
    _cmp(hip.bwarp_tscaled(f01.to(dev), f10.to(dev), t.to(dev), "1-t", "t"), ref, atol=4e-5, ill=ills[1], what="flowback_1")
    alpha = -1.894
    zref = torch.mean(alpha * torch.abs(I0 - oracle.bwarp(I1, f01)), dim=1, keepdim=True)
    _cmp(hip.zmetric(I0.to(dev), I1.to(dev), f01.to(dev), alpha), zref, atol=1e-5, ill=ills[2], what="zmetric")
    lo = torch.randn(N, 4, 9, 15, generator=g)
    _cmp(hip.resize_bilinear(lo.to(dev), 18, 30, mul=2.0),
         F.interpolate(lo, size=(18, 30), mode="bilinear", align_corners=False) * 2.0, atol=1e-6, what="resize x2")
    _cmp(hip.resize_bilinear(lo.to(dev), 72, 120, mul=8.0),
         8 * F.interpolate(lo, scale_factor=(8, 8), mode="bilinear", align_corners=False), atol=4e-6, what="resize x8")
    _cmp(hip.resize_bilinear(lo.to(dev), 20, 37), F.interpolate(lo, size=(20, 37), mode="bilinear", align_corners=False),
         atol=4e-6, what="resize ragged")


# ---------------------------------------------------------------------------------------------------
# convolutions
# ---------------------------------------------------------------------------------------------------
CONVS = [  # cin parts, cout, k, stride, relu, residual, cout_store, up2 flags
    ([96], 96, 3, 1, True, True, None, None),            # rec_ctx_ds.2 (+ residual)
    ([48, 48], 48, 3, 1, False, False, None, None),      # conv_flow1 on cat(feat, warped)
    ([48, 48, 4], 96, 3, 1, True, False, None, None),    # conv_flow2.0 on a 100-channel cat
    ([48], 6, 3, 1, False, False, 4, None),              # conv_flow_bottom.8, first 4 channels
    ([48], 4, 3, 1, False, True, None, None),            # conv_flow2.8 + up_flow
    ([3, 3, 3, 3, 2, 2, 2, 2, 3, 3], 16, 4, 2, True, False, None, None),   # enc1 on the 26-channel cat
    ([16], 32, 4, 2, True, False, None, None),           # enc2
    ([32], 64, 4, 2, True, False, None, None),           # enc3
    ([64], 64, 3, 1, True, False, None, None),           # dec0
    ([64, 32], 32, 3, 1, True, False, None, [True, False]),   # dec1: NN x2 + cat
    ([32, 16], 16, 3, 1, True, False, None, [True, False]),   # dec2
    ([16], 6, 3, 1, False, False, None, [True]),              # dec3 on NN x2
]


@pytest.mark.parametrize("spec", CONVS, ids=[str(i) for i in range(len(CONVS))])
@pytest.mark.parametrize("size", [(2, 24, 40), (1, 22, 70)])
def test_conv_matches_torch_fp32(hip, dev, spec, size):
    parts, cout, k, stride, relu, residual, store, up2 = spec
    N, H, W = size
    g = _gen(7)
    up2 = up2 or [False] * len(parts)
    srcs = [torch.rand(N, c, H // 2 if u else H, W // 2 if u else W, generator=g) * 2 - 1 for c, u in zip(parts, up2)]
    cin = sum(parts)
    wt = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)
    bs = torch.randn(cout, generator=g) * 0.1
    full = torch.cat([F.interpolate(s, scale_factor=2, mode="nearest") if u else s for s, u in zip(srcs, up2)], 1)
    ref = F.conv2d(full, wt, bs, stride=stride, padding=1)
    if relu:
        ref = F.relu(ref)
    if store:
        ref = ref[:, :store]
    res = torch.rand(ref.shape, generator=g) if residual else None
    if residual:
        ref = ref + res
    got = hip.conv2d([s.to(dev) for s in srcs], wt.to(dev), bs.to(dev), stride=stride, relu=relu,
                     residual=res.to(dev) if residual else None, cout_store=store, up2=up2)
    _cmp(got, ref, atol=2e-5, rtol=1e-5, what="conv %s" % (spec,))


def test_conv_batch_strided_views(hip, dev):
    g = _gen(8)
    feat = (torch.rand(2, 96, 12, 20, generator=g) * 2 - 1)
    wt = torch.randn(48, 96, 3, 3, generator=g) / 30
    fd = feat.to(dev)
    got = hip.conv2d([fd[:, 48:], fd[:, :48]], wt.to(dev), None)
    _cmp(got, F.conv2d(torch.cat([feat[:, 48:], feat[:, :48]], 1), wt, None, padding=1), atol=2e-5, what="strided views")


# ---------------------------------------------------------------------------------------------------
# synthesis tail
# ---------------------------------------------------------------------------------------------------
def test_synth_tail_fp64(hip, dev):
    g = _gen(9)
    N, H, W = 2, 19, 33
    refine = torch.randn(N, 6, H, W, generator=g) * 3
    cands = [torch.rand(N, 3, H, W, generator=g) * 2 - 1 for _ in range(6)]
    t = torch.tensor([[0.125], [0.625]])
    T = torch.tensor([1.5616], dtype=torch.float64)
    occ = F.softmax(refine / T, dim=1)
    t4 = t.view(N, 1, 1, 1)
    wk = [(1 - t4), t4] * 3
    num = sum(wk[k] * occ[:, k:k + 1] * cands[k] for k in range(6))
    den = sum(wk[k] * occ[:, k:k + 1] for k in range(6))
    out = hip.synth_tail(refine.to(dev), [c.to(dev) for c in cands], t.to(dev), float(T))
    assert out.dtype == torch.float64
    _cmp(out, num / den, atol=1e-13, what="tail fp64")
    out32 = hip.synth_tail(refine.to(dev), [c.to(dev) for c in cands], t.to(dev), float(T), out_dtype=torch.float32)
    _cmp(out32, (num / den).float(), atol=1e-7, what="tail fp32 out")


# ---------------------------------------------------------------------------------------------------
# whole frame-pair forward vs the reference's golden vectors
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["model_256x256_t0500", "model_200x500_t0125"])
def test_model_matches_reference_golden(hip, oracle, golden, dev, model, case):
    import fldr_harness as Hn
    m, a = model
    g = golden(case)
    u8 = torch.from_numpy(g["frames_u8"])
    frames = Hn.frames_from_uint8(u8).to(dev)
    t = torch.tensor([[float(g["t"])]], device=dev)
    pyr = Hn.build_pyramid(Hn.pad_frames(frames, a), a)
    for i in range(1, 6):
        _cmp(pyr[i], torch.from_numpy(g["pyr%d" % i]), atol=2e-6, what="pyramid %d" % i)
    # stage boundaries, driven exactly like DCTXVFInet.forward does
    flow = None
    with torch.no_grad():
        for level in range(5, 0, -1):
            B, _, _, h, w = pyr[level].shape
            import pca_comp
            pca = pca_comp.to_pca_diff_f32(pyr[level].reshape(6, h, w), m.params[level], a, m.Mean8, m.EV8, m.meanVec8)
            _cmp(pca.view(1, 96, h // 8, w // 8), torch.from_numpy(g["pca%d" % level]), atol=2e-6, what="pca L%d" % level)
            feat = m.extract_features(pca.view(1, 96, h // 8, w // 8))
            _cmp(feat, torch.from_numpy(g["feat%d" % level]), atol=2e-5, what="feat L%d" % level)
            flow = m.vfinet(feat, flow, t.view(1, 1, 1, 1), level=level, is_training=False, normInput=pyr[level])
            _cmp(flow, torch.from_numpy(g["flow%d" % level]), atol=2e-4, rtol=1e-4, what="flow L%d" % level)
        out = Hn.interpolate(m, a, frames, t, pyramid=pyr)
        # the forward's own feature path (round 4): PCA features split-packed only, rec_ctx_ds of all levels in two launches, the
        # second one adding the features back from the packed tensor (hi + lo) — against the reference's features of every level
        import pca_comp
        _, pcs = pca_comp.to_pca_diff_f32_pyramid([pyr[i].reshape(6, pyr[i].shape[3], pyr[i].shape[4]) for i in range(6)], m.params, a,
                                                  m.Mean8, m.EV8, m.meanVec8, want_spk=True, want_f32=False)
        pp = [hip.Spk(pcs[i].buf, (1, 96, pyr[i].shape[3] // 8, pyr[i].shape[4] // 8)) for i in range(6)]
        c0, c2 = m.rec_ctx_ds[0], m.rec_ctx_ds[2]
        ys = hip.conv2d_spk_levels(pp, c0.weight, c0.bias, relu=True, want_f32=False, want_spk=True)
        fl = hip.conv2d_spk_levels(ys, c2.weight, c2.bias, relu=True, residuals=pp, want_f32=True, want_spk=True)
        for level in range(1, 6):
            _cmp(fl[level][0], torch.from_numpy(g["feat%d" % level]), atol=2e-5, what="feat L%d, packed residual" % level)
    assert out.dtype == torch.float64
    H, W = frames.shape[3:]
    ref = torch.from_numpy(g["out"]).double()[:, :, :H, :W]
    err = _cmp(out, ref, atol=2e-5, what="final frame")
    p = Hn.psnr(Hn.to_uint8_image(ref[0]), Hn.to_uint8_image(out[0]))
    print("%s: max|err| %.2e, PSNR(8-bit) gpu vs reference %.1f dB" % (case, err, p))
    assert p > 90.0


def test_flow_levels_with_identity_splat_match_reference_golden(hip, golden, dev, model, monkeypatch):
    """The one whole-pyramid vector of the reference that has NO restated splat inside (tests/golden/flows_identity_splat_256x256.npz,
    tools/make_golden.py: identity_splat_case — the reference's own model run with its CUDA-only splat replaced by the identity): flow
    levels 5..1 from the reference's features through the HIP path — resize kernels, conv_flow_bottom, the paired conv_flow1 launch,
    conv_flow2 with its flow residual, shipped weights — with the feature splat of this package replaced by the same identity.
    Pins everything around the splat against reference-executed numbers only (the other model goldens carry the ORACLE's splat)."""
    m, _ = model
    g, gi = golden("model_256x256_t0500"), golden("flows_identity_splat_256x256")
    calls = []

    def identity_splat(xs, flows, zs, mode, want_f32=True, want_spk=False, spk_batch=False, bounds_ws=None):
        assert want_spk and not want_f32 and zs is None and mode == "softmax" and len(xs) == 2
        calls.append(tuple(xs[0].shape))
        if spk_batch:
            return hip.spk_pack(torch.cat([x.contiguous() for x in xs], 0))
        return tuple(hip.spk_pack(x.contiguous()) for x in xs)
    monkeypatch.setattr(hip, "softsplat_acc64", identity_splat)
    flow = None
    with torch.no_grad():
        for level in range(5, 0, -1):
            feat = torch.from_numpy(g["feat%d" % level]).to(dev)
            flow = m.vfinet.estimate_flow(feat, flow)
            _cmp(flow, torch.from_numpy(gi["flow%d" % level]), atol=2e-4, rtol=1e-4, what="identity-splat flow L%d" % level)
    assert len(calls) == 4                                                  # levels 4..1 splat; level 5 is conv_flow_bottom


# ---------------------------------------------------------------------------------------------------
# the REFERENCE's stand-alone stage vectors (tests/golden/ops.npz, tools/make_golden.py op_cases) on the HIP stacks with the SHIPPED
# weights — the magnitudes the fp16 split's pre-scaling and range guard actually see (the per-layer tests above use random weights)
# ---------------------------------------------------------------------------------------------------
def test_rec_ctx_ds_matches_reference_golden(hip, golden, dev, model):
    """rec_ctx_ds(x) + x (fLDRnet.py:44-49,162) of the reference on its own input vector."""
    m, _ = model
    g = golden("ops")
    err = _cmp(m.extract_features(torch.from_numpy(g["feat_in"]).to(dev)), torch.from_numpy(g["rec_ctx_ds_out"]), atol=2e-5, rtol=1e-5,
               what="rec_ctx_ds vs reference")
    print("rec_ctx_ds vs reference: max|err| %.2e (|ref| <= %.1f)" % (err, float(np.abs(g["rec_ctx_ds_out"]).max())))
    hip.check_range()


def test_conv_flow_bottom_matches_reference_golden(hip, golden, dev, model):
    """conv_flow_bottom (fLDRnet.py:318-327,379-380): five layers, the first four outputs of the last one."""
    m, _ = model
    g = golden("ops")
    f = torch.from_numpy(g["feat_in"]).to(dev)
    got = m.vfinet.estimate_flow(f, None)
    assert got.shape == (1, 4, 20, 28)
    err = _cmp(got, torch.from_numpy(g["conv_flow_bottom_out"][:, :4]), atol=2e-5, rtol=1e-5, what="conv_flow_bottom vs reference")
    print("conv_flow_bottom vs reference: max|err| %.2e" % err)
    hip.check_range()


def test_conv_flow1_matches_reference_golden(hip, golden, dev, model):
    """conv_flow1 (fLDRnet.py:329,389-390) on a 96-channel vector: as one source, and as the two 48-channel sources the model passes
    (feature half + warped half: the concat is never built)."""
    m, _ = model
    g = golden("ops")
    f = torch.from_numpy(g["feat_in"]).to(dev)
    f1 = m.vfinet.conv_flow1
    ref = torch.from_numpy(g["conv_flow1_out"])
    fp = hip.spk_pack(f)
    one = hip.conv2d_spk([fp], f1.weight, f1.bias)
    two = hip.conv2d_spk([fp.narrow(0, 48), fp.narrow(48, 48)], f1.weight, f1.bias)
    err = _cmp(one, ref, atol=2e-5, rtol=1e-5, what="conv_flow1 vs reference")
    assert torch.equal(one, two)
    print("conv_flow1 vs reference: max|err| %.2e" % err)
    hip.check_range()


def test_conv_flow2_matches_reference_golden(hip, golden, dev, model):
    """conv_flow2 (fLDRnet.py:331-345,391) on the reference's 100-channel vector, fed as the model feeds it: three sources
    (48 + 48 + 4 channels), activations split-packed between the five layers."""
    m, _ = model
    g = golden("ops")
    x = torch.from_numpy(g["flow2_in"]).to(dev)
    ca, cb, up = hip.spk_pack(x[:, :48].contiguous()), hip.spk_pack(x[:, 48:96].contiguous()), x[:, 96:].contiguous()
    got = m.vfinet._chain([ca, cb, hip.spk_pack(up)], m.vfinet.conv_flow2, (0, 2, 4, 6, 8))
    err = _cmp(got, torch.from_numpy(g["conv_flow2_out"]), atol=2e-5, rtol=1e-5, what="conv_flow2 vs reference")
    print("conv_flow2 vs reference: max|err| %.2e" % err)
    hip.check_range()


def test_refine_unet_matches_reference_golden(hip, golden, dev, model):
    """PCARefineUNet.forward (fLDRnet.py:619-644) of the reference on its own 26-channel input, three ways: from the concatenated tensor;
    from the ten source tensors the model passes (never concatenated: enc1 assembles them); and through the product's two-kernel tail
    (dec2 -> packed -> dec3 phase convolutions on the matrix cores, want_refine)."""
    m, _ = model
    g = golden("ops")
    u = torch.from_numpy(g["unet_in"]).to(dev)
    ref = torch.from_numpy(g["unet_out"])
    unet = m.vfinet.refine_unet
    got = unet(u)
    err = _cmp(got, ref, atol=1e-4, rtol=1e-5, what="refine_unet(cat) vs reference")
    parts = [3, 3, 3, 3, 2, 2, 2, 2, 3, 3]
    srcs, c0 = [], 0
    for c in parts:
        srcs.append(u[:, c0:c0 + c].contiguous())
        c0 += c
    assert torch.equal(unet(srcs), got)
    d2p = unet.forward_until_dec2(srcs, packed_out=True)
    cands = [torch.zeros(1, 3, 64, 96, device=dev) for _ in range(6)]
    _, refine = hip.dec3_synth(d2p, unet.dec3.weight, unet.dec3.bias, cands, torch.tensor([[0.5]], device=dev), 1.5616, want_refine=True)
    err2 = _cmp(refine, ref, atol=1e-4, rtol=1e-5, what="dec3 phase convolutions (matrix cores) vs reference")
    print("refine_unet vs reference: max|err| %.2e (generic dec3), %.2e (phase-convolution dec3); |ref| <= %.1f" % (err, err2, float(ref.abs().max())))
    hip.check_range()


@pytest.mark.parametrize("case", ["model_256x256_t0500", "model_200x500_t0125"])
def test_level0_stages_match_reference_golden(hip, oracle, golden, dev, model, case):
    """Level 0 of the reference's own forward, stage by stage on the HIP path with the shipped weights: the level-0 PCA projection and
    features (pca0 / feat0), then — driven exactly like DCTVFInet._synthesise — the 26 planes of the UNet input (fLDRnet.py:480; crops
    of the reference's concat), the two backward-warped frames of the splat metric (im_1_0 / im_0_1, :442-446) and the UNet's output
    (:501; crops).  Differences beyond the tolerance are confined to pixels whose backward-warp mask value sits on its hard threshold
    (computed by the oracle from the flows the GPU itself produced)."""
    import fldr_harness as Hn
    import pca_comp
    m, a = model
    g = golden(case)
    frames = Hn.frames_from_uint8(torch.from_numpy(g["frames_u8"])).to(dev)
    tv = float(g["t"])
    t = torch.tensor([[tv]], device=dev)
    pyr = Hn.build_pyramid(Hn.pad_frames(frames, a), a)
    H, W = pyr[0].shape[3:]
    with torch.no_grad():
        pca0 = pca_comp.to_pca_diff_f32(pyr[0].reshape(6, H, W), m.params[0], a, m.Mean8, m.EV8, m.meanVec8).view(1, 96, H // 8, W // 8)
        feat0 = m.extract_features(pca0)
        has_l0 = "pca0" in g.files                                         # (the 200x500 fixture is stored without its level-0 tensors)
        if has_l0:
            _cmp(pca0, torch.from_numpy(g["pca0"]), atol=2e-6, what="pca L0")
            _cmp(feat0, torch.from_numpy(g["feat0"]), atol=2e-5, what="feat L0")
        # the forward's own (all-level, packed) feature path at level 0 — the loop of test_model_matches_reference_golden stops at level 1
        _, pcs = pca_comp.to_pca_diff_f32_pyramid([pyr[i].reshape(6, pyr[i].shape[3], pyr[i].shape[4]) for i in range(6)], m.params, a,
                                                  m.Mean8, m.EV8, m.meanVec8, want_spk=True, want_f32=False)
        pp = [hip.Spk(pcs[i].buf, (1, 96, pyr[i].shape[3] // 8, pyr[i].shape[4] // 8)) for i in range(6)]
        c0, c2 = m.rec_ctx_ds[0], m.rec_ctx_ds[2]
        ys = hip.conv2d_spk_levels(pp, c0.weight, c0.bias, relu=True, want_f32=False, want_spk=True)
        fl = hip.conv2d_spk_levels(ys, c2.weight, c2.bias, relu=True, residuals=pp, want_f32=True, want_spk=True)
        if has_l0:
            _cmp(fl[0][0], torch.from_numpy(g["feat0"]), atol=2e-5, what="feat L0, packed residual")
        else:
            _cmp(fl[0][0], feat0, atol=1e-6, what="feat L0: packed residual vs fp32 residual")
        flow = None
        for level in range(5, -1, -1):
            h, w = pyr[level].shape[3:]
            pca = pca_comp.to_pca_diff_f32(pyr[level].reshape(6, h, w), m.params[level], a, m.Mean8, m.EV8, m.meanVec8).view(1, 96, h // 8, w // 8)
            flow = m.vfinet.estimate_flow(m.extract_features(pca), flow)
        # --- DCTVFInet._synthesise up to the UNet, tensors kept
        vfi = m.vfinet
        T, za0, za1 = vfi._host_scalars()
        t4 = t.view(1, 1, 1, 1).float()
        I0, I1 = pyr[0][:, :, 0], pyr[0][:, :, 1]
        r = hip.level0_prep(flow, I0, I1, t4, H, W, za0, za1, withmask=True, want_z=True)
        bw = hip.splat_bounds_upsampled_pair(flow, t4, "images", 8, H, W)
        warped0, warped1 = hip.softsplat_acc64([I0, I1], [r["flow_t0"], r["flow_t1"]], [r["z0"], r["z1"]], "softmax", bounds_ws=bw)
        srcs = [I0, I1, warped0, warped1, r["flow_t0"], r["flow_t1"], r["flowback_0"], r["flowback_1"], r["im0_tot"], r["im1_tot"]]
        cat = torch.cat([s.contiguous() for s in srcs], 1)
        refine = vfi.refine_unet(srcs)
        d2p = vfi.refine_unet.forward_until_dec2(srcs, packed_out=True)
        cands = [warped0, warped1, r["im0_tot"], r["im1_tot"], I0, I1]
        out2, refine2 = hip.dec3_synth(d2p, vfi.refine_unet.dec3.weight, vfi.refine_unet.dec3.bias, cands, t4, T, want_refine=True)
        # the metric's backward-warped frames (:443,446): public ops on the x8 flows the prep kernel never stores
        U = lambda f: 8 * F.interpolate(f, scale_factor=(8, 8), mode="bilinear", align_corners=False)
        f10, f01 = U(flow[:, :2].cpu()), U(flow[:, 2:].cpu())
        im_1_0 = hip.bwarp(I1.contiguous(), f01.to(dev))
        im_0_1 = hip.bwarp(I0.contiguous(), f10.to(dev))
    # ill-conditioned pixels of each hard mask, from the GPU's own flows (oracle arithmetic on the CPU)
    tc = tv
    ill_fb0 = _bwarp_ill(oracle, (1, 2, H, W), (1 - tc) * f01)
    ill_fb1 = _bwarp_ill(oracle, (1, 2, H, W), tc * f10)
    ill_im0 = _bwarp_ill(oracle, (1, 3, H, W), r["flowback_0"].cpu()) | ill_fb0
    ill_im1 = _bwarp_ill(oracle, (1, 3, H, W), r["flowback_1"].cpu()) | ill_fb1
    none = torch.zeros(1, 1, H, W, dtype=torch.bool)
    ill26 = torch.cat([none.expand(1, 12, H, W), none.expand(1, 4, H, W), ill_fb0.expand(1, 2, H, W), ill_fb1.expand(1, 2, H, W),
                       ill_im0.expand(1, 3, H, W), ill_im1.expand(1, 3, H, W)], 1)
    ill_m10, ill_m01 = _bwarp_ill(oracle, (1, 3, H, W), f01), _bwarp_ill(oracle, (1, 3, H, W), f10)
    worst = {}
    for ci, (y0, x0, hh, ww) in enumerate(g["crops"]):
        sl = (Ellipsis, slice(int(y0), int(y0 + hh)), slice(int(x0), int(x0 + ww)))
        # planes 12-25 carry flows in pixels of the frame (x8 upsampled): tolerance relative to their magnitude
        worst["cat26"] = max(worst.get("cat26", 0.0), _cmp(cat[sl], torch.from_numpy(g["cat26_crops"][ci]), atol=3e-5, rtol=1e-5, ill=ill26[sl],
                                                           what="UNet input planes, crop %d" % ci))
        worst["im_1_0"] = max(worst.get("im_1_0", 0.0), _cmp(im_1_0[sl], torch.from_numpy(g["im_1_0_crops"][ci]), atol=2e-5, ill=ill_m10[sl], what="im_1_0 crop %d" % ci))
        worst["im_0_1"] = max(worst.get("im_0_1", 0.0), _cmp(im_0_1[sl], torch.from_numpy(g["im_0_1_crops"][ci]), atol=2e-5, ill=ill_m01[sl], what="im_0_1 crop %d" % ci))
        for name, rf in (("refine_out", refine), ("refine_out (phase-convolution dec3)", refine2)):
            worst[name] = max(worst.get(name, 0.0), _cmp(rf[sl], torch.from_numpy(g["refine_out_crops"][ci]), atol=2e-4, rtol=1e-5, what="%s crop %d" % (name, ci)))
    np.testing.assert_allclose(refine.double().sum((0, 2, 3)).cpu().numpy(), g["refine_out_sum"], rtol=1e-5, atol=0.5)
    # the WHOLE 26-plane input, not only its crops: per-plane sum and sum of magnitudes against the reference's (a checksum per plane;
    # allowance: 1e-5 of the plane's magnitude + what its ill-conditioned mask pixels can move: at most |value| <= 16 each)
    cs, ca = cat.double().sum((0, 2, 3)).cpu().numpy(), cat.double().abs().sum((0, 2, 3)).cpu().numpy()
    n_ill = ill26.sum((0, 2, 3)).numpy().astype(np.float64)
    slack = 1e-5 * g["cat26_abssum"] + 0.05 + 16.0 * n_ill
    assert (np.abs(cs - g["cat26_sum"]) <= slack).all(), (np.abs(cs - g["cat26_sum"]), slack)
    assert (np.abs(ca - g["cat26_abssum"]) <= slack).all(), (np.abs(ca - g["cat26_abssum"]), slack)
    worst["cat26 plane sums (rel. to magnitude)"] = float((np.abs(cs - g["cat26_sum"]) / g["cat26_abssum"]).max())
    ref = torch.from_numpy(g["out"]).double()[:, :, :H, :W]
    worst["frame (two-kernel tail)"] = _cmp(out2, ref, atol=2e-5, what="frame from dec3_synth")
    print("%s level 0 vs reference: %s; ill-conditioned mask pixels %d" % (case, ", ".join("%s %.2e" % kv for kv in worst.items()), int(ill26.any(1).sum())))
    hip.check_range()


def test_pairs_in_flight_equal_one_at_a_time(hip, dev, model):
    """bench.py's loop — forwards of DIFFERENT 3840x2160 pairs kept in flight on three HIP streams, eagerly and as hipGraph replays — against
    the same forwards run one at a time: every frame the same bits.  Round 6 found that they were not: with another stream's kernels
    keeping the memory pipeline busy, the last of level0_prep's 24 back-to-back gathers read lanes 48-63 of their offsets from a register
    the compiler had already reused (profiles/r06_prep_gather_hazard.txt) — 16-pixel runs of zeros in im1_tot, 1-6 wrong frames in 12,
    never with one forward at a time, which is what every other test runs.  (Full-size frames: the hazard needs the queue depth and the
    memory traffic of the 4K kernels.)"""
    import fldr_harness as Hn
    m, a = model
    t = torch.tensor([[0.5]], device=dev)
    NS, NP = 3, 4
    frames = [Hn.frames_from_uint8(Hn.synthetic_pair(2160, 3840, seed=40 + p)).to(dev) for p in range(NP)]
    with torch.no_grad():
        pyrs = [Hn.build_pyramid(Hn.pad_frames(f, a), a) for f in frames]
        refs = [Hn.interpolate(m, a, frames[k], t, pyramid=pyrs[k]).clone() for k in range(NP)]
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(device=dev) for _ in range(NS)]
        for rep in range(3):
            for s in streams:
                s.wait_stream(torch.cuda.current_stream())
            outs = []
            for i in range(12):
                with torch.cuda.stream(streams[i % NS]):
                    outs.append((i % NP, Hn.interpolate(m, a, frames[i % NP], t, pyramid=pyrs[i % NP])))
            torch.cuda.synchronize()
            bad = [(i, k, float((o - refs[k]).abs().max())) for i, (k, o) in enumerate(outs) if not torch.equal(o, refs[k])]
            assert not bad, ("eager forwards in flight on 3 streams differ from the one-at-a-time frames", rep, bad)
            del outs
    pools = [torch.cuda.graph_pool_handle() for _ in streams]
    gs = {(s, k): Hn.GraphedInterpolator(m, a, frames[k], t, pyramid=pyrs[k], stream=streams[s], pool=pools[s], check=True) for s in range(NS) for k in range(NP)}
    torch.cuda.synchronize()
    for rep in range(3):
        got = []
        for i in range(24):
            sk = (i % NS, i % NP)
            gs[sk].replay()
            with torch.cuda.stream(streams[sk[0]]):
                got.append((sk[1], gs[sk].out.clone()))
        torch.cuda.synchronize()
        bad = [(i, k, float((o - refs[k]).abs().max())) for i, (k, o) in enumerate(got) if not torch.equal(o, refs[k])]
        assert not bad, ("graph replays in flight on 3 streams differ from the one-at-a-time frames", rep, bad)
        del got
    hip.check_range()


def test_every_stage_beside_every_stage_equals_the_stage_alone(dev, clean_launcher):
    """tools/pairwise_concurrency.py: each of the 12 stages of the 4K forward (+ the two-kernel synthesis) as the victim on one HIP stream beside each
    stage, and beside five busy-partner kernels of the test build (matrix instructions, vector FMAs, scalar adds, LDS reads: csrc/test_partner_kernels.hip),
    on a second stream (different frame pairs), 3 runs per cell: every victim result the same bits as the stage alone.  The whole-forward
    test above samples these overlaps at random; this one walks the matrix (level0_prep beside enc1 / dec1 / dec0 was where round 6's
    defect lived: a packed-fp32 instruction that gfx950 executes wrongly beside another kernel's matrix instructions — the matrix-instruction
    partner made that build fail in 8 of 8 runs)."""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = clean_launcher([sys.executable, os.path.join(root, "tools", "pairwise_concurrency.py"), "1"], env=dict(os.environ), timeout=540)
    assert r["rc"] == 0, (r["rc"], r["stdout"][-2500:], r["stderr"][-1500:])
    assert "TOTAL victim results differing from the stage alone: 0" in r["stdout"]


def test_busy_partner_hook_runs_and_checks_its_arguments(hip, dev):
    """The concurrency tests' partner kernel (test build only: csrc/test_partner_kernels.hip): every kind and register footprint launches and finishes,
    bad arguments come back as FLDR_E_ARG instead of a launch."""
    import ctypes
    out = torch.full((512 * 256,), float("nan"), device=dev)
    for kind in range(5):
        for fp in (0, 1, 5, 9):
            hip.busy_partner(out, 512, 1024, 50, kind + 16 * fp)
    hip.busy_partner(out, 256, 125 * 1024, 50, 1)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    with hip.test_hooks() as L:
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        p = ctypes.c_void_p(out.data_ptr())
        for args in ((None, 512, 1024, 10, 1), (p, 0, 1024, 10, 1), (p, 5000, 1024, 10, 1), (p, 512, 512, 10, 1), (p, 512, 200 * 1024, 10, 1), (p, 512, 1024, -1, 1),
                     (p, 512, 1024, 10, 5), (p, 512, 1024, 10, 1 + 16 * 10), (p, 512, 1024, 10, -1)):
            assert L.fldr_debug_busy_partner(*args, s) == -1, args
    with pytest.raises(ValueError):
        hip.busy_partner(out[:100], 512, 1024, 10, 1)


def test_model_matches_oracle_b2(hip, oracle, weights, dev, model):
    """Batch of 2 (the PCA min/max is then taken over the batch, as in the reference)."""
    import fldr_harness as Hn
    m, a = model
    u = [Hn.synthetic_pair(256, 256, seed=s, quadrant=bool(s)) for s in (0, 1)]
    frames = torch.cat([Hn.frames_from_uint8(x) for x in u], 0)
    t = torch.tensor([[0.25], [0.75]])
    out = Hn.interpolate(m, a, frames.to(dev), t.to(dev))
    with torch.no_grad():
        ref = oracle.forward(weights, oracle.pad_and_pyramid(frames), t)
    err = _cmp(out, ref, atol=1e-4, what="B=2 forward")
    print("B=2: max|err| %.2e" % err)
    assert (out.cpu() - ref).abs().mean().item() <= 1e-6


@pytest.mark.parametrize("case", [(180, 300, 0.3, 3), (264, 520, 0.875, 4), (140, 700, 0.5, 5)])
def test_model_matches_oracle_odd_sizes(hip, oracle, weights, dev, model, case):
    """Frame sizes that are not multiples of the 256-pixel padding unit (reflect padding, partial tiles at every level)."""
    import fldr_harness as Hn
    H, W, tv, seed = case
    m, a = model
    frames = Hn.frames_from_uint8(Hn.synthetic_pair(H, W, seed=seed, quadrant=True))
    t = torch.tensor([[tv]])
    out = Hn.interpolate(m, a, frames.to(dev), t.to(dev))
    assert out.shape[-2:] == (H, W)
    with torch.no_grad():
        ref = oracle.forward(weights, oracle.pad_and_pyramid(frames), t)
    ref = ref[..., :H, :W]
    err = _cmp(out, ref, atol=1e-4, what="forward %dx%d" % (H, W))
    print("%dx%d: max|err| %.2e" % (H, W, err))
    assert (out.cpu() - ref).abs().mean().item() <= 1e-6


@pytest.mark.parametrize("case", [("t0", 0.0, False), ("t1", 1.0, False), ("still", 0.5, True), ("t_eps", 1.0e-3, False)])
def test_model_edge_cases_of_t_and_motion(hip, oracle, weights, dev, model, case):
    """Edge cases of the blend (fLDRnet.py:511-524): t = 0 and t = 1 (half of the six weights are exactly zero: the normalisation rests on
    the other three), t = 1e-3, and two IDENTICAL frames (zero motion: every splat lands on its own cell, every backward-warp mask sits at
    exactly 1) — whole forward against the oracle."""
    import fldr_harness as Hn
    name, tv, still = case
    m, a = model
    u8 = Hn.synthetic_pair(192, 320, seed=9, quadrant=True)
    if still:
        u8 = torch.stack([u8[0], u8[0]], 0)
    frames = Hn.frames_from_uint8(u8)
    t = torch.tensor([[tv]])
    out = Hn.interpolate(m, a, frames.to(dev), t.to(dev))
    with torch.no_grad():
        ref = oracle.forward(weights, oracle.pad_and_pyramid(frames), t)[..., :192, :320]
    err = _cmp(out, ref, atol=1e-4, what="forward, " + name)
    assert (out.cpu() - ref).abs().mean().item() <= 1e-6
    if still:                                                            # zero motion: the interpolated frame is the frame itself, to the network's noise
        assert (out.cpu() - frames[:, :, 0].double()).abs().mean().item() < 2e-2
    print("%s: max|err| %.2e" % (name, err))
    hip.check_range()


def test_model_smallest_frame_and_flow_output(hip, oracle, weights, dev):
    """The smallest frame the reference's reflect padding accepts for the 5-scale path (129 x 131: 127 / 125 padded pixels < the frame),
    and --testgetflowout (fLDRnet.py:407,535: the forward also returns the t-scaled level-0 flows) against the oracle's level-0 flow."""
    import fldr_harness as Hn
    args = Hn.args_config()
    args.testgetflowout = True
    m, _, a = Hn.prepare_model(dev, args=args)
    frames = Hn.frames_from_uint8(Hn.synthetic_pair(129, 131, seed=12))
    t = torch.tensor([[0.25]])
    with torch.no_grad():
        pyr = Hn.build_pyramid(Hn.pad_frames(frames.to(dev), a), a)
        out, flow_out = m([None] * 6, t.to(dev), normInput=pyr, is_training=False, validation=False)
        keep = {}
        ref = oracle.forward(weights, oracle.pad_and_pyramid(frames), t, keep=keep)
    _cmp(out[..., :129, :131], ref[..., :129, :131], atol=1e-4, what="129x131 forward")
    f0 = keep["flows"][0]
    want = torch.cat([0.25 * f0[:, 2:], (1 - 0.25) * f0[:, :2]], 1)
    assert flow_out is not None and flow_out.shape == want.shape
    _cmp(flow_out, want, atol=2e-4, rtol=1e-4, what="testgetflowout")
    hip.check_range()


@pytest.mark.parametrize("case", ["depth_S3_100x150", "depth_S4_128x200", "depth_S6_300x400", "depth_S7_520x530"])
def test_model_pyramid_depths(hip, oracle, weights, golden, dev, case):
    """--test3scales / --test4scales / --test6scales / --test7scales (main.py:243-268): the whole forward with S_tst + 1 pyramid
    levels (padding unit 2^S_tst * 8) against the REFERENCE's own output at that depth and against the oracle."""
    import fldr_harness as Hn
    g = golden(case)
    S = int(g["S_tst"])
    m, _, a = Hn.prepare_model(dev, args=Hn.args_config(test_scales=S))
    frames = Hn.frames_from_uint8(torch.from_numpy(g["frames_u8"]))
    H, W = frames.shape[-2:]
    t = torch.tensor([[float(g["t"])]])
    out = Hn.interpolate(m, a, frames.to(dev), t.to(dev))
    assert out.shape[-2:] == (H, W) and out.dtype == torch.float64
    y0, x0, h, w = (int(v) for v in g["window"])
    err = _cmp(out[..., y0:y0 + h, x0:x0 + w], torch.from_numpy(g["out"]), atol=1e-4, what="S_tst=%d vs reference" % S)
    # the WHOLE frame against the reference through its per-channel checksums (the deep cases store only a window of the frame):
    # mean error per value <= 1e-6 like the oracle bound below; and the padded size the reference worked on
    assert list(Hn.pad_frames(frames, a).shape[-2:]) == list(g["padded"])
    npx = float(H * W)
    assert (np.abs(out.sum((0, 2, 3)).cpu().numpy() - g["out_sum"]) <= 1e-6 * npx).all()
    assert (np.abs(out.abs().sum((0, 2, 3)).cpu().numpy() - g["out_abssum"]) <= 1e-6 * npx).all()
    with torch.no_grad():
        ref = oracle.forward(weights, oracle.pad_and_pyramid(frames, n_levels=S + 1), t)[..., :H, :W]
    _cmp(out, ref, atol=1e-4, what="S_tst=%d vs oracle" % S)
    assert (out.cpu() - ref).abs().mean().item() <= 1e-6
    p8 = Hn.psnr(Hn.to_uint8_image(ref[0]), Hn.to_uint8_image(out[0]))
    print("S_tst=%d: max|err| vs reference %.2e, 8-bit PSNR vs oracle %.1f dB" % (S, err, p8))
    assert p8 >= 90.0


@pytest.mark.parametrize("case", [(256, 384, 0.5, 11), (200, 456, 0.25, 12)])
def test_model_matches_oracle_varying_motion(hip, oracle, weights, dev, model, case):
    """Pairs under a smoothly varying motion field (zoom + rotation + shift: the flow changes from pixel to pixel, sources of
    one row land on several target rows) instead of the global / per-quadrant shifts of the other whole-model cases."""
    import fldr_harness as Hn
    H, W, tv, seed = case
    m, a = model
    frames = Hn.frames_from_uint8(Hn.synthetic_pair_varying(H, W, seed=seed))
    t = torch.tensor([[tv]])
    out = Hn.interpolate(m, a, frames.to(dev), t.to(dev))
    with torch.no_grad():
        ref = oracle.forward(weights, oracle.pad_and_pyramid(frames), t)[..., :H, :W]
    err = _cmp(out, ref, atol=1e-4, what="varying motion %dx%d" % (H, W))
    print("%dx%d varying motion: max|err| %.2e" % (H, W, err))
    assert (out.cpu() - ref).abs().mean().item() <= 1e-6


# ---------------------------------------------------------------------------------------------------
# full-size (BASELINE config 2: 3840x2160) checks
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frames4k(dev):
    import fldr_harness as Hn
    return Hn.frames_from_uint8(Hn.synthetic_pair(2160, 3840, seed=1, quadrant=True)).to(dev)


def test_4k_forward_properties(hip, dev, model, frames4k):
    import fldr_harness as Hn
    m, a = model
    t = torch.tensor([[0.5]], device=dev)
    out = Hn.interpolate(m, a, frames4k, t)
    assert out.shape == (1, 3, 2160, 3840) and out.dtype == torch.float64 and torch.isfinite(out).all()
    out2 = Hn.interpolate(m, a, frames4k, t)
    # Deterministic by construction since round 3: every splat accumulates fp32 products in fp64 LDS tiles (sums of a few fp32
    # values are exact in fp64, so their order does not matter) and nothing else in the forward is order-dependent — unlike the
    # reference, whose fp32 atomicAdd order varies from run to run.  Two forwards: the same bits.
    assert torch.equal(out, out2)
    # static scene: both inputs equal -> the interpolated frame is that frame
    same = frames4k.clone()
    same[:, :, 1] = same[:, :, 0]
    o3 = Hn.interpolate(m, a, same, t)
    p = Hn.psnr(Hn.to_uint8_image(same[0, :, 0]), Hn.to_uint8_image(o3[0]))
    print("static-scene PSNR at 4K: %.1f dB" % p)
    assert p > 40.0


def test_4k_splat_mass_and_linearity(hip, dev):
    H, W = 2304, 3840
    g = torch.Generator(device="cpu").manual_seed(11)
    flow = ((torch.rand(1, 2, H // 8, W // 8, generator=g) - 0.5) * 6).to(dev)
    flow = hip.resize_bilinear(flow, H, W, mul=8.0)
    x = torch.rand(1, 2, H, W, device=dev)
    y = torch.rand(1, 2, H, W, device=dev)
    sx, sy = hip.softsplat_fwd(x, flow), hip.softsplat_fwd(y, flow)
    sxy = hip.softsplat_fwd(2.0 * x - 0.5 * y, flow)
    assert (sxy - (2.0 * sx - 0.5 * sy)).abs().max().item() < 1e-4          # linearity
    ones = torch.ones(1, 1, H, W, device=dev)
    acc = hip.softsplat_fwd(ones, flow)
    # mass conservation: every source deposits the sum of its in-bounds corner weights
    xs = torch.arange(W, device=dev, dtype=torch.float32).view(1, W) + flow[0, 0]
    ys = torch.arange(H, device=dev, dtype=torch.float32).view(H, 1) + flow[0, 1]
    tot = 0
    for tx, wx in ((xs.floor(), xs.floor() + 1 - xs), (xs.floor() + 1, xs - xs.floor())):
        for ty, wy in ((ys.floor(), ys.floor() + 1 - ys), (ys.floor() + 1, ys - ys.floor())):
            tot = tot + (wx * wy * ((tx >= 0) & (tx < W) & (ty >= 0) & (ty < H))).double().sum()
    assert abs(acc.double().sum().item() - tot.item()) / tot.item() < 1e-6


@pytest.mark.timeout(900)
def test_4k_forward_matches_oracle(hip, oracle, weights, dev, model, frames4k):
    """BASELINE config 2 against the CPU oracle on the same seeded synthetic pair (tens of seconds of CPU)."""
    import fldr_harness as Hn
    m, a = model
    t = torch.tensor([[0.5]])
    out = Hn.interpolate(m, a, frames4k, t.to(dev)).cpu()
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    with torch.no_grad():
        ref = oracle.forward(weights, oracle.pad_and_pyramid(frames4k.cpu()), t)[:, :, :2160, :3840]
    err = (out - ref).abs()
    p = Hn.psnr(Hn.to_uint8_image(ref[0]), Hn.to_uint8_image(out[0]))
    print("4K: max|err| %.2e mean %.2e; PSNR(8-bit) gpu vs oracle %.1f dB" % (err.max().item(), err.mean().item(), p))
    assert err.max().item() <= 1e-4 and err.mean().item() <= 1e-6 and p >= 90.0


def test_pwcnet_forward_runs_on_the_correlation_kernel(hip, oracle, dev):
    """a17: signature + wiring only (weights are not shipped: numerics unpinned)."""
    from OpticalFlow.PWCNet import PWCNet
    from OpticalFlow import correlation
    torch.manual_seed(0)
    net = PWCNet().to(dev).eval()
    a = torch.rand(2, 3, 100, 180, device=dev)
    b = torch.rand(2, 3, 100, 180, device=dev)
    calls = []
    orig = correlation.FunctionCorrelation
    correlation.FunctionCorrelation = lambda f, s: (calls.append((f.shape, f.detach().cpu(), s.detach().cpu())), orig(f, s))[1]
    try:
        with torch.no_grad():
            flow = net(a, b)
    finally:
        correlation.FunctionCorrelation = orig
    assert flow.shape == (2, 2, 100, 180) and torch.isfinite(flow).all()
    assert [c[0][1] for c in calls] == [196, 128, 96, 64, 32]          # one cost volume per decoder level
    _, f, s = calls[0]
    _cmp(orig(f.to(dev), s.to(dev)), oracle.correlation(f, s), atol=1e-5, rtol=1e-5, what="in-network cost volume")


def test_fused_dec3_synth_matches_unfused(hip, dev, hooks):
    """dec3-on-nearest-x2 as four 2x2 phase convolutions + fp64 tail == 3x3 conv kernel + fldr_synth_tail."""
    g = _gen(12)
    N, h, w = 2, 20, 38
    d2 = torch.rand(N, 16, h, w, generator=g)                              # post-ReLU activations
    wt = torch.randn(6, 16, 3, 3, generator=g) / 6
    bs = torch.randn(6, generator=g) * 0.3
    cands = [torch.rand(N, 3, 2 * h, 2 * w, generator=g) * 2 - 1 for _ in range(6)]
    t = torch.tensor([[0.25], [0.5]])
    ref_logits = F.conv2d(F.interpolate(d2, scale_factor=2, mode="nearest"), wt, bs, padding=1)
    out, logits = hip.dec3_synth(d2.to(dev), wt.to(dev), bs.to(dev), [c.to(dev) for c in cands], t.to(dev), 1.5616, want_refine=True)
    _cmp(logits, ref_logits, atol=3e-6, rtol=1e-6, what="phase-decomposed dec3 logits")
    unf = hip.synth_tail(hip.conv2d([d2.to(dev)], wt.to(dev), bs.to(dev), up2=[True]), [c.to(dev) for c in cands], t.to(dev), 1.5616)
    _cmp(out, unf, atol=2e-6, what="fused vs unfused tail")
    occ = F.softmax(ref_logits.double() / 1.5616, dim=1)
    t4 = t.view(N, 1, 1, 1)
    wk = [(1 - t4), t4] * 3
    num = sum(wk[k] * occ[:, k:k + 1] * cands[k] for k in range(6))
    den = sum(wk[k] * occ[:, k:k + 1] for k in range(6))
    _cmp(out, num / den, atol=2e-6, what="fused tail vs torch")
    # the tile-grid shift (wide frames) only moves tile boundaries: same bits
    try:
        for xs in (16, 5, 31):
            hip.lib().fldr_debug_dec3_xshift(xs)
            o2 = hip.dec3_synth(d2.to(dev), wt.to(dev), bs.to(dev), [c.to(dev) for c in cands], t.to(dev), 1.5616)
            assert torch.equal(o2, out), xs
    finally:
        hip.lib().fldr_debug_dec3_xshift(-1)


@pytest.mark.parametrize("shape", [(2, 20, 38), (1, 8, 32), (1, 37, 70), (1, 64, 96)])
def test_fused_dec3_synth_on_the_matrix_cores(hip, dev, shape):
    """fldr_dec3_synth_spk: the phase convolutions of the fused dec3 + blend kernel on the fp16 matrix cores (3 x fp16 split) from
    dec2's split-packed output, against torch (logits and blended frame) and against the fp32-FMA kernel: partial tiles, tiles
    at every border, two samples."""
    g = _gen(44)
    N, h, w = shape
    d2 = torch.rand(N, 16, h, w, generator=g) * 1.7                         # post-ReLU activations
    wt = torch.randn(6, 16, 3, 3, generator=g) / 6
    bs = torch.randn(6, generator=g) * 0.3
    cands = [(torch.rand(N, 3, 2 * h, 2 * w, generator=g) * 2 - 1).to(dev) for _ in range(6)]
    t = torch.tensor([[0.25], [0.5]])[:N]
    ref_logits = F.conv2d(F.interpolate(d2.double(), scale_factor=2, mode="nearest"), wt.double(), bs.double(), padding=1)
    d2p = hip.spk_pack(d2.to(dev))
    out, logits = hip.dec3_synth(d2p, wt.to(dev), bs.to(dev), cands, t.to(dev), 1.5616, want_refine=True)
    _cmp(logits, ref_logits.float(), atol=4e-6, rtol=2e-6, what="matrix-core dec3 logits")
    occ = F.softmax(ref_logits / 1.5616, dim=1)
    t4 = t.view(N, 1, 1, 1).double()
    wk = [(1 - t4), t4] * 3
    num = sum(wk[k] * occ[:, k:k + 1] * cands[k].cpu().double() for k in range(6))
    den = sum(wk[k] * occ[:, k:k + 1] for k in range(6))
    _cmp(out, num / den, atol=3e-6, what="matrix-core dec3 + blend vs torch")
    vec = hip.dec3_synth(d2.to(dev), wt.to(dev), bs.to(dev), cands, t.to(dev), 1.5616)
    _cmp(out, vec, atol=3e-6, what="matrix-core vs fp32-FMA kernel")
    o32 = hip.dec3_synth(d2p, wt.to(dev), bs.to(dev), cands, t.to(dev), 1.5616, out_dtype=torch.float32)
    assert o32.dtype == torch.float32 and torch.equal(o32, out.float())


@pytest.mark.parametrize("shape", [(1, 16, 64), (2, 24, 40), (1, 20, 72), (1, 8, 36), (1, 72, 136)])
def test_dec2_dec3_fused_producer_consumer_kernel(hip, dev, shape):
    """fldr_dec23_synth (round 5): dec2 = ReLU(conv3x3(cat(nearest-x2(dec1), enc1))) produced tile by tile in LDS by four waves while eight
    others run dec3's phase convolutions + fp64 softmax / blend on the previous tile — against fp64 torch (the bound of the matrix-core
    dec3 test, 3e-6) and against the two-kernel path (conv2d_spk + dec3_synth on the packed tensor): full and partial tiles, tiles at
    every border, two samples, candidates that are strided views (as I0 / I1 are planes of the frame pair tensor), the fp32 output.
    At these shapes every workgroup does one tile; the walks of many tiles per workgroup (the producer-to-consumer handoff from one
    tile to the next) are tested in tests/test_gpu_schedule.py::test_dec23_bits_independent_of_workgroups."""
    g = _gen(45)
    N, h, w = shape                                                          # half resolution (dec2 / enc1); dec1 at h/2 x w/2
    dec1 = torch.rand(N, 32, h // 2, w // 2, generator=g) * 1.5             # post-ReLU activations
    enc1 = torch.rand(N, 16, h, w, generator=g) * 1.5
    w2 = torch.randn(16, 48, 3, 3, generator=g) / 12
    b2 = torch.randn(16, generator=g) * 0.2
    w3 = torch.randn(6, 16, 3, 3, generator=g) / 6
    b3 = torch.randn(6, generator=g) * 0.3
    cands = [(torch.rand(N, 3, 2 * h, 2 * w, generator=g) * 2 - 1).to(dev) for _ in range(4)]
    pair = (torch.rand(N, 3, 2, 2 * h, 2 * w, generator=g) * 2 - 1).to(dev)
    cands += [pair[:, :, 0], pair[:, :, 1]]                                  # channel stride 2 H W, batch stride 6 H W
    t = torch.tensor([[0.25], [0.5]])[:N]
    cat = torch.cat([F.interpolate(dec1.double(), scale_factor=2, mode="nearest"), enc1.double()], 1)
    d2 = F.relu(F.conv2d(cat, w2.double(), b2.double(), padding=1))
    logits = F.conv2d(F.interpolate(d2, scale_factor=2, mode="nearest"), w3.double(), b3.double(), padding=1)
    occ = F.softmax(logits / 1.5616, dim=1)
    t4 = t.view(N, 1, 1, 1).double()
    wk = [(1 - t4), t4] * 3
    ref = sum(wk[k] * occ[:, k:k + 1] * cands[k].cpu().double() for k in range(6)) / sum(wk[k] * occ[:, k:k + 1] for k in range(6))
    dec1p, enc1p = hip.spk_pack(dec1.to(dev)), hip.spk_pack(enc1.to(dev))
    out = hip.dec23_synth(dec1p, enc1p, w2.to(dev), b2.to(dev), w3.to(dev), b3.to(dev), cands, t.to(dev), 1.5616)
    assert out.dtype == torch.float64 and out.shape == (N, 3, 2 * h, 2 * w)
    _cmp(out, ref, atol=3e-6, what="fused dec2 + dec3 + blend vs fp64 torch")
    d2p = hip.conv2d_spk([dec1p, enc1p], w2.to(dev), b2.to(dev), relu=True, up2=[True, False], want_f32=False, want_spk=True)
    two = hip.dec3_synth(d2p, w3.to(dev), b3.to(dev), cands, t.to(dev), 1.5616)
    _cmp(out, two, atol=3e-6, what="fused vs conv2d_spk + dec3_synth")
    assert torch.equal(out, hip.dec23_synth(dec1p, enc1p, w2.to(dev), b2.to(dev), w3.to(dev), b3.to(dev), cands, t.to(dev), 1.5616))
    o32 = hip.dec23_synth(dec1p, enc1p, w2.to(dev), b2.to(dev), w3.to(dev), b3.to(dev), cands, t.to(dev), 1.5616, out_dtype=torch.float32)
    assert o32.dtype == torch.float32 and torch.equal(o32, out.float())
    hip.check_range()


def test_ring_fault_poisons_outputs_and_raises_in_the_next_forward(hip, dev, model):
    """The fault path of the convolution ring, forced through the test build (fldr_debug_ring_spin_limit(0): every wait that is not
    satisfied at once expires — a consumer then runs on with operands that have not landed):
      (i)   the convolution writes NaN instead of its result (fp32 and packed outputs), the event is counted (fldr_ring_status) and
            stored into the host-visible status words without any synchronisation by the caller;
      (ii)  every frame-writing kernel (fldr_synth_tail, fldr_dec23_synth, fldr_dec3_synth_spk) launched while the flag is still unseen
            writes a NaN frame — each adds the device's poison to its blend weight —, never a plausible wrong one;
      (iii) the NEXT model(...) call raises FldrError on entry (DCTXVFInet.forward polls the status words) — the drop-in path of
            INTEGRATION.md section 1, where nobody calls check_range();
      (iv)  after the reset that the exception performs, the same convolution and forward give their clean results again, bit for bit."""
    import fldr_harness as Hn
    m, a = model
    g = _gen(77)
    x = torch.rand(1, 96, 40, 64, generator=g).to(dev) * 2 - 1
    c = m.rec_ctx_ds[0]
    frames = Hn.frames_from_uint8(Hn.synthetic_pair(256, 256, seed=5)).to(dev)
    t = torch.tensor([[0.5]], device=dev)
    with hip.test_hooks() as L:
        hip.check_range()
        clean = hip.conv2d_spk([hip.spk_pack(x)], c.weight, c.bias, relu=True, want_f32=True, want_spk=True)
        clean_frame = Hn.interpolate(m, a, frames, t)
        words = hip.status_words()
        assert words[0] == 0 and words[1] == 0
        try:
            assert L.fldr_debug_ring_spin_limit(0) == 0
            bad = hip.conv2d_spk([hip.spk_pack(x)], c.weight, c.bias, relu=True, want_f32=True, want_spk=True)
            torch.cuda.synchronize()
            assert torch.isnan(bad[0]).all(), "a convolution whose ring waits expired must write NaN, not values"
            assert torch.isnan(bad[1].float()).all()
            assert words[1] == 1 and words[0] == 0                       # visible to the host with no library call at all
            assert L.fldr_debug_ring_timeouts() > 0
            assert L.fldr_debug_ring_spin_limit(-1) == 1 << 21           # waits are patient again; the flag is still set and unseen
        finally:
            L.fldr_debug_ring_spin_limit(-1)
        # (ii) callers that do not look at the flags: every frame-writing kernel is poisoned
        pyr = Hn.build_pyramid(Hn.pad_frames(frames, a), a)
        T, _, _ = m.vfinet._host_scalars()
        cands = [torch.rand(1, 3, 64, 96, device=dev) for _ in range(6)]
        tail = hip.synth_tail(torch.randn(1, 6, 64, 96, device=dev), cands, t, T)
        assert torch.isnan(tail).all()
        dec1 = hip.spk_pack(torch.rand(1, 32, 16, 24, device=dev))
        enc1 = hip.spk_pack(torch.rand(1, 16, 32, 48, device=dev))
        un = m.vfinet.refine_unet
        fr = hip.dec23_synth(dec1, enc1, un.dec2.weight, un.dec2.bias, un.dec3.weight, un.dec3.bias, cands, t, T)
        assert torch.isnan(fr).all(), "fldr_dec23_synth after a ring fault must write NaN frames"
        d2p = hip.conv2d_spk([dec1, enc1], un.dec2.weight, un.dec2.bias, relu=True, up2=[True, False], want_f32=False, want_spk=True)
        assert torch.isnan(hip.dec3_synth(d2p, un.dec3.weight, un.dec3.bias, cands, t, T)).all()
        # (iii) the next forward raises on entry, and the exception resets the flags
        with pytest.raises(hip.FldrError, match="ring"):
            m([None] * 6, t, normInput=pyr, is_training=False, validation=False)
        assert words[1] == 0 and words[0] == 0 and L.fldr_debug_ring_timeouts() == 0
        # (iv) clean again
        again = hip.conv2d_spk([hip.spk_pack(x)], c.weight, c.bias, relu=True, want_f32=True, want_spk=True)
        assert torch.equal(again[0], clean[0]) and torch.equal(again[1].float(), clean[1].float())
        assert torch.equal(Hn.interpolate(m, a, frames, t), clean_frame)
        hip.check_range()
    # the range flag takes the same road: saturated activations are visible in word [0] without a synchronising call
    big = torch.full((1, 16, 16, 32), 1.0e5, device=dev)
    w = torch.ones(16, 16, 3, 3, device=dev)
    hip.check_range()
    words = hip.status_words()
    out = hip.conv2d_spk([hip.spk_pack(big)], w, None, want_f32=True, want_spk=True)
    torch.cuda.synchronize()
    assert torch.isfinite(out[0]).all()
    assert words[0] == 1 and words[1] == 0
    with pytest.raises(hip.FldrError, match="fp16 split range"):
        m([None] * 6, t, normInput=Hn.build_pyramid(Hn.pad_frames(frames, a), a), is_training=False, validation=False)
    assert words[0] == 0


def test_pair_invariant_cache_multi_t(hip, oracle, weights, dev, model):
    """8x protocol: 7 outputs per pair with PCA/flows/z computed once == 7 independent forwards == oracle."""
    import fldr_harness as Hn
    m, a = model
    frames = Hn.frames_from_uint8(Hn.synthetic_pair(256, 384, seed=3, quadrant=True)).to(dev)
    ts = [k / 8 for k in range(1, 8)]
    cached = Hn.interpolate_multi(m, a, frames, ts)
    assert m.pair_cache is False and m._pair_state is None
    pyr = oracle.pad_and_pyramid(frames.cpu())
    for tv, c in zip(ts, cached):
        t = torch.tensor([[tv]])
        plain = Hn.interpolate(m, a, frames, t.to(dev))
        # The cache only skips recomputation and the default path is deterministic (fp64-accumulated splats): the same bits.
        # (Rounds 1-2 summed the feature splats with fp32 atomics: two runs then differed in the last bits of the flows, and the
        # backward warp's hard mask threshold — mask < 0.999 -> 0, fLDRnet.py:573-574 — could flip a pixel: bounded outliers.)
        assert torch.equal(c, plain), "cached vs uncached t=%g: %.3e" % (tv, (c - plain).abs().max().item())
        if tv in (0.125, 0.5):
            with torch.no_grad():
                ref = oracle.forward(weights, pyr, t)[:, :, :256, :384]
            _cmp(c, ref, atol=1e-4, what="cached vs oracle t=%g" % tv)
    # the later outputs of a pair are independent once the cache is filled: dealt to side streams, the same frames (same cache: same bits)
    side = [torch.cuda.Stream(device=dev) for _ in range(3)]
    par = Hn.interpolate_multi(m, a, frames, ts, streams=side)
    torch.cuda.synchronize()
    for tv, c, q in zip(ts, cached, par):
        assert torch.equal(q, c), "side streams vs one stream t=%g" % tv
    # deterministic mode (gather splat for the feature maps): cached and uncached outputs are the same bits
    prev = hip.SPLAT_FEATURES
    try:
        hip.SPLAT_FEATURES = "gather"
        det = Hn.interpolate_multi(m, a, frames, [0.5, 0.875])
        for tv, c in zip([0.5, 0.875], det):
            assert torch.equal(c, Hn.interpolate(m, a, frames, torch.tensor([[tv]], device=dev))), tv
        det_s = Hn.interpolate_multi(m, a, frames, [0.5, 0.875, 0.25], streams=side)
        torch.cuda.synchronize()
        assert torch.equal(det_s[0], det[0]) and torch.equal(det_s[1], det[1])
    finally:
        hip.SPLAT_FEATURES = prev
    # a different pair must not hit the cache
    m.pair_cache = True
    try:
        t = torch.tensor([[0.5]], device=dev)
        o1 = Hn.interpolate(m, a, frames, t)
        other = Hn.frames_from_uint8(Hn.synthetic_pair(256, 384, seed=4)).to(dev)
        o2 = Hn.interpolate(m, a, other, t)
        m.pair_cache = False
        m._pair_state = None
        _cmp(o2, Hn.interpolate(m, a, other, t), atol=2e-5, what="cache miss on a new pair")
        assert (o1 - o2).abs().max().item() > 1e-2
    finally:
        m.pair_cache = False
        m._pair_state = None


@pytest.mark.parametrize("shape", [([96], 96), ([48, 48, 4], 96), ([48, 48], 48), ([64], 64), ([64, 32], 32), ([48], 4)])
def test_split_fp16_conv_is_fp32_equivalent(hip, dev, shape):
    """The 3 x fp16-split MFMA convolution against an fp64 reference: its error must be at the level of the exact
    fp32 MFMA kernel's (both differ from fp64 only by fp32 accumulation rounding)."""
    parts, cout = shape
    g = _gen(13)
    N, H, W = 1, 41, 77
    srcs = [F.relu(torch.randn(N, c, H, W, generator=g)) * (0.02 if i % 2 else 1.0) for i, c in enumerate(parts)]
    cin = sum(parts)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * 0.03
    bs = torch.randn(cout, generator=g) * 0.1
    ref = F.conv2d(torch.cat(srcs, 1).double(), wt.double(), bs.double(), padding=1)
    dsrc = [s.to(dev) for s in srcs]
    e = {}
    for prec in ("fp32", "split"):
        got = hip.conv2d(dsrc, wt.to(dev), bs.to(dev), precision=prec).double().cpu()
        e[prec] = ((got - ref).abs().mean().item(), (got - ref).abs().max().item())
    print("cin %3d cout %2d: mean|err| fp32-MFMA %.2e  split %.2e ; max %.2e / %.2e (|ref| mean %.2e)"
          % (cin, cout, e["fp32"][0], e["split"][0], e["fp32"][1], e["split"][1], ref.abs().mean().item()))
    assert e["split"][0] <= 1.5 * e["fp32"][0] + 1e-8 and e["split"][1] <= 2.0 * e["fp32"][1] + 1e-7


def test_split_conv_range_guard(hip, dev):
    """fp16 ends at 65504: the hi/lo split behind the split-precision convolutions must never turn a finite activation
    into inf / NaN.  Up to 131008 the value is still represented (hi saturates, lo carries the excess to fp16
    precision: absolute error <= 16); beyond it the value saturates to a finite number; both cases and NaN inputs raise
    the sticky status flag (fldr_range_status), in-range data does not."""
    g = _gen(41)
    N, C, H, W = 1, 48, 24, 40
    wt = (torch.randn(32, C, 3, 3, generator=g) * 0.02).to(dev)
    x = (torch.randn(N, C, H, W, generator=g) * 50).to(dev)
    hip.range_status(reset=True)
    ref = hip.conv2d([x], wt, None, precision="fp32")
    got = hip.conv2d_spk([x], wt, None)
    assert not hip.range_status() and (got - ref).abs().max().item() <= 1e-3
    big = x.clone()
    big[0, 3, 5, 7] = 1.0e5                                 # beyond fp16, inside the extended exact range
    big[0, 9, 11, 13] = -9.0e4
    ref = hip.conv2d([big], wt, None, precision="fp32")
    for srcs in ([big], [hip.spk_pack(big)]):               # packed on the fly / packed by the caller
        hip.range_status(reset=True)
        got = hip.conv2d_spk(srcs if not isinstance(srcs[0], hip.Spk) else srcs, wt, None)
        assert torch.isfinite(got).all()
        assert (got - ref).abs().max().item() <= 16.0 * wt.abs().max().item() * 1.01     # <= 16 absolute on the one big input of a window
    hip.spk_pack(big)
    assert hip.range_status()                               # ... and it was flagged
    assert not hip.range_status()                           # sticky until read with reset
    huge = x.clone()
    huge[0, 0, 0, 0] = 3.0e7
    huge[0, 1, 2, 3] = float("nan")
    got = hip.conv2d_spk([huge], wt, None, want_f32=True, want_spk=True)
    assert torch.isfinite(got[0]).all() and torch.isfinite(got[1].float()).all()      # saturated, never inf / NaN
    with pytest.raises(hip.FldrError):
        hip.check_range()
    # the stride-2 encoders and the register-staged split conv stage fp32 sources through the same guarded split
    w4 = (torch.randn(16, C, 4, 4, generator=g) * 0.02).to(dev)
    o = hip.conv2d([huge.nan_to_num(0.0)], w4, None, stride=2)
    o2 = hip.conv2d([huge.nan_to_num(0.0)], wt, None, precision="split")
    assert torch.isfinite(o).all() and torch.isfinite(o2).all() and hip.range_status()


def test_fp16_conv_path_config5(hip, oracle, weights, dev, model):
    """BASELINE config 5: 3x3 convs with plain fp16 inputs (fp32 accumulate).  Not fp32-equivalent: report the error
    and the PSNR between its rounded 8-bit frame and the oracle's (the fp32-class paths are at ~100 dB)."""
    import fldr_harness as Hn
    m, a = model
    frames = Hn.frames_from_uint8(Hn.synthetic_pair(512, 768, seed=5, quadrant=True)).to(dev)
    t = torch.tensor([[0.5]])
    with torch.no_grad():
        ref = oracle.forward(weights, oracle.pad_and_pyramid(frames.cpu()), t)
    res = {}
    prev = hip.CONV_PRECISION
    try:
        for prec in ("fp32", "split", "fp16"):
            hip.CONV_PRECISION = prec
            out = Hn.interpolate(m, a, frames, t.to(dev)).cpu()
            err = (out - ref).abs()
            res[prec] = (err.max().item(), err.mean().item(), Hn.psnr(Hn.to_uint8_image(ref[0]), Hn.to_uint8_image(out[0])))
    finally:
        hip.CONV_PRECISION = prev
    for k, v in res.items():
        print("conv precision %-5s: max|err| %.2e mean %.2e  PSNR(8-bit vs oracle) %.1f dB" % ((k,) + v))
    assert res["split"][1] <= 2.0 * res["fp32"][1] + 1e-8            # the split path is fp32-class
    assert res["fp16"][2] > 45.0                                      # fp16 inputs: visually lossless, but not fp32-class


@pytest.mark.parametrize("size", [(200, 500), (256, 256), (130, 300)])
def test_gpu_ingest_matches_cpu_caller(hip, oracle, dev, size):
    """uint8 -> normalise -> reflect pad -> bicubic pyramid on the device == the reference's CPU pre-processing."""
    import fldr_harness as Hn
    H, W = size
    u8 = Hn.synthetic_pair(H, W, seed=6, quadrant=True)                 # [2,3,H,W]
    ref = oracle.pad_and_pyramid(oracle.frames_from_uint8(u8))
    got = hip.ingest_pyramid(u8.unsqueeze(0).to(dev))
    assert len(got) == 6
    assert torch.equal(got[0].cpu(), ref[0])                            # normalisation + reflect padding: bit exact
    for i in range(1, 6):
        _cmp(got[i], ref[i], atol=2e-6, what="bicubic level %d" % i)


@pytest.mark.parametrize("case", [(200, 328, 6, 1), (260, 515, 6, 2), (130, 258, 4, 1), (300, 522, 7, 1), (64, 70, 3, 1), (2160, 3840, 6, 1)])
def test_fused_ingest_pyramid_bit_identical(hip, dev, case):
    """Round 4: fldr_ingest_pyramid_u8 (the uint8 frames read once, every pyramid level written from a staged 64 x 64 tile, one launch)
    against fldr_ingest_u8 + one fldr_pyramid_bicubic per level: every level bit for bit — widths that are not multiples of 4 (byte
    path), reflect padding across tile borders, batch of 2, 3 ... 7 levels, the 4K geometry."""
    import fldr_harness as Hn
    H, W, nl, B = case
    u8 = torch.stack([Hn.synthetic_pair(H, W, seed=20 + k, quadrant=True) for k in range(B)], 0).to(dev)
    prev = hip.INGEST_FUSED
    try:
        hip.INGEST_FUSED = False
        ref = hip.ingest_pyramid(u8, nl)
        hip.INGEST_FUSED = True
        got = hip.ingest_pyramid(u8, nl)
    finally:
        hip.INGEST_FUSED = prev
    assert len(got) == len(ref) == nl
    for i in range(nl):
        assert got[i].shape == ref[i].shape and torch.equal(got[i], ref[i]), (i, (got[i] - ref[i]).abs().max().item())


def test_interpolate_u8_reports_psnr_and_ssim(hip, oracle, dev, model):
    """uint8 in -> uint8 out with PSNR and SSIM-Y against a ground truth, all on the device (main.py:885-911)."""
    import fldr_harness as Hn
    m, a = model
    u = Hn.synthetic_pair(200, 328, seed=6)
    gt = u[0:1].to(dev)                                              # any uint8 frame serves as "ground truth" here
    img, (ps, ss) = Hn.interpolate_u8(m, a, u.unsqueeze(0).to(dev), torch.tensor([[0.5]], device=dev), target_u8=gt, want_ssim=True)
    hwc = lambda t: np.transpose(t.cpu().numpy(), (1, 2, 0)).astype(np.float64)
    assert ss[0] == pytest.approx(oracle.ssim_y(hwc(gt[0]), hwc(img[0])), abs=1e-10)
    assert ps[0] == pytest.approx(oracle.psnr(hwc(gt[0]), hwc(img[0])), abs=1e-9)


def test_gpu_metrics_and_u8_roundtrip(hip, oracle, weights, dev, model):
    import fldr_harness as Hn
    m, a = model
    H, W = 200, 330
    u8 = Hn.synthetic_pair(H, W, seed=8)
    t = torch.tensor([[0.5]])
    gt = Hn.synthetic_pair(H, W, seed=9)[0:1]                           # any uint8 "ground truth" [1,3,H,W]
    img, ps = Hn.interpolate_u8(m, a, u8.unsqueeze(0).to(dev), t.to(dev), target_u8=gt.to(dev))
    assert img.dtype == torch.uint8 and img.shape == (1, 3, H, W) and len(ps) == 1
    with torch.no_grad():
        ref = oracle.forward(weights, oracle.pad_and_pyramid(oracle.frames_from_uint8(u8)), t)[:, :, :H, :W]
    ref_img = oracle.to_uint8_image(ref, H, W)                          # [H,W,3] float
    diff = (img[0].permute(1, 2, 0).cpu().double().numpy() - ref_img)
    assert (np.abs(diff) > 0).mean() < 1e-3 and np.abs(diff).max() <= 1  # rounding ties aside, identical 8-bit frames
    want = oracle.psnr(gt[0].permute(1, 2, 0).double().numpy(), img[0].permute(1, 2, 0).cpu().double().numpy())
    assert abs(ps[0] - want) < 1e-9


@pytest.mark.parametrize("size", [(256, 384), (200, 330), (270, 482), (200, 331)])
def test_interpolate_u8_direct_frame_equals_rounded_fp64_frame(hip, dev, model, size):
    """Without a ground truth interpolate_u8 takes the rounded 8-bit frame straight out of the fused synthesis kernel (fldr_dec23_synth's
    out_u8: the fp64 frame is never written): the same bytes as rounding the fp64 frame with fldr_frame_metrics — sizes that need
    padding and a crop, an odd width (falls back to the fp64 frame + frame_metrics)."""
    import fldr_harness as Hn
    m, a = model
    H, W = size
    u8 = Hn.synthetic_pair(H, W, seed=21).unsqueeze(0).to(dev)
    t = torch.tensor([[0.5]], device=dev)
    img, none = Hn.interpolate_u8(m, a, u8, t)
    assert none is None and img.dtype == torch.uint8 and img.shape == (1, 3, H, W)
    assert not hasattr(m.vfinet, "emit_u8")                              # the request is an argument of the call, not model state
    with torch.no_grad():
        pyr = hip.ingest_pyramid(u8, a.S_tst + 1)
        pred, _ = m([None] * (a.S_tst + 1), t, normInput=pyr, is_training=False, validation=False)
    assert pred.dtype == torch.float64
    _, ref = hip.frame_metrics(pred, H, W, None, want_u8=True)
    assert torch.equal(img, ref)
    hip.check_range()


def test_dec23_synth_u8_output_with_crop(hip, dev):
    """fldr_dec23_synth's third output form against its fp64 frame rounded by fldr_frame_metrics: crops that cut tiles, two samples."""
    g = _gen(46)
    N, h, w = 2, 40, 72
    dec1p = hip.spk_pack((torch.rand(N, 32, h // 2, w // 2, generator=g) * 1.5).to(dev))
    enc1p = hip.spk_pack((torch.rand(N, 16, h, w, generator=g) * 1.5).to(dev))
    w2, b2 = (torch.randn(16, 48, 3, 3, generator=g) / 12).to(dev), (torch.randn(16, generator=g) * 0.2).to(dev)
    w3, b3 = (torch.randn(6, 16, 3, 3, generator=g) / 6).to(dev), (torch.randn(6, generator=g) * 0.3).to(dev)
    cands = [(torch.rand(N, 3, 2 * h, 2 * w, generator=g) * 2.4 - 1.2).to(dev) for _ in range(6)]      # beyond [-1, 1]: the clamp acts
    t = torch.tensor([[0.25], [0.5]], device=dev)
    frame = hip.dec23_synth(dec1p, enc1p, w2, b2, w3, b3, cands, t, 1.5616)
    for (Hc, Wc) in ((2 * h, 2 * w), (2 * h - 5, 2 * w - 6), (17, 34)):
        got = hip.dec23_synth(dec1p, enc1p, w2, b2, w3, b3, cands, t, 1.5616, u8_crop=(Hc, Wc))
        _, ref = hip.frame_metrics(frame, Hc, Wc, None, want_u8=True)
        assert got.dtype == torch.uint8 and got.shape == (N, 3, Hc, Wc) and torch.equal(got, ref)
    with pytest.raises(Exception):
        hip.dec23_synth(dec1p, enc1p, w2, b2, w3, b3, cands, t, 1.5616, u8_crop=(10, 11))      # odd width


@pytest.mark.parametrize("size", [(96, 128), (61, 203), (7, 9), (540, 960)])
def test_gpu_ssim_y_matches_oracle(hip, oracle, dev, size):
    """fldr_ssim_y_u8 (utils.ssim_bgr on the device, 8f-3) against the oracle's restatement on seeded frames, a batch of
    two with different distortions; fp64 throughout -> 1e-10."""
    H, W = size
    u = oracle.synthetic_pair(H + 0, W + 0, seed=9, quadrant=True)              # [2,3,H,W] uint8, channel 0 = B
    tgt = u[0]
    g = _gen(3)
    noisy = (tgt.float() + torch.randn(tgt.shape, generator=g) * 9).round().clamp(0, 255).to(torch.uint8)
    preds = torch.stack([u[1], noisy], 0)
    tgts = torch.stack([tgt, tgt], 0)
    got = hip.ssim_y_u8(preds.to(dev), tgts.to(dev)).cpu().tolist()
    hwc = lambda t: np.transpose(t.numpy(), (1, 2, 0)).astype(np.float64)
    for b in range(2):
        ref = oracle.ssim_y(hwc(tgts[b]), hwc(preds[b]))
        assert got[b] == pytest.approx(ref, abs=1e-10), (b, got[b], ref)
    same = hip.ssim_y_u8(tgts.to(dev), tgts.to(dev)).cpu().tolist()
    assert same[0] == pytest.approx(1.0, abs=1e-13)
    import fldr_harness as Hn
    assert Hn.ssim_bgr(hwc(tgts[1]), hwc(preds[1])) == pytest.approx(got[1], abs=1e-13)
    if H == 7:
        with pytest.raises(ValueError):
            hip.ssim_y_u8(preds[:, :, :6].contiguous().to(dev), tgts[:, :, :6].contiguous().to(dev))


def test_odd_shape_stress_of_kernel_variants(hip, dev, capsys, hooks):
    """tools/stress_shapes.py: ~240 random odd shapes (tiny / partial tiles, several samples, multi-source, odd channel
    counts) of every kernel that has a variant hook or an unfused counterpart — persistent vs per-tile stride-2 conv, the LDS-DMA
    packed-source stride-2 kernel vs the register-staged one, the 32x32x16 ring conv vs the 16x16x32 ring,
    split-packed vs register-staged 3x3 conv under both unit policies, band vs strip splat, fused level-0 prep vs the
    kernels it replaces, one-pass vs two-pass PCA, fused dec3 + tail vs conv + tail, dec3 + blend on the matrix cores vs the
    fp32-FMA kernel, the image splat's four-pixel walk vs the one-pixel walk, parked vs recomputed PCA projections."""
    import os
    import runpy
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runpy.run_path(os.path.join(root, "tools", "stress_shapes.py"), run_name="__main__")
    out = capsys.readouterr().out
    assert "MISMATCH" not in out, out
    assert out.count(" 0 mismatches") == 11, out


def test_operators_random_odd_shapes_vs_oracle(hip, oracle, dev):
    """Correlation (forward / backward) and the raw splat (forward / backward) on random odd shapes — single rows / columns,
    sizes that are not multiples of the 8x32 / 64x4 tiles, several samples — against the oracle.  The backward warp, the splat
    metric and the resizes at such shapes: tests/test_gpu_warp_ops.py."""
    import random
    from OpticalFlow import correlation
    rnd = random.Random(7)
    g = _gen(77)
    for _ in range(6):
        N, C, H, W = rnd.choice([1, 2]), rnd.choice([1, 2, 5, 17, 33]), rnd.choice([1, 2, 7, 9, 31, 40]), rnd.choice([1, 3, 15, 33, 65])
        a = torch.randn(N, C, H, W, generator=g); b = torch.randn(N, C, H, W, generator=g)
        _cmp(correlation.FunctionCorrelation(a.to(dev), b.to(dev)), oracle.correlation(a, b), atol=2e-6 * math.sqrt(C) + 1e-6, rtol=1e-5,
             what="correlation %s" % ((N, C, H, W),))
        gc = torch.randn(N, 81, H, W, generator=g)
        ga, gb = hip.correlation_bwd(a.to(dev), b.to(dev), gc.to(dev))
        ra, rb = oracle.correlation_backward(a, b, gc)
        _cmp(ga, ra, atol=5e-6, rtol=1e-5, what="correlation gradFirst %s" % ((N, C, H, W),))
        _cmp(gb, rb, atol=5e-6, rtol=1e-5, what="correlation gradSecond %s" % ((N, C, H, W),))
    for _ in range(6):
        N, C, H, W = rnd.choice([1, 2]), rnd.choice([1, 3, 4, 7, 9]), rnd.choice([1, 2, 5, 33, 40]), rnd.choice([1, 2, 63, 64, 65, 130])
        x = torch.rand(N, C, H, W, generator=g) * 2 - 1
        flow = (torch.rand(N, 2, H, W, generator=g) - 0.5) * rnd.choice([0.0, 2.0, 30.0])
        go = torch.randn(N, C, H, W, generator=g)
        _cmp(hip.softsplat_fwd(x.to(dev), flow.to(dev)), oracle.splat_forward(x, flow), atol=3e-5, rtol=1e-5, what="raw splat %s" % ((N, C, H, W),))
        gi, gf = hip.softsplat_bwd(x.to(dev), flow.to(dev), go.to(dev))
        ri, rf = oracle.splat_backward(x, flow, go)
        _cmp(gi, ri, atol=3e-6, rtol=1e-5, what="splat gradInput %s" % ((N, C, H, W),))
        _cmp(gf, rf, atol=5e-5, rtol=1e-5, what="splat gradFlow %s" % ((N, C, H, W),))


@pytest.mark.timeout(600)
def test_bench_rccl_process_group_world_size_one(dev, clean_launcher):
    """The multi-GPU branch of bench.py on the hardware a 1-GPU lease has: `python -m torch.distributed.run --nproc-per-node 1
    bench.py --gpus 1` with FLDR_BENCH_FORCE_PG=1 makes the rank call dist.init_process_group("nccl", device_id=...) — RCCL on
    ROCm — and run every barrier, the MAX all_reduce and the all_gather of the timed region on DEVICE tensors at world size 1,
    then one JSON line.  The rank is started by the GPU-clean helper process of tests/conftest.py (this pytest process has touched
    the GPU and must not fork + exec other programs).
    What this proves: the library loads, the communicator initialises, the reductions work; NOT a scaling curve."""
    import json
    import os
    import socket
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s_ = socket.socket(); s_.bind(("127.0.0.1", 0)); port = s_.getsockname()[1]; s_.close()
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["FLDR_BENCH_FORCE_PG"] = "1"
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "0", "--sustained-s", "0",
           "--no-cpu-baseline", "--varying-motion-steps", "0", "--incl-ingest-steps", "0", "--multi-t-pairs", "0", "--fp16-mode-steps", "0"]
    r = clean_launcher(cmd, env=env, timeout=540)
    assert r["rc"] == 0, (r["stdout"][-2000:], r["stderr"][-4000:])
    js = [json.loads(l) for l in r["stdout"].splitlines() if l.startswith("{")]
    assert len(js) == 1, r["stdout"][-2000:]
    j = js[0]
    pg = j["config"]["process_group"]
    assert pg["backend"].startswith("nccl") and pg["world_size"] == 1 and pg["forced_at_world_size_1"] is True
    assert j["n_gpus"] == 1 and j["steps"] == 2 and j["value"] > 0 and len(j["config"]["per_rank_pairs_per_s"]) == 1


def test_every_entry_point_rejects_null_arguments(dev, clean_launcher):
    """Error behaviour of the C ABI (include/fldr_hip.h: every compute entry returns a negative FLDR_E_* code for arguments it cannot run
    on, before any launch): tools/abi_null_probe.py calls every exported non-debug entry point with null pointers / zero sizes and, where
    it takes a descriptor, with a zero-initialised one — in a process of its own, so that a missing check is a failed test (the child's
    segmentation fault), not a dead session.  Size queries of a shape answer FLDR_E_ARG for the zero shape as well."""
    import json
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = clean_launcher([sys.executable, os.path.join(root, "tools", "abi_null_probe.py")], env=dict(os.environ), timeout=300)
    assert r["rc"] == 0, (r["rc"], r["stdout"][-1500:], r["stderr"][-3000:])
    codes = json.loads([l for l in r["stdout"].splitlines() if l.startswith("{")][-1])
    assert len(codes) >= 50, len(codes)
    constants = ("fldr_dec23_prepack_size", "fldr_dec3_prepack_spk_size", "fldr_sizeof_desc")      # sizes that do not depend on a pointer or a shape
    bad = {k: v for k, v in codes.items() if not all(c is not None and (c < 0 or k in constants) for c in v)}
    assert not bad, bad
    for k in ("fldr_conv2d_spk", "fldr_dec23_synth", "fldr_level0_prep", "fldr_softsplat_acc64", "fldr_pca_project_pyramid", "fldr_conv2d_s2_spk",
              "fldr_correlation_fwd", "fldr_ingest_pyramid_u8", "fldr_status_word"):
        assert codes[k] == [-1, -1], (k, codes[k])                        # FLDR_E_ARG, with and without a (zeroed) descriptor


def test_bench_two_ranks_share_the_gpu_rehearsal(dev, clean_launcher):
    """The N > 1 path of bench.py with REAL device work in every rank, as far as a 1-GPU lease allows: `bench.py --gpus 2 --share-gpu`
    starts two ranks through its own launcher (python -m torch.distributed.run), both run their forwards on device 0 (RCCL refuses two
    ranks on one device: the process group is gloo), each on its own disjoint pairs (shard_pairs), and rank 0 prints one line with the
    MAX-over-ranks time, two per-rank rates, cpu_baseline absent only because the test asks so.  Small frames: two processes with 4K
    pyramids would only make the test slow.  What this proves: two GPU processes of this package start, load the library, bind their
    status blocks, run and meet at the barriers; NOT a scaling number (the line says `rehearsal`)."""
    import json
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--share-gpu", "--backend", "gloo", "--steps", "4", "--warmup", "1",
           "--height", "540", "--width", "960", "--sustained-s", "0", "--no-cpu-baseline", "--varying-motion-steps", "0", "--incl-ingest-steps", "0",
           "--multi-t-pairs", "0", "--fp16-mode-steps", "0", "--config5-steps", "0"]
    r = clean_launcher(cmd, env=env, timeout=540)
    assert r["rc"] == 0, (r["stdout"][-2000:], r["stderr"][-4000:])
    js = [json.loads(l) for l in r["stdout"].splitlines() if l.startswith("{")]
    assert len(js) == 1, r["stdout"][-2000:]
    j = js[0]
    assert j["n_gpus"] == 2 and j["steps"] == 4 and j["value"] > 0 and "rehearsal" in j
    assert len(j["config"]["per_rank_pairs_per_s"]) == 2 and all(x > 0 for x in j["config"]["per_rank_pairs_per_s"])
    assert j["config"]["process_group"]["backend"] == "gloo" and j["config"]["process_group"]["world_size"] == 2
    assert j["config"]["parallelism"].startswith("dp2")


@pytest.mark.timeout(600)
def test_bench_dump_outputs_are_the_last_timed_frame(dev, model, clean_launcher, tmp_path):
    """`bench.py --dump-outputs DIR` (the output-for-output comparison of two builds): two runs with the same arguments write the same
    float64 frame bit for bit, and that frame is the forward of the pair the LAST timed step interpolated (--steps 3 over 4 pairs:
    pair 2, t = 0.5) — computed here in-process from the same seeded synthetic pair.  540x960: the whole frame fits the dump budget."""
    import json
    import os
    import sys
    import fldr_harness as Hn
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    frames = []
    for run in ("a", "b"):
        d = str(tmp_path / run)
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--height", "540", "--width", "960",
               "--sustained-s", "0", "--no-cpu-baseline", "--varying-motion-steps", "0", "--incl-ingest-steps", "0", "--multi-t-pairs", "0",
               "--fp16-mode-steps", "0", "--config5-steps", "0", "--dump-outputs", d]
        r = clean_launcher(cmd, env=env, timeout=540)
        assert r["rc"] == 0, (r["stdout"][-2000:], r["stderr"][-4000:])
        js = [json.loads(l) for l in r["stdout"].splitlines() if l.startswith("{")]
        assert len(js) == 1 and js[0]["steps"] == 3 and js[0]["ms_per_step"] > 0, r["stdout"][-2000:]
        assert js[0]["dump_outputs"]["arrays"] == {"frame": [1, 3, 540, 960]}, js[0]["dump_outputs"]
        assert sorted(os.listdir(d)) == ["frame.npy"]
        f = np.load(os.path.join(d, "frame.npy"))
        assert f.dtype == np.float64 and f.shape == (1, 3, 540, 960) and np.isfinite(f).all()
        frames.append(f)
    assert np.array_equal(frames[0], frames[1])
    m, a = model
    fr = Hn.frames_from_uint8(Hn.synthetic_pair(540, 960, seed=2)).to(dev)
    with torch.no_grad():
        ref = Hn.interpolate(m, a, fr, torch.tensor([[0.5]], device=dev)).cpu().numpy()
    assert np.abs(frames[0] - ref).max() <= 1e-6, np.abs(frames[0] - ref).max()


@pytest.mark.timeout(900)
def test_bench_full_adds_every_leg_a_plain_run_skips(dev, clean_launcher):
    """A plain `bench.py` line carries the headline and nothing that takes runs of its own; `--full` adds latency, the sustained rate, the
    eager loop, the informational legs, the roofline and the CPU baseline with the parity of the GPU frame against the oracle.  540x960
    with short legs (multi-t and config 5 run at 4K only)."""
    import json
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    base = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--height", "540", "--width", "960"]
    lines = {}
    for name, extra in (("plain", []), ("full", ["--full", "--sustained-s", "0.2", "--varying-motion-steps", "6", "--incl-ingest-steps", "6",
                                                 "--fp16-mode-steps", "6"])):
        r = clean_launcher(base + extra, env=env, timeout=420)
        assert r["rc"] == 0, (name, r["stdout"][-2000:], r["stderr"][-4000:])
        js = [json.loads(l) for l in r["stdout"].splitlines() if l.startswith("{")]
        assert len(js) == 1 and js[0]["steps"] == 3 and js[0]["warmup"] == 1 and js[0]["value"] > 0, r["stdout"][-2000:]
        lines[name] = js[0]
    legs = ("sustained", "varying_motion", "incl_ingest", "fp16_conv_mode", "roofline", "cpu_baseline", "parity")
    p, f = lines["plain"], lines["full"]
    assert not [k for k in legs if k in p] and "single_stream_latency_ms" not in p["config"], p
    assert p["config"]["hip_graphs"]["on"] and "eager_ms_per_step" not in p["config"]["hip_graphs"]
    assert all(k in f for k in legs), sorted(f)
    assert f["config"]["single_stream_latency_ms"] > 0 and f["config"]["hip_graphs"]["eager_ms_per_step"] > 0
    assert f["roofline"]["launch_ms"] > 0 and f["cpu_baseline"]["value"] > 0
    assert f["parity"]["max_abs_err"] < 2e-5 and f["parity"]["psnr_8bit_db"] > 90.0, f["parity"]


def test_evaluate_dir_matches_per_frame_pipeline(hip, dev, model, tmp_path):
    """fldr_harness.evaluate_dir (the dataset-shaped entry: main.py:815-911) on a folder of PNG frames written here — one scene of
    5 frames, multiple = 4: the pair (0, 4) and its three intermediate targets — against the per-frame pipeline the other tests
    pin (interpolate_u8 with the target: PSNR / SSIM-Y on the device)."""
    import os
    from PIL import Image
    import fldr_harness as Hn
    m, a = model
    H, W = 192, 320                                                         # (reflect padding to 256 x 512 needs pad < size)
    base = Hn.synthetic_pair(H + 8, W + 16, seed=11)[0]
    frames = [base[:, k:k + H, int(1.5 * k):int(1.5 * k) + W].contiguous() for k in range(5)]     # a scene panning by (1.5, 1) px per frame
    folder = os.path.join(str(tmp_path), "Type1", "TEST01")
    os.makedirs(folder)
    for k, f in enumerate(frames):
        Image.fromarray(np.ascontiguousarray(f.permute(1, 2, 0).numpy()[:, :, ::-1])).save(os.path.join(folder, "%05d.png" % k))
    res = Hn.evaluate_dir(str(tmp_path), multiple=4, t_step_size=4, model=m, args=a, device=dev)
    assert res["frames"] == 3 and res["pairs"] == 1 and m.pair_cache is False and m._pair_state is None
    u8 = torch.stack([frames[0], frames[4]], 0).unsqueeze(0).to(dev)
    ps, ss = [], []
    for k, tv in ((1, 0.25), (2, 0.5), (3, 0.75)):
        _, (p, s_) = Hn.interpolate_u8(m, a, u8, torch.tensor([[tv]], device=dev), target_u8=frames[k].unsqueeze(0).to(dev), want_ssim=True)
        ps.append(p[0]); ss.append(s_[0])
    assert res["psnr"] == pytest.approx(sum(ps) / 3, rel=1e-9) and res["ssim"] == pytest.approx(sum(ss) / 3, rel=1e-9)
    assert res["per_t"][0.5] == pytest.approx(ps[1], rel=1e-9) and res["psnr"] > 20.0
