"""Schedule invariance of the persistent kernels: a kernel's bits must not depend on how many workgroups walk its tiles, or in
what order.

The launchers size a persistent grid as min(tiles per XCD, cap).  At the shapes of the other unit tests that is about one tile per
workgroup, so the code that moves a workgroup from one tile to the next (buffer parity, ring-slot reuse, the next tile's geometry,
crossing a sample, group or level boundary) hardly runs there.  The test build's knobs force a handful of workgroups, which turns
every small shape into a deep walk.  Each family runs at the default schedule and at every forced one and must give the same bits;
the deepest walk (one workgroup per XCD) is also compared with references that do not walk — fp64 torch, and where one exists a
kernel of the same arithmetic that is not persistent — so that a fault both schedules share still fails.

Every knob a test changes is restored on the way out (`knobs`), and every knob test requires that no bounded ring wait expired."""
import contextlib
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


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


# the argument with which each fldr_debug_<knob> only reports its value (each hook's convention: include/fldr_hip_test_hooks.h)
_QUERY = {"spk_wgs_per_xcd": 0, "spk_small_units": 0, "spk_variant": -1, "ring32": -1, "ring_tile_width": -1, "ring_consumers": 0,
          "ring_resident": -1, "s2_wgs_per_xcd": 0, "s2_dma": -1, "s2_xshift": -2, "s2_persistent": -1, "dec23_wgs_per_xcd": 0,
          "pca_workgroups": 0, "pca_variant": -1, "dec3_xcd": -1, "corr_xcd": -1, "corr_variant": -1, "corr_chunk": 0}


@contextlib.contextmanager
def knobs(L, **values):
    """Set fldr_debug_<name> to each value for the block, restore every knob it changed in `finally` (the test build's knobs are
    global to the process: a knob left changed would silently alter later tests), and on leaving the block require that no bounded
    ring wait expired."""
    prev = {}
    try:
        for name, v in values.items():
            fn = getattr(L, "fldr_debug_" + name)
            prev[name] = fn(_QUERY[name])
            assert fn(v) == v, (name, v)
        yield
    finally:
        for name, v in prev.items():
            getattr(L, "fldr_debug_" + name)(v)
    assert L.fldr_debug_ring_timeouts() == 0, "a bounded ring wait expired"


def _bits(x):
    return x.buf if hasattr(x, "buf") else x


def _same(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(_bits(a), _bits(b)), (what, i)


def test_knobs_query_set_and_restore(hip, hooks):
    """The two walk-depth hooks of this module query with any value <= 0 and report their defaults (the LDS caps), and `knobs` puts
    every value back, also when its block raises."""
    L = hooks
    assert L.fldr_debug_dec23_wgs_per_xcd(0) == 32 and L.fldr_debug_dec23_wgs_per_xcd(-3) == 32
    assert L.fldr_debug_s2_wgs_per_xcd(0) == 64 and L.fldr_debug_s2_wgs_per_xcd(-1) == 64
    with pytest.raises(RuntimeError, match="inside"):
        with knobs(L, dec23_wgs_per_xcd=2, s2_wgs_per_xcd=3, pca_workgroups=17, s2_xshift=0, ring32=0):
            assert (L.fldr_debug_dec23_wgs_per_xcd(0), L.fldr_debug_s2_wgs_per_xcd(0), L.fldr_debug_s2_xshift(-2)) == (2, 3, 0)
            raise RuntimeError("inside")
    assert (L.fldr_debug_dec23_wgs_per_xcd(0), L.fldr_debug_s2_wgs_per_xcd(0), L.fldr_debug_pca_workgroups(0), L.fldr_debug_s2_xshift(-2),
            L.fldr_debug_ring32(-1)) == (32, 64, 512, -1, 1)


def _conv_bound(x64, w64, b64, K, res64=None, **conv):
    """Elementwise bound on |kernel - fp64| of a 3 x fp16-split convolution that accumulates K products in fp32: the split products
    (2^-20 relative at most), recursive fp32 summation ((K + 16) 2^-24 of the sum of the terms' magnitudes) and the output's own
    rounding all stay below it.  A term taken from the wrong tile, sample or channel group is of the order of that sum itself."""
    mag = F.conv2d(x64.abs(), w64.abs(), b64.abs() if b64 is not None else None, **conv)
    if res64 is not None:
        mag = mag + res64.abs()
    return ((K + 16) * 2.0 ** -24 + 2.0 ** -20) * mag + 1e-30


def _check64(got, ref, bound, what):
    got = got.double().cpu()
    assert torch.isfinite(got).all(), what + ": non-finite values"
    err = (got - ref).abs()
    bad = err > bound
    assert not bad.any(), "%s: %d values beyond the bound, largest excess %.3e" % (what, int(bad.sum()), float((err - bound).max()))


# ---------------------------------------------------------------------------------------------------
# ring 3x3 convolutions (conv_ring_kernels.hip), capped by fldr_debug_spk_wgs_per_xcd (default 32)
# ---------------------------------------------------------------------------------------------------
_SPK_VALUES = (1, 2, 3, 5, 7, 32)

# (N, channels per source, nearest-x2 per source, cout, cout_store, H, W, relu, residual)
_RING_CASES = [(3, [16], [0], 16, None, 45, 100, True, True),              # one group, three samples, ragged tiles
               (1, [32, 16], [1, 0], 16, None, 50, 98, True, False),       # nearest-x2 source; the resident-weight ring applies (3 chunks)
               (3, [48], [0], 48, None, 37, 75, False, True),              # one 48-channel group (three 16-channel sub-groups)
               (1, [96], [0], 96, None, 61, 130, True, False),             # two groups (six sub-groups)
               (2, [48, 48, 4], [0, 0, 0], 96, None, 36, 60, True, True),  # three sources, a partial last input group
               (3, [40], [0], 96, None, 19, 45, False, False),             # a partial input chunk
               (3, [48], [0], 6, 4, 9, 15, True, False)]                   # a partial output group, fewer channels stored

# pipelines whose results are the same bits whatever the schedule: (consumer waves, tile width, resident weights).  The tile width is
# forced because the automatic choice reads the workgroup count, and so does ring32_pays: ring32 is off here (its own test below).
_RING_PIPES = ((8, 32, 0), (8, 16, 0), (4, 32, 0), (8, 32, 1))


@pytest.mark.parametrize("case", _RING_CASES)
def test_ring_conv_bits_independent_of_workgroups(hip, dev, case, hooks):
    """fldr_conv2d_spk on the loader / consumer ring (4 and 8 consumer waves, 8x16 and 8x32 tiles, resident weights; with and without
    16-channel sub-groups) at 1, 2, 3, 5, 7 and 32 workgroups per XCD — counts that are no multiple of the group count are rounded up
    by the launcher: fp32 and packed outputs are the bits of the default schedule.  The deepest walk equals the register-staged split
    convolution (no persistent walk) and fp64 within the summation bound."""
    L = hooks
    N, cs, ups, cout, cst, H, W, relu, res = case
    g = _gen(61)
    srcs = [torch.randn(N, c, H // (2 if u else 1), W // (2 if u else 1), generator=g).to(dev) for c, u in zip(cs, ups)]
    wt = (torch.randn(cout, sum(cs), 3, 3, generator=g) / 20).to(dev)
    b = torch.randn(cout, generator=g).to(dev)
    rs = torch.randn(N, cst or cout, H, W, generator=g).to(dev) if res else None
    up2 = [bool(u) for u in ups]
    packed = [hip.spk_pack(x) for x in srcs]
    split = hip.conv2d(srcs, wt, b, relu=relu, residual=rs, cout_store=cst, up2=up2, precision="split")
    x64 = torch.cat([F.interpolate(x.double().cpu(), scale_factor=2, mode="nearest") if u else x.double().cpu() for x, u in zip(srcs, ups)], 1)
    w64, b64 = wt.double().cpu()[:cst or cout], b.double().cpu()[:cst or cout]
    r64 = rs.double().cpu() if res else None
    ref = F.conv2d(x64, w64, b64, padding=1)
    ref = (F.relu(ref) if relu else ref) + (r64 if res else 0)         # the residual is added after the activation
    bound = _conv_bound(x64, w64, b64, sum(cs) * 9, r64, padding=1)

    def run():
        return hip.conv2d_spk(packed, wt, b, relu=relu, residual=rs, cout_store=cst, up2=up2, want_f32=True, want_spk=True)

    for small in ((-1,) if cout <= 16 else (-1, 1 << 20)):                # never / always 16-channel sub-groups
        for cons, tw, resident in _RING_PIPES:
            what = (small, cons, tw, resident)
            with knobs(L, spk_variant=1, ring32=0, spk_small_units=small, ring_consumers=cons, ring_tile_width=tw, ring_resident=resident):
                dflt = run()
                for v in _SPK_VALUES:
                    with knobs(L, spk_wgs_per_xcd=v):
                        got = run()
                    _same(got, dflt, what + (v,))
                    if v == 1:
                        assert torch.equal(got[0], split), what
                        assert torch.equal(hip.spk_pack(split).buf, got[1].buf), what
                        _check64(got[0], ref, bound, "ring conv, one workgroup per XCD %s" % (what,))


@pytest.mark.parametrize("case", [(96, 96, True, True), (48, 16, False, False), (64, 40, True, True)])
def test_multi_level_conv_bits_independent_of_workgroups(hip, dev, case, hooks):
    """fldr_conv2d_spk_levels: the units of all levels, numbered level after level, dealt to 1 .. 32 workgroups per XCD, so that a
    workgroup walks from level to level down to a 1x1 level: the bits of the default schedule.  The deepest walk equals the per-level
    split convolution and fp64 within the summation bound."""
    L = hooks
    cin, cout, relu, res = case
    g = _gen(62)
    sizes = [(72, 120), (36, 60), (18, 30), (9, 15), (5, 33), (3, 2), (1, 1)]
    xs = [torch.randn(1, cin, h, w, generator=g).to(dev) for h, w in sizes]
    wt = (torch.randn(cout, cin, 3, 3, generator=g) / 20).to(dev)
    b = torch.randn(cout, generator=g).to(dev)
    rs = [torch.randn(1, cout, h, w, generator=g).to(dev) for h, w in sizes] if res else [None] * len(sizes)
    packed = [hip.spk_pack(x) for x in xs]

    def run():
        return [o for pair in hip.conv2d_spk_levels(packed, wt, b, relu=relu, residuals=rs if res else None, want_f32=True, want_spk=True)
                for o in pair]

    with knobs(L, spk_variant=1):
        dflt = run()
        for v in _SPK_VALUES:
            with knobs(L, spk_wgs_per_xcd=v):
                got = run()
            _same(got, dflt, v)
        with knobs(L, spk_wgs_per_xcd=1):
            deep = run()
    w64, b64 = wt.double().cpu(), b.double().cpu()
    for l, (x, r) in enumerate(zip(xs, rs)):
        assert torch.equal(deep[2 * l], hip.conv2d([x], wt, b, relu=relu, residual=r, precision="split")), sizes[l]
        x64, r64 = x.double().cpu(), (r.double().cpu() if res else None)
        ref = F.conv2d(x64, w64, b64, padding=1)
        ref = (F.relu(ref) if relu else ref) + (r64 if res else 0)
        _check64(deep[2 * l], ref, _conv_bound(x64, w64, b64, cin * 9, r64, padding=1), "levels, level %s" % (sizes[l],))


@pytest.mark.parametrize("case", [(3, [64], 64, 29, 70, True), (3, [40], 96, 17, 33, True), (3, [32, 32], 96, 45, 100, False)])
def test_ring32_bits_independent_of_workgroups(hip, dev, case, hooks):
    """conv3x3_ring32_kernel (forced wherever it applies): packed outputs of 64 and 96 channels, three samples, at every forced
    workgroup count per XCD are the bits of the default schedule.  The deepest walk is within the 16x16x32 ring's rounding (the bound
    of test_ring32_conv_matches_the_16x16x32_kernels) and within the summation bound of fp64."""
    L = hooks
    N, cs, cout, H, W, relu = case
    g = _gen(63)
    srcs = [torch.randn(N, c, H, W, generator=g).to(dev) for c in cs]
    wt = (torch.randn(cout, sum(cs), 3, 3, generator=g) / (sum(cs) * 9) ** 0.5).to(dev)
    b = torch.randn(cout, generator=g).to(dev)
    packed = [hip.spk_pack(x) for x in srcs]

    def run():
        return hip.conv2d_spk(packed, wt, b, relu=relu, want_f32=False, want_spk=True)

    with knobs(L, spk_variant=1, ring32=0, spk_small_units=-1, ring_tile_width=32):
        other = run().float()                                             # the 16x16x32 ring
    with knobs(L, spk_variant=1, ring32=2, spk_small_units=-1, ring_tile_width=0, ring_consumers=8):
        dflt = run()
        for v in _SPK_VALUES:
            with knobs(L, spk_wgs_per_xcd=v):
                got = run()
            assert torch.equal(got.buf, dflt.buf), v
        with knobs(L, spk_wgs_per_xcd=1):
            deep = run().float()
    assert (deep - other).abs().max().item() <= 3e-6 * float(other.abs().max()) + 1e-7
    x64 = torch.cat([p.float().double().cpu() for p in packed], 1)
    w64, b64 = wt.double().cpu(), b.double().cpu()
    ref = F.conv2d(x64, w64, b64, padding=1)
    ref = F.relu(ref) if relu else ref
    _check64(deep, ref, _conv_bound(x64, w64, b64, sum(cs) * 9, padding=1), "ring32, one workgroup per XCD")


# ---------------------------------------------------------------------------------------------------
# stride-2 encoders (conv_s2_split_kernels.hip), capped by fldr_debug_s2_wgs_per_xcd (default 64: the LDS caps rule)
# ---------------------------------------------------------------------------------------------------
_S2_VALUES = (1, 2, 3, 7)


@pytest.mark.parametrize("shape", [(8, 16, 34, 130), (24, 32, 40, 72), (40, 24, 30, 44), (16, 32, 18, 520), (32, 16, 66, 98)])
def test_stride2_bits_independent_of_workgroups(hip, dev, shape, hooks):
    """The persistent stride-2 encoders, two samples, at 1, 2, 3 and 7 workgroups per XCD: the fp32-source kernel (conv2d stride 2;
    tile-grid shift automatic — 15 on the wide case — and 0) and the packed-source kernels (conv2d_s2_spk, the pair launch) on the
    register-staged and the LDS-DMA staging — fp32 and packed outputs are the bits of the default schedule.  The deepest walk: the
    fp32-source kernel equals the per-tile kernel (no walk), every output is within 3e-6 of fp64 (the bound of
    test_stride2_lds_dma_kernel), the packed twin is the pack of the fp32 output."""
    L = hooks
    cin, cout, H, W = shape
    N = 2
    g = _gen(64)
    x = (F.relu(torch.randn(N, cin, H, W, generator=g)) * 3).to(dev)
    wt = (torch.randn(cout, cin, 4, 4, generator=g) / (cin * 16) ** 0.5).to(dev)
    wt2 = (torch.randn(cout, cin, 4, 4, generator=g) / (cin * 16) ** 0.5).to(dev)
    b, b2 = torch.randn(cout, generator=g).to(dev), torch.randn(cout, generator=g).to(dev)
    xp = hip.spk_pack(x)
    assert hip.s2_spk_ok(wt)

    def run():
        outs = list(hip.conv2d([x], wt, b, stride=2, relu=True, precision="split", want_spk=True))
        outs += list(hip.conv2d_s2_spk(xp, wt, b, relu=True, want_f32=True, want_spk=True))
        return outs + hip.conv2d_s2_spk_pair(xp, [(wt, b), (wt2, b2)], relu=False)

    def near64(got, src, w, bias, relu, what):
        ref = F.conv2d(src.double().cpu(), w.double().cpu(), bias.double().cpu(), stride=2, padding=1)
        ref = F.relu(ref) if relu else ref
        err = (got.double().cpu() - ref).abs().max().item()
        assert torch.isfinite(got).all() and err <= 3e-6 * float(ref.abs().max()) + 1e-7, (what, err)

    with knobs(L, s2_persistent=0):
        per_tile = hip.conv2d([x], wt, b, stride=2, relu=True, precision="split", want_spk=True)
    xv = xp.float()
    for xshift in (-1, 0):
        for dma in (0, 1):
            what = (xshift, dma)
            with knobs(L, s2_persistent=1, s2_xshift=xshift, s2_dma=dma):
                dflt = run()
                for v in _S2_VALUES:
                    with knobs(L, s2_wgs_per_xcd=v):
                        got = run()
                    _same(got, dflt, what + (v,))
                with knobs(L, s2_wgs_per_xcd=1):
                    deep = run()
            _same(deep[:2], per_tile, what)
            near64(deep[0], x, wt, b, True, "fp32-source kernel")
            assert torch.equal(hip.spk_pack(deep[2]).buf, deep[3].buf), what
            near64(deep[2], xv, wt, b, True, "packed-source kernel")
            near64(deep[4].float(), xv, wt, b, False, "pair launch, first problem")
            near64(deep[5].float(), xv, wt2, b2, False, "pair launch, second problem")


# ---------------------------------------------------------------------------------------------------
# fused dec2 + dec3 + blend (dec23_kernels.hip), capped by fldr_debug_dec23_wgs_per_xcd (default 32)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 16, 64), (2, 40, 100), (1, 72, 136), (2, 80, 264)])
def test_dec23_bits_independent_of_workgroups(hip, dev, shape, hooks):
    """fldr_dec23_synth with 1, 2 and 3 workgroups per XCD: four producer waves hand tile after tile to eight consumer waves through
    the LDS buffers of one workgroup (23 tiles per workgroup at one per XCD on the largest case).  The fp64 frame, the fp32 frame and
    the 8-bit frame cropped to an odd height are the bits of the default schedule; the deepest walk is within 3e-6 of fp64 torch (the
    bound of test_dec2_dec3_fused_producer_consumer_kernel) and its 8-bit frame is frame_metrics' rounding of its fp64 frame.
    Candidates include strided views (I0 / I1 as planes of the frame pair tensor)."""
    L = hooks
    N, h, w = shape                                                        # half resolution (dec2 / enc1); dec1 at h/2 x w/2
    g = _gen(65)
    dec1 = torch.rand(N, 32, h // 2, w // 2, generator=g) * 1.5
    enc1 = torch.rand(N, 16, h, w, generator=g) * 1.5
    w2 = torch.randn(16, 48, 3, 3, generator=g) / 12
    b2 = torch.randn(16, generator=g) * 0.2
    w3 = torch.randn(6, 16, 3, 3, generator=g) / 6
    b3 = torch.randn(6, generator=g) * 0.3
    cands = [(torch.rand(N, 3, 2 * h, 2 * w, generator=g) * 2 - 1).to(dev) for _ in range(4)]
    pair = (torch.rand(N, 3, 2, 2 * h, 2 * w, generator=g) * 2 - 1).to(dev)
    cands += [pair[:, :, 0], pair[:, :, 1]]
    t = torch.tensor([[0.25], [0.6]])[:N]
    cat = torch.cat([F.interpolate(dec1.double(), scale_factor=2, mode="nearest"), enc1.double()], 1)
    d2 = F.relu(F.conv2d(cat, w2.double(), b2.double(), padding=1))
    logits = F.conv2d(F.interpolate(d2, scale_factor=2, mode="nearest"), w3.double(), b3.double(), padding=1)
    occ = F.softmax(logits / 1.5616, dim=1)
    t4 = t.view(N, 1, 1, 1).double()
    wk = [(1 - t4), t4] * 3
    ref = sum(wk[k] * occ[:, k:k + 1] * cands[k].cpu().double() for k in range(6)) / sum(wk[k] * occ[:, k:k + 1] for k in range(6))
    args = (hip.spk_pack(dec1.to(dev)), hip.spk_pack(enc1.to(dev)), w2.to(dev), b2.to(dev), w3.to(dev), b3.to(dev), cands, t.to(dev), 1.5616)
    crop = (2 * h - 3, 2 * w - 2)

    def run():
        return [hip.dec23_synth(*args), hip.dec23_synth(*args, out_dtype=torch.float32), hip.dec23_synth(*args, u8_crop=crop)]

    with knobs(L, dec23_wgs_per_xcd=32):
        dflt = run()
    for v in (1, 2, 3):
        with knobs(L, dec23_wgs_per_xcd=v):
            got = run()
        _same(got, dflt, v)
    with knobs(L, dec23_wgs_per_xcd=1):
        deep = run()
    tiles = N * math.ceil(h / 8) * math.ceil(w / 32)
    print("dec23 %s: %d tiles, up to %d per workgroup at one workgroup per XCD" % (shape, tiles, math.ceil(tiles / 8)))
    assert deep[0].dtype == torch.float64 and deep[0].shape == (N, 3, 2 * h, 2 * w)
    err = (deep[0].cpu() - ref).abs().max().item()
    assert torch.isfinite(deep[0]).all() and err <= 3e-6, err
    assert torch.equal(deep[1], deep[0].float())
    _, r8 = hip.frame_metrics(deep[0], crop[0], crop[1], None, want_u8=True)
    assert deep[2].shape == (N, 3) + crop and torch.equal(deep[2], r8)
    hip.check_range()


# ---------------------------------------------------------------------------------------------------
# two-pass PCA pyramid (pca_pyramid_kernels.hip), fldr_debug_pca_workgroups (default 512)
# ---------------------------------------------------------------------------------------------------
_PCA_LEVELS = [(512, 1024), (64, 96), (32, 48), (16, 24), (8, 8), (40, 520)]


@pytest.mark.parametrize("variant,K", [(0, 16), (0, 8), (0, 4), (1, 16)])
def test_pca_pyramid_bits_independent_of_workgroups(hip, oracle, dev, model, variant, K, hooks):
    """fldr_pca_project_pyramid on 1, 2, 3, 17 and 512 persistent workgroups: the vector kernel (K = 16, 8, 4) and the fp64
    matrix-core kernel; the projections parked between the passes for every level, the levels above a size, or none.  A level of
    512 x 1024 makes hundreds of items, so one workgroup walks every item of every level and the min / max reduction runs over all
    of them.  fp32 output, packed twin and min / max are the bits of the default schedule.  The deepest walk: the vector kernel
    equals the per-level one-pass kernels bit for bit (as test_pca_pyramid_bit_identical_to_per_level asserts at the default
    schedule), every variant is within 2e-7 of the fp64 oracle (the bound of test_pca_pyramid_matrix_core_kernel)."""
    L = hooks
    m, _ = model
    g = _gen(66)
    ev, mean, mv = m.EV8.detach()[:K].contiguous(), m.Mean8.detach(), m.meanVec8.detach()[:K].contiguous()
    P = 5 if K == 4 else 6                                                # an odd number of planes
    planes = [(torch.rand(P, h, w, generator=g) * 2 - 1).to(dev) for (h, w) in _PCA_LEVELS]
    raw_mins = (0, P * (32 // 8) * (48 // 8) * K * 8 + 1, 1 << 40)

    def run():
        outs = []
        for raw_min in raw_mins:
            o32, osp, mm = hip.pca_project_pyramid(planes, ev, mean, mv, want_f32=True, want_spk=True, raw_min_bytes=raw_min)
            outs += o32 + osp + [mm.clone()]
        return outs

    with knobs(L, pca_variant=variant):
        dflt = run()
        for v in (1, 2, 3, 17, 512):
            with knobs(L, pca_workgroups=v):
                got = run()
            _same(got, dflt, v)
        with knobs(L, pca_workgroups=1):
            o32, osp, mm = hip.pca_project_pyramid(planes, ev, mean, mv, want_f32=True, want_spk=True)
    for i, pl in enumerate(planes):
        s32, _, smm, _ = hip.pca_project_stream(pl, ev, mean, mv, want_spk=False)
        if variant == 0:
            assert torch.equal(s32, o32[i]) and torch.equal(smm, mm[i]), i
        else:
            assert torch.allclose(smm, mm[i], rtol=1e-13, atol=0.0), (i, smm, mm[i])
        Pl, Hl, Wl = pl.shape
        assert torch.equal(hip.spk_pack(o32[i].reshape(1, Pl * K, Hl // 8, Wl // 8)).buf, osp[i].buf), i
        ref = oracle.to_pca_diff(pl.double().cpu(), mean.cpu(), ev.cpu(), mv.cpu())
        err = (o32[i].reshape(ref.shape).double().cpu() - ref).abs().max().item()
        assert torch.isfinite(o32[i]).all() and err <= 2e-7, (i, err)


# ---------------------------------------------------------------------------------------------------
# tile order: XCD-contiguous ranges (grid padded to a multiple of 8) against row-major
# ---------------------------------------------------------------------------------------------------
# (N, h, w) at dec2's resolution, 8 x 32 tiles: 1, 3, 7, 9 (three samples) and 17 tiles in all
_DEC3_SHAPES = [(1, 5, 20), (1, 20, 30), (1, 8, 200), (3, 8, 70), (1, 136, 30)]


@pytest.mark.parametrize("shape", _DEC3_SHAPES)
def test_dec3_tile_order_identical(hip, dev, shape, hooks):
    """fldr_dec3_synth (fp32-FMA kernel) and fldr_dec3_synth_spk (matrix cores) with the tiles dealt in XCD-contiguous ranges —
    where padding blocks of the grid have no tile — and row-major: the same fp64 and fp32 frames and logits; within 3e-6 of fp64
    torch."""
    L = hooks
    N, h, w = shape
    g = _gen(67)
    d2 = torch.rand(N, 16, h, w, generator=g) * 1.7
    wt = torch.randn(6, 16, 3, 3, generator=g) / 6
    bs = torch.randn(6, generator=g) * 0.3
    cands = [(torch.rand(N, 3, 2 * h, 2 * w, generator=g) * 2 - 1).to(dev) for _ in range(6)]
    t = torch.tensor([[0.25], [0.5], [0.8]])[:N]
    logits = F.conv2d(F.interpolate(d2.double(), scale_factor=2, mode="nearest"), wt.double(), bs.double(), padding=1)
    occ = F.softmax(logits / 1.5616, dim=1)
    t4 = t.view(N, 1, 1, 1).double()
    wk = [(1 - t4), t4] * 3
    ref = sum(wk[k] * occ[:, k:k + 1] * cands[k].cpu().double() for k in range(6)) / sum(wk[k] * occ[:, k:k + 1] for k in range(6))
    srcs = (d2.to(dev), hip.spk_pack(d2.to(dev)))

    def run():
        outs = []
        for src in srcs:
            outs += list(hip.dec3_synth(src, wt.to(dev), bs.to(dev), cands, t.to(dev), 1.5616, want_refine=True))
            outs.append(hip.dec3_synth(src, wt.to(dev), bs.to(dev), cands, t.to(dev), 1.5616, out_dtype=torch.float32))
        return outs

    with knobs(L, dec3_xcd=1):
        contiguous = run()
    with knobs(L, dec3_xcd=0):
        row_major = run()
    _same(row_major, contiguous, "dec3 tile order")
    for i in (0, 3):
        err = (contiguous[i].cpu() - ref).abs().max().item()
        assert torch.isfinite(contiguous[i]).all() and err <= 3e-6, (i, err)


# (N, C, H, W), W % 4 == 0 (the LDS-DMA kernel), 8 x 32 tiles: 1, 3, 7, 9 (three samples) and 17 tiles in all
_CORR_SHAPES = [(1, 16, 5, 20), (1, 24, 20, 28), (1, 37, 8, 200), (3, 16, 8, 68), (1, 81, 136, 28)]


@pytest.mark.parametrize("shape", _CORR_SHAPES)
def test_correlation_tile_order_identical(hip, oracle, dev, shape, hooks):
    """The LDS-DMA cost-volume kernel (8- and 16-channel chunks) with XCD-contiguous tile ranges (padding blocks without a tile at
    these counts) and row-major: the bits of the synchronous kernel, which has no tile order of its own; within the bound of
    test_correlation_matches_oracle."""
    L = hooks
    g = _gen(68)
    a = torch.randn(*shape, generator=g)
    b = torch.randn(*shape, generator=g)
    ad, bd = a.to(dev), b.to(dev)
    with knobs(L, corr_variant=0):
        sync = hip.correlation_fwd(ad, bd)
    for cc in (8, 16):
        for xcd in (1, 0):
            with knobs(L, corr_variant=1, corr_chunk=cc, corr_xcd=xcd):
                got = hip.correlation_fwd(ad, bd)
            assert torch.equal(got, sync), (cc, xcd)
    ref = oracle.correlation(a, b).double()
    err = (sync.double().cpu() - ref).abs()
    assert torch.isfinite(sync).all() and (err <= 2e-6 * math.sqrt(shape[1]) + 1e-6 + 1e-5 * ref.abs()).all(), err.max().item()


# ---------------------------------------------------------------------------------------------------
# the whole forward under the deepest schedule of every family at once
# ---------------------------------------------------------------------------------------------------
_DEEPEST = dict(spk_wgs_per_xcd=1, s2_wgs_per_xcd=1, dec23_wgs_per_xcd=1, pca_workgroups=1, dec3_xcd=0, corr_xcd=0)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("B,H,W,ts", [(1, 264, 520, (0.5,)), (2, 256, 256, (0.3, 0.7))])
def test_forward_bits_under_deepest_schedule(hip, dev, model, B, H, W, ts, hooks):
    """One eager forward of the test build with every persistent family at its deepest walk at the same time (one workgroup per XCD
    for the ring convolutions, the stride-2 encoders, dec23 and the PCA pyramid; row-major dec3 and cost-volume tiles): the fp64 frame
    and interpolate_u8's bytes are the bits of the default schedule.  ring32 is off in both runs: whether it pays depends on the
    workgroup count, and it sums in another order."""
    import fldr_harness as Hn
    L = hooks
    m, a = model
    u8 = torch.stack([Hn.synthetic_pair(H, W, seed=11 + k) for k in range(B)])            # [B,2,3,H,W]
    frames = torch.cat([Hn.frames_from_uint8(p) for p in u8]).to(dev)
    t = torch.tensor([[v] for v in ts], device=dev)
    u8d = u8.to(dev)

    def run():
        f64 = Hn.interpolate(m, a, frames, t)
        img, _ = Hn.interpolate_u8(m, a, u8d, t)
        torch.cuda.synchronize()
        return [f64.clone(), img.clone()]

    with knobs(L, ring32=0):
        dflt = run()
        with knobs(L, **_DEEPEST):
            deep = run()
    assert dflt[0].shape == (B, 3, H, W) and torch.isfinite(dflt[0]).all() and dflt[1].shape == (B, 3, H, W)
    for i, what in enumerate(("fp64 frame", "interpolate_u8")):
        assert torch.equal(deep[i], dflt[i]), "%s: %d values differ" % (what, int((deep[i] != dflt[i]).sum()))
    hip.check_range()
