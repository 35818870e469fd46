"""Row limits of the fused synthesis path (fldr_synth_row_plan and the row-limited entry points): a limited launch writes the rows it is
asked for with the bits of the unlimited launch and leaves every row at or beyond its rounded-up limit untouched; a whole forward whose
caller only looks at the top Hc rows gives exactly those rows.  256 x 256 padded pairs: the smallest shape at which every stage has more
than one tile row (enc3 / dec0: 32 rows = 4 tile rows); 256 x 512 once for enc1's x-shifted tile grid."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture
def nan_empty(monkeypatch):
    """Every tensor the library wrappers allocate with torch.empty starts as NaN (integers: all bits set): an untouched output row is
    recognisable, and so is a kernel that reads one (NaN spreads, and the fp16 split of a NaN sets the range flag)."""
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


@pytest.fixture(scope="module")
def net(dev):
    import fldr_harness as Hn
    m, _, a = Hn.prepare_model(dev)
    return m, a


def _rand(dev, *shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return ((torch.rand(*shape, generator=g) * 2 - 1) * scale).to(dev)


def _up(rows, tile, full):
    return min(full, -(-rows // tile) * tile)


def _limits(tile, full):
    """One tile, a tile boundary +- 1 row, everything."""
    b = (full // 2) // tile * tile
    return (tile, b - 1, b, b + 1, full)


def _rows_match(got, ref, written, what):
    """Rows < written: the bits of the unlimited launch; rows >= written: untouched (NaN, or all bits set)."""
    assert got.shape == ref.shape
    assert torch.equal(got[..., :written, :], ref[..., :written, :]), what
    rest = got[..., written:, :]
    if rest.numel():
        if rest.is_floating_point():
            assert bool(torch.isnan(rest).all()), what
        else:
            assert bool((rest.contiguous().view(torch.uint8) == 255).all()), what


@pytest.fixture(scope="module")
def level0(dev, net):
    """Inputs of the level-0 stages at 256 x 256 and the unlimited results they are compared with (computed once)."""
    import fldr_hip as hip
    m, a = net
    H = W = 256
    flow_lo = _rand(dev, 1, 4, H // 8, W // 8, seed=1, scale=0.7)
    x = _rand(dev, 1, 3, 2, H, W, seed=2)
    I0, I1 = x[:, :, 0], x[:, :, 1]
    t4 = torch.full((1, 1, 1, 1), 0.4, device=dev)
    T, za0, za1 = m.vfinet._host_scalars()
    ref = hip.level0_prep(flow_lo, I0, I1, t4, H, W, za0, za1)
    bw = hip.splat_bounds_upsampled_pair(flow_lo, t4, "images", 8, H, W)
    warped = hip.softsplat_acc64([I0, I1], [ref["flow_t0"], ref["flow_t1"]], [ref["z0"], ref["z1"]], "softmax", bounds_ws=bw)
    torch.cuda.synchronize()
    return dict(H=H, W=W, flow_lo=flow_lo, I0=I0, I1=I1, t4=t4, za=(za0, za1), ref=ref, bw=bw, warped=warped, T=T)


def test_prep_rows(dev, level0, nan_empty):
    """level0_prep_kernel: phase 2 (flowback, im_tot) stops at the limit, row by row; phase 1 keeps every row."""
    import fldr_hip as hip
    L = level0
    for rows in _limits(4, L["H"]):
        r = hip.level0_prep(L["flow_lo"], L["I0"], L["I1"], L["t4"], L["H"], L["W"], *L["za"], rows2=rows)
        for k in ("z0", "z1", "flow_t0", "flow_t1"):
            assert torch.equal(r[k], L["ref"][k]), (rows, k)
        for k in ("flowback_0", "flowback_1", "im0_tot", "im1_tot"):
            _rows_match(r[k], L["ref"][k], rows, (rows, k))
    hip.check_range()


def test_image_splat_rows(dev, level0, nan_empty):
    """splat_acc64_kernel, image configuration (64 x 24 tiles in columns of three): whole columns and the trailing tiles of the last one."""
    import fldr_hip as hip
    L = level0
    r = L["ref"]
    for rows in _limits(24, L["H"]) + (72, 73):
        w = hip.softsplat_acc64([L["I0"], L["I1"]], [r["flow_t0"], r["flow_t1"]], [r["z0"], r["z1"]], "softmax", bounds_ws=L["bw"], rows=rows)
        for k in range(2):
            _rows_match(w[k], L["warped"][k], _up(rows, 24, L["H"]), (rows, k))
    hip.check_range()


@pytest.mark.parametrize("W", [256, 512])
def test_enc1_rows(dev, net, nan_empty, W):
    """conv4x4s2_pers_kernel on enc1's ten fp32 sources (W = 512: the x-shifted, line-aligned tile grid): out_rows, and src_rows — a source
    row at or beyond it is zero padding, so the result is the unlimited convolution of the sources with those rows zeroed, whatever they hold."""
    import fldr_hip as hip
    m, a = net
    u = m.vfinet.refine_unet
    H = 256
    chans = (3, 3, 3, 3, 2, 2, 2, 2, 3, 3)
    pair = _rand(dev, 1, 3, 2, H, W, seed=3)
    srcs = [pair[:, :, 0], pair[:, :, 1]] + [_rand(dev, 1, c, H, W, seed=10 + i) for i, c in enumerate(chans[2:])]
    kw = dict(stride=2, relu=True, want_f32=False, want_spk=True)
    ref = hip.conv2d(srcs, u.enc1.weight, u.enc1.bias, **kw).float()
    for rows in _limits(8, H // 2):
        got = hip.conv2d(srcs, u.enc1.weight, u.enc1.bias, rows=rows, **kw).float()
        _rows_match(got, ref, _up(rows, 8, H // 2), rows)
    for src_rows in (130, 131):
        zeroed = [s.clone() for s in srcs]
        dirty = [s.clone() for s in srcs]
        for z, d in zip(zeroed, dirty):
            z[:, :, src_rows:] = 0.0
            d[:, :, src_rows:] = NAN
        want = hip.conv2d(zeroed, u.enc1.weight, u.enc1.bias, **kw).float()
        got = hip.conv2d(dirty, u.enc1.weight, u.enc1.bias, rows=72, src_rows=src_rows, **kw).float()
        _rows_match(got, want, 72, src_rows)
        assert torch.equal(got[:, :, :(src_rows - 2) // 2], ref[:, :, :(src_rows - 2) // 2])          # windows above the limit: the unlimited bits
    hip.check_range()


def test_enc2_enc3_rows(dev, net, nan_empty):
    """conv4x4s2_dma_spk_kernel: enc2 (16 -> 32 at 128 x 128) and the enc3 pair launch (32 -> 2 x 32 at 64 x 64)."""
    import fldr_hip as hip
    m, a = net
    u = m.vfinet.refine_unet
    x1 = hip.spk_pack(_rand(dev, 1, 16, 128, 128, seed=20))
    kw = dict(relu=True, want_f32=False, want_spk=True)
    ref2 = hip.conv2d_s2_spk(x1, u.enc2.weight, u.enc2.bias, **kw).float()
    for rows in _limits(8, 64):
        got = hip.conv2d_s2_spk(x1, u.enc2.weight, u.enc2.bias, rows=rows, **kw).float()
        _rows_match(got, ref2, _up(rows, 8, 64), rows)
    x2f = _rand(dev, 1, 32, 64, 64, seed=21)
    x2 = hip.spk_pack(x2f)
    halves = u._enc3_halves()
    assert halves is not None
    ref3 = [o.float() for o in hip.conv2d_s2_spk_pair(x2, halves, relu=True)]
    for rows in _limits(8, 32):
        got = hip.conv2d_s2_spk_pair(x2, halves, relu=True, rows=rows)
        for k in range(2):
            _rows_match(got[k].float(), ref3[k], _up(rows, 8, 32), (rows, k))
    # src_rows: rows at or beyond it are never read (NaN there) and count as zero padding
    for src_rows in (34, 35):
        zeroed, dirty = x2f.clone(), x2f.clone()
        zeroed[:, :, src_rows:] = 0.0
        dirty[:, :, src_rows:] = NAN
        want = [o.float() for o in hip.conv2d_s2_spk_pair(hip.spk_pack(zeroed), halves, relu=True)]
        dp = hip.spk_pack(zeroed)
        dp.buf.view(1, 4, 2, 64, 64 * 8)[:, :, :, src_rows:] = NAN       # [N][groups][hi, lo][rows][W x 8 halves]
        got = hip.conv2d_s2_spk_pair(dp, halves, relu=True, rows=24, src_rows=src_rows)
        for k in range(2):
            _rows_match(got[k].float(), want[k], 24, (src_rows, k))
        one = hip.conv2d_s2_spk(dp, halves[0][0], halves[0][1], rows=24, src_rows=src_rows, **kw).float()
        _rows_match(one, want[0], 24, src_rows)
    hip.check_range()


def test_dec0_dec1_rows(dev, net, nan_empty):
    """conv3x3_ring_kernel as dec0 (two 32-channel sources, 64 -> 64 at 32 x 32) and dec1 (nearest-x2 of dec0 + enc2, 96 -> 32 at 64 x 64)."""
    import fldr_hip as hip
    m, a = net
    u = m.vfinet.refine_unet
    e3 = [hip.spk_pack(_rand(dev, 1, 32, 32, 32, seed=30 + k)) for k in range(2)]
    kw = dict(relu=True, want_f32=False, want_spk=True)
    ref0 = hip.conv2d_spk(e3, u.dec0.weight, u.dec0.bias, **kw)
    for rows in _limits(8, 32):
        got = hip.conv2d_spk(e3, u.dec0.weight, u.dec0.bias, rows=rows, **kw)
        _rows_match(got.float(), ref0.float(), _up(rows, 8, 32), rows)
    e2 = hip.spk_pack(_rand(dev, 1, 32, 64, 64, seed=32))
    ref1 = hip.conv2d_spk([ref0, e2], u.dec1.weight, u.dec1.bias, up2=[True, False], **kw).float()
    for rows in _limits(8, 64):
        got = hip.conv2d_spk([ref0, e2], u.dec1.weight, u.dec1.bias, up2=[True, False], rows=rows, **kw).float()
        _rows_match(got, ref1, _up(rows, 8, 64), rows)
    hip.check_range()


@pytest.mark.parametrize("form", ["f64", "u8", "u16"])
def test_dec23_rows(dev, net, nan_empty, form):
    """dec23_synth_kernel in its fp64, 8-bit and 16-bit output forms: the tile walk stops at the tile row (16 frame rows) of the limit."""
    import fldr_hip as hip
    m, a = net
    u = m.vfinet.refine_unet
    H = W = 256
    d1 = hip.spk_pack(_rand(dev, 1, 32, H // 4, W // 4, seed=40).abs())
    e1 = hip.spk_pack(_rand(dev, 1, 16, H // 2, W // 2, seed=41).abs())
    cands = [_rand(dev, 1, 3, H, W, seed=42 + k) for k in range(6)]
    t4 = torch.full((1, 1, 1, 1), 0.3, device=dev)
    T = m.vfinet._host_scalars()[0]
    crop = {"f64": {}, "u8": {"u8_crop": (200, 254)}, "u16": {"u16_crop": (200, 254)}}[form]
    shown = 200 if crop else H
    args = (d1, e1, u.dec2.weight, u.dec2.bias, u.dec3.weight, u.dec3.bias, cands, t4, T)
    ref = hip.dec23_synth(*args, **crop)
    for rows in _limits(16, H):
        got = hip.dec23_synth(*args, rows=rows, **crop)
        _rows_match(got, ref, min(shown, _up(rows, 16, H)), (form, rows))
    hip.check_range()


# ---- the whole forward ---------------------------------------------------------------------------------------------------------

CROPS = (8, 100, 129, 200, 239, 240, 241, 255, 256)


def _forward(m, a, pyr, t, **kw):
    with torch.no_grad():
        out, _ = m([None] * (a.S_tst + 1), t, normInput=pyr, is_training=False, validation=False, **kw)
    return out


@pytest.fixture(scope="module")
def pairs(dev, net):
    """Pyramids of one and of two 256 x 256 pairs, and their unlimited frames in the three output forms (computed once)."""
    import fldr_harness as Hn
    m, a = net
    out = {}
    for B in (1, 2):
        frames = torch.cat([Hn.frames_from_uint8(Hn.synthetic_pair(256, 256, seed=5 + b).to(dev)) for b in range(B)])
        t = torch.tensor([[0.5], [0.3]][:B], device=dev)
        with torch.no_grad():
            pyr = Hn.build_pyramid(Hn.pad_frames(frames, a), a)
        ref = {"f64": _forward(m, a, pyr, t), "u8": _forward(m, a, pyr, t, emit_u8=(256, 256)), "u16": _forward(m, a, pyr, t, emit_u16=(256, 256))}
        assert ref["f64"].dtype == torch.float64 and ref["u8"].dtype == torch.uint8 and ref["u16"].dtype == torch.uint16
        out[B] = (pyr, t, ref)
    torch.cuda.synchronize()
    return out


def _cropped_forwards_match(m, a, pyr, t, ref, Hc):
    got = {"f64": _forward(m, a, pyr, t, crop=(Hc, 256)), "u8": _forward(m, a, pyr, t, emit_u8=(Hc, 256)), "u16": _forward(m, a, pyr, t, emit_u16=(Hc, 256))}
    for form, g in got.items():
        assert g.shape[2] == (256 if form == "f64" else Hc)
        assert torch.equal(g[:, :, :Hc].contiguous().view(torch.uint8), ref[form][:, :, :Hc].contiguous().view(torch.uint8)), (form, Hc)


@pytest.mark.parametrize("Hc", CROPS)
def test_forward_shows_the_same_rows(dev, net, pairs, Hc):
    import fldr_hip as hip
    m, a = net
    pyr, t, ref = pairs[1]
    _cropped_forwards_match(m, a, pyr, t, ref, Hc)
    hip.check_range()


def test_forward_batch_of_two(dev, net, pairs):
    import fldr_hip as hip
    m, a = net
    pyr, t, ref = pairs[2]
    _cropped_forwards_match(m, a, pyr, t, ref, 129)
    hip.check_range()


def test_forward_on_dirty_memory(dev, net, pairs, monkeypatch):
    """The same with the allocator's cached blocks dirtied: NaN-filled tensors of every size the forward allocates are created and freed
    right before each forward, so a kernel that reads a row nobody wrote reads NaN — a different frame, and the range flag."""
    import fldr_hip as hip
    m, a = net
    pyr, t, ref = pairs[1]
    sizes = []
    real = torch.empty

    def recording(*args, **kw):
        x = real(*args, **kw)
        sizes.append(x.numel() * x.element_size())
        return x
    monkeypatch.setattr(torch, "empty", recording)
    _forward(m, a, pyr, t, crop=(100, 256))
    monkeypatch.setattr(torch, "empty", real)
    assert len(sizes) > 20
    torch.cuda.synchronize()

    def dirty():
        junk = [torch.full((max(n // 4, 1),), NAN, device=dev, dtype=torch.float32) for n in sizes for _ in range(2)]
        torch.cuda.synchronize()
        del junk

    for Hc in CROPS:
        for form, kw in (("f64", {"crop": (Hc, 256)}), ("u8", {"emit_u8": (Hc, 256)}), ("u16", {"emit_u16": (Hc, 256)})):
            dirty()
            g = _forward(m, a, pyr, t, **kw)
            assert torch.equal(g[:, :, :Hc].contiguous().view(torch.uint8), ref[form][:, :, :Hc].contiguous().view(torch.uint8)), (form, Hc)
    hip.check_range()


def test_graph_replay_with_a_crop(dev, net):
    """A captured 200 x 256 pair (padded to 256 x 256: the harness passes its 200 rows as the crop) replays the eager frame."""
    import fldr_harness as Hn
    import fldr_hip as hip
    m, a = net
    frames = Hn.frames_from_uint8(Hn.synthetic_pair(200, 256, seed=9).to(dev))
    t = torch.tensor([[0.5]], device=dev)
    g = Hn.GraphedInterpolator(m, a, frames, t, check=True)
    out = g(frames, t)
    torch.cuda.synchronize()
    assert out.shape == (1, 3, 200, 256) and torch.equal(out, Hn.interpolate(m, a, frames, t))
    hip.check_range()
