"""The 10-bit path on the GPU: the 16-bit ingest (fldr_ingest_pyramid_u16), the 16-bit rounded output of the fused synthesis
(fldr_dec23_synth_u16) with its reference fldr_quantize_u16, and the two 10-bit forms of the C model API (FLDR_MODEL_IN_U10_PLANAR /
FLDR_MODEL_OUT_U10_PLANAR), and the video API at depth 10 (P010 and yuv420p10le against tests/yuv_hd_oracle.py, sessions, the C example).
Every comparison is exact unless it says otherwise.

10-bit frames are uint16 tensors with code values 0 .. 1023.  Test frames are made from fldr_harness.synthetic_pair's texture at ten
bits (the 8-bit recipe with 1023 in place of 255), so they use the low two bits an 8-bit frame does not have."""
import ctypes
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXV = 1023


@pytest.fixture(scope="module")
def hip():
    import fldr_hip
    fldr_hip.lib()
    return fldr_hip


@pytest.fixture(scope="module")
def py_model(dev):
    """(DCTXVFInet, args, NativeModel) at the shipped pyramid depth."""
    import fldr_harness as Hn
    import fldr_model
    m, _, a = Hn.prepare_model(dev)
    nm = fldr_model.NativeModel.from_module(m)
    yield m, a, nm
    nm.close()


def pair10(H, W, seed=0, quadrant=False):
    """fldr_harness.synthetic_pair at ten bits: uint16 [2,3,H,W], code values 0 .. 1023."""
    import fldr_harness as Hn
    base = Hn.texture(H + 64, W + 64, seed)
    I0 = base[..., 32:H + 32, 32:W + 32]
    if not quadrant:
        I1 = base[..., 36:H + 36, 38:W + 38]
    else:
        I1 = I0.clone()
        h2, w2 = H // 2, W // 2
        for (ys, xs, dy, dx) in ((0, 0, 8, 12), (0, 1, -8, 12), (1, 0, 8, -12), (1, 1, -8, -12)):
            y0, x0 = ys * h2, xs * w2
            I1[..., y0:y0 + h2, x0:x0 + w2] = base[..., 32 + y0 + dy:32 + y0 + dy + h2, 32 + x0 + dx:32 + x0 + dx + w2]
    q = lambda a: (a.clamp(0, 1) * MAXV).round().to(torch.int32).to(torch.uint16)
    return torch.stack([q(I0[0]), q(I1[0])], 0)


def i32(x):
    """uint16 tensors compared / counted as int32 (torch implements few operations on uint16)."""
    return x.cpu().to(torch.int32)


def norm10(u16):
    """The definition of the 10-bit ingest, by torch on the CPU: u16.float() / 1023 * 2 - 1, one rounding per operation."""
    f = u16.cpu().to(torch.int32).to(torch.float32) / float(MAXV)
    f = f * 2.0
    return f - 1.0


def level0_ref(u16, n_levels):
    """[B,2,3,H,W] uint16 -> the reference level 0 [B,3,2,Hp,Wp]: normalised, reflect-padded right / bottom (main.py:848)."""
    B, T, C, H, W = u16.shape
    div = (2 ** (n_levels - 1)) * 8
    Hp, Wp = (H + div - 1) // div * div, (W + div - 1) // div * div
    x = norm10(u16).permute(0, 2, 1, 3, 4).reshape(B, 6, H, W)
    x = F.pad(x, (0, Wp - W, 0, Hp - H), mode="reflect")
    return x.reshape(B, 3, 2, Hp, Wp)


# ---- libfldr_hip.so: the 16-bit ingest ----------------------------------------------------------------------------------------------
INGEST_CASES = [(200, 328, 6, 1), (260, 515, 6, 2), (130, 258, 4, 1), (300, 522, 7, 1), (64, 70, 3, 1), (2160, 3840, 6, 1)]


@pytest.mark.parametrize("case", INGEST_CASES)
@pytest.mark.parametrize("offset", [0, 1])
def test_ingest_pyramid_u16_levels(hip, dev, case, offset):
    """Level 0 is torch's ((u16.float() / 1023) * 2 - 1), reflect-padded, bit for bit; every further level is fldr_pyramid_bicubic of that
    level 0 bit for bit.  The cases of test_fused_ingest_pyramid_bit_identical, each also with the base pointer one element into its
    buffer (not 8-byte aligned: the per-pixel path)."""
    H, W, nl, B = case
    u16 = torch.stack([pair10(H, W, seed=20 + k, quadrant=True) for k in range(B)], 0)
    buf = torch.zeros(u16.numel() + 4, dtype=torch.int16, device=dev).view(torch.uint16)
    view = buf[offset:offset + u16.numel()].view(u16.shape)
    view.copy_(u16.to(dev))
    assert view.data_ptr() % 8 == 2 * offset
    got = hip.ingest_pyramid_u16(view, nl)
    assert len(got) == nl
    ref0 = level0_ref(u16, nl)
    assert got[0].shape == ref0.shape and torch.equal(got[0].cpu(), ref0)
    Hp, Wp = ref0.shape[-2:]
    for i in range(1, nl):
        lv = torch.empty(B, 3, 2, Hp >> i, Wp >> i, device=dev)
        rc = hip.lib().fldr_pyramid_bicubic(ctypes.c_void_p(got[0].data_ptr()), ctypes.c_void_p(lv.data_ptr()), B * 6, Hp, Wp, 1 << i, None)
        assert rc == 0
        torch.cuda.synchronize()
        assert got[i].shape == lv.shape and torch.equal(got[i], lv), (i, (got[i] - lv).abs().max().item())
    # the plain per-level path (what deeper pyramids use) gives the same level 0
    prev = hip.INGEST_FUSED
    try:
        hip.INGEST_FUSED = False
        plain = hip.ingest_pyramid_u16(view, nl)
    finally:
        hip.INGEST_FUSED = prev
    for i in range(nl):
        assert torch.equal(plain[i], got[i]), i


@pytest.mark.parametrize("size", [(200, 500), (256, 256), (130, 300)])
def test_ingest_u16_matches_the_cpu_caller(hip, oracle, dev, size):
    """Against the reference's CPU pre-processing fed u16 / 1023 * 2 - 1, within test_gpu_ingest_matches_cpu_caller's 2e-6."""
    H, W = size
    u16 = pair10(H, W, seed=6, quadrant=True)
    frames = norm10(u16).permute(1, 0, 2, 3).unsqueeze(0).contiguous()          # [1,3,2,H,W]
    ref = oracle.pad_and_pyramid(frames)
    got = hip.ingest_pyramid_u16(u16.unsqueeze(0).to(dev))
    assert len(got) == 6
    assert torch.equal(got[0].cpu(), ref[0])
    for i in range(1, 6):
        err = (got[i].cpu() - ref[i]).abs().max().item()
        assert err <= 2e-6, (i, err)


@pytest.mark.parametrize("case", [(200, 328, 6, 1), (130, 258, 4, 2)])
def test_ingest_u16_with_maxval_255_gives_the_8_bit_bits(hip, dev, case):
    import fldr_harness as Hn
    H, W, nl, B = case
    u8 = torch.stack([Hn.synthetic_pair(H, W, seed=3 + k, quadrant=True) for k in range(B)], 0).to(dev)
    want = hip.ingest_pyramid(u8, nl)
    got = hip.ingest_pyramid_u16(u8.cpu().to(torch.int32).to(torch.uint16).to(dev), nl, maxval=255)
    for i in range(nl):
        assert torch.equal(got[i], want[i]), i


def test_ingest_u16_clamps_values_above_the_white_level(hip, dev):
    u16 = pair10(64, 72, seed=1).unsqueeze(0)
    hot = i32(u16)
    hot[0, 0, 1, 5, 7] = 4095
    hot[0, 1, 2, 63, 71] = 65535
    cl = hot.clamp(max=MAXV).to(torch.uint16)
    hot = hot.to(torch.uint16)
    a, b = hip.ingest_pyramid_u16(hot.to(dev), 3), hip.ingest_pyramid_u16(cl.to(dev), 3)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---- libfldr_hip.so: the rounded 16-bit frame ---------------------------------------------------------------------------------------
def quant_ref(x64, H, W):
    """round_half_even(clip((x + 1) / 2, 0, 1) * 1023) by torch in fp64, cropped."""
    v = ((x64[:, :, :H, :W].cpu().double() + 1.0) / 2.0).clamp(0.0, 1.0) * float(MAXV)
    return torch.round(v).to(torch.int32)


def test_quantize_u16_is_round_half_even(hip, dev):
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(2, 3, 40, 72, generator=g, dtype=torch.float64) * 2.4 - 1.2)
    # the ends of the range, values beyond them, both zeros and the neighbours of +-1
    x[0, 0, 0, :8] = torch.tensor([-1.0, 1.0, -1.5, 1.5, 0.0, -0.0, 1.0 - 2.0 ** -52, -1.0 + 2.0 ** -52], dtype=torch.float64)
    x[0, 0, 1, 0] = float("nan")
    got = hip.quantize_u16(x.to(dev), 37, 71)
    want = quant_ref(x, 37, 71)
    want[0, 0, 1, 0] = 0                                                     # a poisoned frame: 0, as the 8-bit form
    assert got.dtype == torch.uint16 and got.shape == (2, 3, 37, 71)
    assert torch.equal(i32(got).cpu(), want)
    got32 = hip.quantize_u16(x.float().to(dev), 37, 71)
    want32 = quant_ref(x.float().double(), 37, 71)
    want32[0, 0, 1, 0] = 0
    assert torch.equal(i32(got32).cpu(), want32)


def _dec23_inputs(N, h, w, dev, seed=65):
    g = torch.Generator().manual_seed(seed)
    dec1 = torch.rand(N, 32, h // 2, w // 2, generator=g) * 1.5
    enc1 = torch.rand(N, 16, h, w, generator=g) * 1.5
    w2 = torch.randn(16, 48, 3, 3, generator=g) / 12
    b2 = torch.randn(16, generator=g) * 0.2
    w3 = torch.randn(6, 16, 3, 3, generator=g) / 6
    b3 = torch.randn(6, generator=g) * 0.3
    # candidates a little outside [-1, 1] so that both clamps act
    cands = [(torch.rand(N, 3, 2 * h, 2 * w, generator=g) * 2.2 - 1.1).to(dev) for _ in range(4)]
    pair = (torch.rand(N, 3, 2, 2 * h, 2 * w, generator=g) * 2.2 - 1.1).to(dev)
    cands += [pair[:, :, 0], pair[:, :, 1]]
    t = torch.tensor([[0.25], [0.6]])[:N]
    return lambda hip: (hip.spk_pack(dec1.to(dev)), hip.spk_pack(enc1.to(dev)), w2.to(dev), b2.to(dev), w3.to(dev), b3.to(dev), cands, t.to(dev),
                        1.5616)


@pytest.mark.parametrize("N,h,w,crop", [(1, 128, 128, (256, 256)), (2, 52, 84, (101, 166)), (1, 1080, 1920, (2160, 3840)),
                                        (1, 1080, 2048, (2160, 4096))])
def test_fused_u16_frame_is_the_quantised_fp64_frame(hip, dev, N, h, w, crop):
    """fldr_dec23_synth_u16 == fldr_quantize_u16 of fldr_dec23_synth's fp64 frame == torch's fp64 rounding of it; 256 x 256, a case cropped
    to an odd height from a padded frame, 2160 x 3840 and 2160 x 4096."""
    args = _dec23_inputs(N, h, w, dev)(hip)
    f64 = hip.dec23_synth(*args)
    u16 = hip.dec23_synth(*args, u16_crop=crop)
    q = hip.quantize_u16(f64, crop[0], crop[1])
    torch.cuda.synchronize()
    assert u16.dtype == torch.uint16 and u16.shape == (N, 3) + crop
    assert torch.equal(i32(u16), i32(q))
    assert torch.equal(i32(q).cpu(), quant_ref(f64, crop[0], crop[1]))
    assert int(i32(u16).max()) == MAXV and int(i32(u16).min()) == 0          # both ends of the range occur
    hip.check_range()


@pytest.mark.parametrize("shape", [(2, 40, 100), (2, 80, 264)])
def test_fused_u16_bits_independent_of_workgroups(hip, dev, shape):
    """tests/test_gpu_schedule.py's forced-workgroup-count walk for the 16-bit instantiation (the test build's knob)."""
    N, h, w = shape
    crop = (2 * h - 3, 2 * w - 2)
    with hip.test_hooks() as L:
        args = _dec23_inputs(N, h, w, dev)(hip)
        prev = L.fldr_debug_dec23_wgs_per_xcd(0)
        try:
            dflt = hip.dec23_synth(*args, u16_crop=crop)
            f64 = hip.dec23_synth(*args)
            for v in (1, 2, 3):
                assert L.fldr_debug_dec23_wgs_per_xcd(v) == v
                got = hip.dec23_synth(*args, u16_crop=crop)
                assert torch.equal(i32(got), i32(dflt)), v
        finally:
            L.fldr_debug_dec23_wgs_per_xcd(prev)
        assert L.fldr_debug_ring_timeouts() == 0
        assert torch.equal(i32(dflt), i32(hip.quantize_u16(f64, crop[0], crop[1])))
    tiles = N * math.ceil(h / 8) * math.ceil(w / 32)
    print("dec23 u16 %s: %d tiles, up to %d per workgroup at one workgroup per XCD" % (shape, tiles, math.ceil(tiles / 8)))


# ---- the harness ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(256, 384), (200, 301)])
def test_interpolate_u16_is_the_quantised_forward(hip, dev, py_model, H, W):
    import fldr_harness as Hn
    m, a, _ = py_model
    u16 = pair10(H, W, seed=5).unsqueeze(0).to(dev)
    t = torch.tensor([[0.375]], device=dev)
    got = Hn.interpolate_u16(m, a, u16, t)
    pyr = hip.ingest_pyramid_u16(u16, a.S_tst + 1)
    with torch.no_grad():
        f64, _ = m([None] * (a.S_tst + 1), t, normInput=pyr, is_training=False, validation=False)
    assert got.dtype == torch.uint16 and got.shape == (1, 3, H, W)
    assert torch.equal(i32(got).cpu(), quant_ref(f64, H, W))


# ---- libfldr_model.so ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,t", [(256, 256, 0.5), (200, 500, 0.125), (2160, 3840, 0.5)])
def test_u10_in_f64_out_equals_python_forward(hip, dev, py_model, H, W, t):
    """The pattern of test_fp64_frame_equals_python_forward: IN_U10_PLANAR + OUT_F64 is DCTXVFInet.forward on ingest_pyramid_u16's levels."""
    import fldr_harness as Hn
    import fldr_model
    m, a, nm = py_model
    u16 = pair10(H, W, seed=3).unsqueeze(0).to(dev)
    pyr = hip.ingest_pyramid_u16(u16, 6)
    Hp, Wp = fldr_model.padded_size(H, W)
    kept = [torch.full((1, 3, 2, Hp >> i, Wp >> i), float("nan"), device=dev) for i in range(6)]
    got = nm.interpolate_u10(u16, [t], out="f64", pyramid_out=kept)[:, :, :H, :W]
    frames = norm10(u16)[0].permute(1, 0, 2, 3).unsqueeze(0).to(dev)             # only its shape is used once a pyramid is given
    ref = Hn.interpolate(m, a, frames, torch.tensor([[t]], device=dev), pyramid=pyr)
    torch.cuda.synchronize()
    for i in range(6):
        assert torch.equal(kept[i], pyr[i]), i
    assert got.dtype == torch.float64 and got.shape == ref.shape
    assert torch.equal(got, ref), float((got - ref).abs().max())


def test_u10_in_f64_out_matches_the_oracle(dev, py_model, oracle, weights):
    """256 x 256, t = 0.5 against the CPU oracle fed pad_and_pyramid(u16 / 1023 * 2 - 1), within test_fp64_frame_matches_the_oracle's 2e-5."""
    _, _, nm = py_model
    u16 = pair10(256, 256, seed=0).unsqueeze(0)
    got = nm.interpolate_u10(u16.to(dev), [0.5], out="f64")[:, :, :256, :256]
    frames = norm10(u16)[0].permute(1, 0, 2, 3).unsqueeze(0).contiguous()
    with torch.no_grad():
        ref = oracle.forward(weights, oracle.pad_and_pyramid(frames), torch.tensor([[0.5]]))[:, :, :256, :256]
    assert (got.cpu() - ref).abs().max().item() < 2e-5


@pytest.mark.parametrize("H,W", [(256, 384), (200, 301), (2160, 3840)])
def test_u10_out_is_the_quantised_fp64_frame(dev, py_model, H, W):
    """An even width (the fused 16-bit form) and an odd one (fp64 frame + fldr_quantize_u16)."""
    _, _, nm = py_model
    u16 = pair10(H, W, seed=5).unsqueeze(0).to(dev)
    f64 = nm.interpolate_u10(u16, [0.375], out="f64")
    got = nm.interpolate_u10(u16, [0.375])
    assert got.dtype == torch.uint16 and got.shape == (1, 3, H, W)
    assert torch.equal(i32(got).cpu(), quant_ref(f64, H, W))


@pytest.mark.parametrize("H,W", [(256, 384), (200, 301)])
def test_mixed_depths(dev, py_model, H, W):
    """10-bit in with 8-bit out is the 8-bit rounding of the 10-bit pair's fp64 frame; 8-bit in with 10-bit out is the 10-bit rounding of
    the 8-bit pair's fp64 frame."""
    import fldr_harness as Hn
    import fldr_hip
    _, _, nm = py_model
    u16 = pair10(H, W, seed=7).unsqueeze(0).to(dev)
    f64 = nm.interpolate_u10(u16, [0.5], out="f64")
    _, want8 = fldr_hip.frame_metrics(f64, H, W, None, want_u8=True)
    assert torch.equal(nm.interpolate_u10(u16, [0.5], out="u8"), want8)
    u8 = Hn.synthetic_pair(H, W, seed=7).unsqueeze(0).to(dev)
    Hp, Wp = f64.shape[-2:]
    pyr = fldr_hip.ingest_pyramid(u8, 6)
    f64_8 = nm.forward_pyramid(pyr, [0.5], H, W)
    assert torch.equal(i32(nm.interpolate_u10(u8, [0.5])).cpu(), quant_ref(f64_8, H, W))


def test_seven_outputs_equal_seven_single_forwards(dev, py_model):
    _, _, nm = py_model
    H, W = 200, 328
    u16 = pair10(H, W, seed=9).unsqueeze(0).to(dev)
    ts = [(k + 1) / 8 for k in range(7)]
    multi = nm.interpolate_u10(u16, ts)
    for k, t in enumerate(ts):
        assert torch.equal(i32(multi[k:k + 1]), i32(nm.interpolate_u10(u16, [t]))), k
    assert not torch.equal(i32(multi[0]), i32(multi[6]))


def test_three_streams_equal_one_at_a_time(dev, py_model):
    _, _, nm = py_model
    H, W = 256, 384
    pairs = [pair10(H, W, seed=11 + k).unsqueeze(0).to(dev) for k in range(3)]
    want = [nm.interpolate_u10(p, [0.5]) for p in pairs]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=dev) for _ in range(3)]
    wss = [nm.workspace(H, W, 1) for _ in range(3)]
    got = [None] * 3
    for rep in range(3):
        for k in range(3):
            with torch.cuda.stream(streams[k]):
                got[k] = nm.interpolate_u10(pairs[k], [0.5], ws=wss[k], stream=streams[k])
    torch.cuda.synchronize()
    for k in range(3):
        assert torch.equal(i32(got[k]), i32(want[k])), k


def test_captured_graph_replays_the_eager_words_and_reads_t(dev, py_model):
    import fldr_model as M
    _, _, nm = py_model
    H, W = 256, 256
    u16 = pair10(H, W, seed=13).unsqueeze(0).to(dev)
    want = {t: nm.interpolate_u10(u16, [t]).clone() for t in (0.25, 0.75)}
    tt = torch.tensor([0.25], device=dev)
    ws = nm.workspace(H, W, 1)
    out = torch.zeros(1, 3, H, W, dtype=torch.int16, device=dev).view(torch.uint16)
    io = M.IO()
    io.batch, io.H, io.W, io.input, io.frames_u8 = 1, H, W, M.IN_U10_PLANAR, u16.data_ptr()
    io.n_t, io.t, io.output = 1, tt.data_ptr(), M.OUT_U10_PLANAR
    ptrs = (ctypes.c_void_p * 1)(out.data_ptr())
    io.out = ctypes.cast(ptrs, ctypes.POINTER(ctypes.c_void_p))
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        assert nm.forward(io, ws, s) == 0                                     # warm: everything that allocates lazily has run
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        assert nm.forward(io, ws, s) == 0
    out.view(torch.int16).zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(i32(out), i32(want[0.25]))
    tt.fill_(0.75)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(i32(out), i32(want[0.75]))


def test_refused_calls_write_nothing(dev, py_model):
    import fldr_model as M
    _, _, nm = py_model
    H, W = 200, 328
    u16 = pair10(H, W, seed=1).unsqueeze(0).to(dev)
    tt = torch.tensor([0.5], device=dev)
    ws = torch.full((nm.workspace_bytes(H, W, 1),), 0x5a, dtype=torch.uint8, device=dev)
    buf = torch.full((3 * H * W + 8,), 0x5a5a, dtype=torch.int16, device=dev).view(torch.uint16)

    def io_for(inp, outp, out_ptr, frames_ptr):
        io = M.IO()
        io.batch, io.H, io.W, io.input, io.frames_u8 = 1, H, W, inp, frames_ptr
        io.n_t, io.t, io.output = 1, tt.data_ptr(), outp
        ptrs = (ctypes.c_void_p * 1)(out_ptr)
        io.out = ctypes.cast(ptrs, ctypes.POINTER(ctypes.c_void_p))
        io._keep = ptrs
        return io
    cases = [(io_for(4, M.OUT_U10_PLANAR, buf.data_ptr(), u16.data_ptr()), M.E_ARG),                  # beyond the last input form
             (io_for(M.IN_U10_PLANAR, 4, buf.data_ptr(), u16.data_ptr()), M.E_ARG),                   # beyond the last output form
             (io_for(M.IN_U10_PLANAR, M.OUT_U10_PLANAR, buf.data_ptr(), None), M.E_ARG),              # no frames
             (io_for(M.IN_U10_PLANAR, M.OUT_U10_PLANAR, buf.data_ptr(), u16.data_ptr() + 1), M.E_ARG),  # odd frame address
             (io_for(M.IN_U10_PLANAR, M.OUT_U10_PLANAR, buf.data_ptr() + 2, u16.data_ptr()), M.E_ARG)]  # output not 4-byte aligned
    for io, code in cases:
        assert nm.forward(io, ws) == code
    io = io_for(M.IN_U10_PLANAR, M.OUT_U10_PLANAR, buf.data_ptr(), u16.data_ptr())
    assert nm.forward(io, ws[:ws.numel() - 256]) == M.E_WORKSPACE
    torch.cuda.synchronize()
    assert bool((ws == 0x5a).all()) and bool((i32(buf) == 0x5a5a).all())
    assert nm.forward(io, ws) == 0                                            # and the same call, unbroken, runs
    torch.cuda.synchronize()
    assert not bool((i32(buf[:3 * H * W]) == 0x5a5a).all())


def test_workspace_bytes_are_the_parents(py_model):
    """The 10-bit forms need no new workspace region: fldr_model_workspace_bytes returns what it returned before they existed (values
    recorded from the parent commit's library, tests/golden/model_workspace_bytes.json)."""
    _, _, nm = py_model
    rows = json.load(open(os.path.join(ROOT, "tests", "golden", "model_workspace_bytes.json")))["test_scales_5"]
    assert len(rows) >= 5
    for H, W, n_t, want in rows:
        assert nm.workspace_bytes(H, W, n_t) == want, (H, W, n_t)


# ---- content: why ten bits ------------------------------------------------------------------------------------------------------------
def test_a_smooth_ramp_keeps_more_levels_than_eight_bits_can(dev, py_model):
    """A horizontal ramp over 200 ten-bit codes across the width, moved 6 pixels between the frames.  The 10-bit forward's output holds
    more distinct values than the 8-bit forward of the same frames shifted right by two bits can hold at all (256; about 50 on this
    ramp)."""
    _, _, nm = py_model
    H, W = 256, 512
    x = torch.arange(W + 6, dtype=torch.float64)
    ramp = torch.round(400.0 + 200.0 * x / (W + 5)).to(torch.int32)            # codes 400 .. 600
    f0, f1 = ramp[6:6 + W], ramp[:W]
    pair = torch.stack([f0, f1]).view(2, 1, 1, W).expand(2, 3, H, W).contiguous()
    u16 = pair.to(torch.uint16).unsqueeze(0).to(dev)
    u8 = (pair >> 2).to(torch.uint8).unsqueeze(0).to(dev)
    out10 = i32(nm.interpolate_u10(u16, [0.5]))[0, 1, 32:H - 32, 32:W - 32]
    out8 = nm.interpolate_u8(u8, [0.5])[0, 1, 32:H - 32, 32:W - 32]
    n10, n8 = int(torch.unique(out10).numel()), int(torch.unique(out8).numel())
    print("distinct values on the ramp: 10-bit forward %d, 8-bit forward %d" % (n10, n8))
    assert n8 <= 256 and n10 > n8


# ---- libfldr_video.so at depth 10: P010 (nv12) and yuv420p10le (i420) ---------------------------------------------------------------
import functools  # noqa: E402
import shutil  # noqa: E402
import subprocess  # noqa: E402

import numpy as np  # noqa: E402

import yuv_hd_oracle as HD  # noqa: E402
import yuv_oracle as O8  # noqa: E402

PKG = os.path.join(ROOT, "fldr-vfi_amd")
SIZES = [(256, 256), (201, 333), (1080, 1920), (2160, 3840), (2160, 4096)]       # tests/test_gpu_video.py's
FORMATS = [(m, r) for m in HD.MATRICES for r in HD.RANGES]


@pytest.fixture(scope="module")
def nv(dev):
    import fldr_harness as Hn
    import fldr_model
    import fldr_video
    nm = fldr_model.NativeModel.from_npz(Hn.DEFAULT_WEIGHTS, device=dev.index or 0)
    yield fldr_video.NativeVideo(nm)
    nm.close()


@functools.lru_cache(maxsize=2)
def _yuv10_pair(H, W, mat, rng, seed=0):
    """((Y, U, V), (Y, U, V)) code values of a 10-bit synthetic pair, and the oracle's 10-bit BGR frames [2,3,H,W] of those planes."""
    bgr0 = pair10(H, W, seed=seed).numpy()
    yuv = [HD.bgr_to_yuv420(bgr0[i], mat, rng, 10) for i in range(2)]
    bgr = np.stack([HD.yuv420_to_bgr(*yuv[i], mat, rng, 10) for i in range(2)])
    return yuv, bgr


def _to_dev(planes, dev, pad=0, fill=0, offset=0):
    """Device copies of host planes (uint8 or uint16); pad > 0: each plane a view into a buffer `pad` elements wider per row (gap
    elements = fill), starting `offset` elements into it.  -> (views, buffers)."""
    views, bufs = [], []
    for p in planes:
        r, c = p.shape
        t = torch.from_numpy(np.ascontiguousarray(p))
        if not pad and not offset:
            views.append(t.to(dev)); bufs.append(None)
            continue
        pitch = c + pad
        host = np.full(r * pitch + offset + pitch, fill, p.dtype)
        host[offset:offset + r * pitch].reshape(r, pitch)[:, :c] = p
        buf = torch.from_numpy(host).to(dev)
        views.append(buf[offset:offset + r * pitch].view(r, pitch)[:, :c]); bufs.append(buf)
    return tuple(views), bufs


def _host(frame):
    return tuple(p.cpu().numpy() for p in frame)


def _fmt(layout, mat, rng, depth=10):
    import fldr_video
    return fldr_video.Format(layout, mat, rng, depth)


def _check_out10(frame, layout, want_yuv):
    planes = _host(frame)
    if layout == "nv12":
        assert all(int((p & 63).max()) == 0 for p in planes)                      # P010: the low six bits are written as zero
    else:
        assert all(int(p.max()) <= 1023 for p in planes)
    for g, w in zip(HD.unpack_planes(planes, layout, 10), want_yuv):
        assert np.array_equal(g, w), layout


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("mat,rng", FORMATS)
def test_yuv10_forward_equals_model_on_oracle_bgr(nv, dev, H, W, mat, rng):
    """For P010 and yuv420p10le (with random bits in the six the container does not use): the input kernel gives the oracle's 10-bit BGR
    words, the forward is the model's U10 forward on them, the output kernel gives the oracle's YUV of the model's planar output."""
    yuv, bgr = _yuv10_pair(H, W, mat, rng)
    ref = i32(nv.model.interpolate_u10(torch.from_numpy(bgr)[None].to(dev), [0.5])[0]).numpy()
    dirt = np.random.default_rng(H + W)
    for layout in ("nv12", "i420"):
        frames = [_to_dev(HD.pack_planes(*yuv[i], layout, 10, dirt=dirt), dev)[0] for i in range(2)]
        fmt = _fmt(layout, mat, rng)
        ws = nv.workspace(H, W, 1)
        outs = nv.forward(frames, [0.5], fmt, fmt, ws=ws)
        torch.cuda.synchronize()
        pair, planar = nv.planar(ws, H, W, 1, 10, 10)
        assert np.array_equal(i32(pair).numpy(), bgr.astype(np.int32)), layout
        got = i32(planar[0]).numpy()
        assert np.array_equal(got, ref), layout
        _check_out10(outs[0], layout, HD.bgr_to_yuv420(got.astype(np.uint16), mat, rng, 10))


@pytest.mark.parametrize("H,W,pad,offset", [(256, 256, 32, 0), (201, 333, 13, 5), (1080, 1920, 64, 2048)])
def test_pitched_10_bit_planes_are_not_touched_outside_their_rows(nv, dev, H, W, pad, offset):
    mat, rng = "bt709", "limited"
    yuv, _ = _yuv10_pair(H, W, mat, rng, seed=2)
    for layout in ("nv12", "i420"):
        fmt = _fmt(layout, mat, rng)
        packed = [_to_dev(HD.pack_planes(*yuv[i], layout, 10), dev)[0] for i in range(2)]
        want = nv.forward(packed, [0.5], fmt, fmt)
        # inputs: gaps filled with a value that would change the result if read; outputs: gaps filled with a sentinel
        frames = [_to_dev(HD.pack_planes(*yuv[i], layout, 10), dev, pad=pad, fill=0xffff, offset=offset)[0] for i in range(2)]
        shapes = [tuple(p.shape) for p in packed[0]]
        out_views, out_bufs = _to_dev([np.zeros(s, np.uint16) for s in shapes], dev, pad=pad, fill=0xa5a5, offset=offset)
        for v in out_views:
            v.view(torch.int16).fill_(0x1111)
        nv.forward(frames, [0.5], fmt, fmt, outs=[out_views])
        torch.cuda.synchronize()
        for v, w, buf, s in zip(out_views, want[0], out_bufs, shapes):
            assert np.array_equal(v.cpu().numpy(), w.cpu().numpy()), layout
            host = buf.cpu().numpy()
            r, c = s
            pitch = c + pad
            body = host[offset:offset + r * pitch].reshape(r, pitch)
            assert (host[:offset] == 0xa5a5).all() and (host[offset + r * pitch:] == 0xa5a5).all() and (body[:, c:] == 0xa5a5).all(), layout


@pytest.mark.parametrize("H,W", [(256, 256), (201, 333)])
def test_mixed_depths_through_the_video_api(nv, dev, H, W):
    """10-bit in with 8-bit out, and 8-bit in with 10-bit out: each side is its own conversion around the model's mixed forward."""
    import fldr_harness as Hn
    mat, rng = "bt709", "limited"
    yuv, bgr = _yuv10_pair(H, W, mat, rng, seed=4)
    frames = [_to_dev(HD.pack_planes(*yuv[i], "nv12", 10), dev)[0] for i in range(2)]
    ws = nv.workspace(H, W, 1)
    outs = nv.forward(frames, [0.5], _fmt("nv12", mat, rng, 10), _fmt("i420", mat, rng, 8), ws=ws)
    torch.cuda.synchronize()
    pair, planar = nv.planar(ws, H, W, 1, 10, 8)
    assert np.array_equal(i32(pair).numpy(), bgr.astype(np.int32))
    ref8 = nv.model.interpolate_u10(torch.from_numpy(bgr)[None].to(dev), [0.5], out="u8")[0].cpu().numpy()
    assert planar[0].dtype == torch.uint8 and np.array_equal(planar[0].cpu().numpy(), ref8)
    for g, w in zip(_host(outs[0]), O8.bgr_to_yuv420(ref8, mat, rng)):
        assert g.dtype == np.uint8 and np.array_equal(g, w)
    # the reverse
    u8 = Hn.synthetic_pair(H, W, seed=4).numpy()
    yuv8 = [O8.bgr_to_yuv420(u8[i], mat, rng) for i in range(2)]
    bgr8 = np.stack([O8.yuv420_to_bgr(*yuv8[i], mat, rng) for i in range(2)])
    frames8 = [tuple(torch.from_numpy(p).to(dev) for p in yuv8[i]) for i in range(2)]
    outs = nv.forward(frames8, [0.5], _fmt("i420", mat, rng, 8), _fmt("nv12", mat, rng, 10), ws=ws)
    torch.cuda.synchronize()
    pair, planar = nv.planar(ws, H, W, 1, 8, 10)
    assert np.array_equal(pair.cpu().numpy(), bgr8)
    ref10 = i32(nv.model.interpolate_u10(torch.from_numpy(bgr8)[None].to(dev), [0.5])[0]).numpy()
    assert np.array_equal(i32(planar[0]).numpy(), ref10)
    _check_out10(outs[0], "nv12", HD.bgr_to_yuv420(ref10.astype(np.uint16), mat, rng, 10))


def _clip10(H, W, n, seed):
    big = pair10(H + 4 * n, W + 6 * n, seed=seed).numpy()[0]
    return [np.ascontiguousarray(big[:, 4 * k:4 * k + H, 6 * k:6 * k + W]) for k in range(n)]


@pytest.mark.parametrize("layout,n_t", [("nv12", 1), ("i420", 3)])
def test_10_bit_session_pushes_equal_forwards_on_consecutive_frames(nv, dev, layout, n_t):
    import fldr_video
    H, W, mat, rng = 201, 334, "bt709", "limited"
    fmt = _fmt(layout, mat, rng)
    clip = [HD.pack_planes(*HD.bgr_to_yuv420(f, mat, rng, 10), layout, 10) for f in _clip10(H, W, 4, seed=8)]
    s = fldr_video.Session(nv.model, H, W, n_t, fmt, fmt)
    assert s.push(clip[0]) == []
    t = [(k + 1) / (n_t + 1) for k in range(n_t)]
    for k in range(1, 4):
        outs = s.push(clip[k])
        assert len(outs) == n_t
        frames = [_to_dev(clip[k - 1], dev)[0], _to_dev(clip[k], dev)[0]]
        want = nv.forward(frames, t, fmt, fmt)
        torch.cuda.synchronize()
        for j in range(n_t):
            for g, w in zip(outs[j], _host(want[j])):
                assert g.dtype == np.uint16 and np.array_equal(g, w), (k, j)
    s.close()


def test_c_example_with_p10_writes_the_sessions_bytes(nv, dev, clean_launcher, tmp_path):
    import fldr_harness as Hn
    import fldr_video
    H, W, F_ = 256, 448, 2
    frames = [HD.pack_planes(*HD.bgr_to_yuv420(f, "bt709", "limited", 10), "i420", 10) for f in _clip10(H, W, 4, seed=6)]
    raw = [b"".join(p.astype("<u2").tobytes() for p in f) for f in frames]
    (tmp_path / "in.yuv").write_bytes(b"".join(raw))
    exe = str(tmp_path / "fldr_slowmo")
    subprocess.run([shutil.which("cc") or "gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "examples", "fldr_slowmo.c"), "-L" + PKG, "-l:libfldr_video.so", "-l:libfldr_model.so",
                    "-Wl,-rpath," + PKG], check=True)
    cmd = '"%s" "%s" %d %d %d p10 < "%s" > "%s"' % (exe, Hn.DEFAULT_WEIGHTS, W, H, F_, tmp_path / "in.yuv", tmp_path / "out.yuv")
    r = clean_launcher(["sh", "-c", cmd], env=dict(os.environ), timeout=300)
    assert r["rc"] == 0, r
    data = (tmp_path / "out.yuv").read_bytes()
    n = len(raw[0])
    assert n == 2 * (H * W + 2 * (H // 2) * (W // 2)) and len(data) == 7 * n
    got = [data[k * n:(k + 1) * n] for k in range(7)]
    for k in range(4):
        assert got[2 * k] == raw[k], k
    fmt = _fmt("i420", "bt709", "limited")
    s = fldr_video.Session(nv.model, H, W, F_ - 1, fmt, fmt)
    s.push(frames[0])
    for k in range(1, 4):
        outs = s.push(frames[k])
        assert got[2 * k - 1] == b"".join(p.astype("<u2").tobytes() for p in outs[0]), k
    s.close()


def test_u10_forms_at_pyramid_depth_7_use_the_per_level_ingest(hip, dev):
    """Eight levels are more than the one-launch ingest holds: the model then runs fldr_ingest_u16 + fldr_pyramid_bicubic per level.  Its
    fp64 frame is the Python forward on ingest_pyramid_u16's eight levels, its 10-bit frame the rounding of that."""
    import fldr_harness as Hn
    import fldr_model
    a = Hn.args_config(test_scales=7)
    m, _, a = Hn.prepare_model(dev, args=a)
    nm = fldr_model.NativeModel.from_module(m)
    try:
        H, W, t = 520, 530, 0.375
        u16 = pair10(H, W, seed=2).unsqueeze(0).to(dev)
        pyr = hip.ingest_pyramid_u16(u16, 8)
        assert len(pyr) == 8
        frames = norm10(u16)[0].permute(1, 0, 2, 3).unsqueeze(0).to(dev)
        ref = Hn.interpolate(m, a, frames, torch.tensor([[t]], device=dev), pyramid=pyr)
        f64 = nm.interpolate_u10(u16, [t], out="f64")
        assert torch.equal(f64[:, :, :H, :W], ref)
        assert torch.equal(i32(nm.interpolate_u10(u16, [t])), quant_ref(f64, H, W))
    finally:
        nm.close()
