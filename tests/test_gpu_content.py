"""The whole forward on the content of real video (tests/content_pairs.py) against the CPU oracle: black, flat and fading frames, a
scene cut, letterbox bars, clipped highlights and shadows, sensor grain, a pan of W/12, 5 px stripes and a small object on a flat
background — every case at 960x540, four at 3840x2160 and two at 963x541, t = 0.375.  The network itself produces the flows here
(large and incoherent on a cut or a fade from black), so every kernel of the forward sees them: the PCA projection's global min/max
on constant frames, the feature splats and their candidate bounds, level0_prep's backward warps and masks, the image splats, the
UNet and the blend.

Each run checks (1) the frame against the oracle with the bound of test_4k_strong_nonrigid_motion_matches_oracle (at most 1e-6 of
the values beyond 1e-4, mean error <= 1e-6, >= 90 dB between the rounded 8-bit frames; where the oracle is ill-conditioned, as the
groups below state, with the one-patch allowance, against the oracle's synthesis on the GPU's own level-0 flow, or — stripes — no
further from that synthesis than the oracle is from itself), (2) the level-0 flows (--testgetflowout) against the oracle's at the
bound of test_model_smallest_frame_and_flow_output (2e-4 + 1e-4 |ref|: where a failure starts; on a cut, where the
oracle does not determine its own flow to that bound, the bounded count and size of _cut_flow_bound), (3) a
finite frame and clear status words, (4) libfldr_model.so's uint8 forward == fldr_harness.interpolate_u8 byte for byte and, at 4K,
(5) a second forward bit for bit."""
import pytest
import torch

import content_pairs as C

pytestmark = pytest.mark.gpu

T = 0.375
SEED = 1

# The frame against the oracle at the whole-frame bound.
FULL = [("black", 540, 960), ("clipped", 540, 960), ("flat", 540, 960), ("grain", 540, 960), ("letterbox", 540, 960),
        ("object", 540, 960), ("black", 2160, 3840), ("letterbox", 2160, 3840), ("pan", 2160, 3840), ("clipped", 541, 963)]
# The same bound with the one-patch allowance of test_4k_strong_nonrigid_motion_matches_oracle (see _patch_allowance).
PATCH = [("pan", 540, 960)]
# The oracle frame is ill-conditioned in the level-0 flow (flows that agree to fp32 rounding move it beyond the whole-frame bound; the
# oracle misses that bound against itself across CPU thread counts): the frame is compared, at the whole-frame bound, with
# the oracle's level-0 synthesis run on the GPU's own level-0 flow.
OWN_FLOW = [("cut", 540, 960), ("fade", 540, 960), ("fade_in", 540, 960), ("cut", 541, 963), ("cut", 2160, 3840)]
# As OWN_FLOW, but the frame is held to the oracle's own disagreement with itself (see _stripes_bound).
SELF_BOUND = [("stripes", 540, 960)]
RUNS = [pytest.param(*r, kind, id="%s-%dx%d" % (r[0], r[2], r[1]))
        for kind, runs in (("full", FULL), ("patch", PATCH), ("own_flow", OWN_FLOW), ("self_bound", SELF_BOUND)) for r in runs]

# The oracle's own level-0 flow on a cut is not determined to the flow bound (see _cut_flow_bound).
CUT_FLOW_MAX, CUT_FLOW_FRAC = 0.1, 0.02
BWARP_BAND = 1e-4       # |mask value - 0.999| below which the backward warp's hard threshold (fLDRnet.py:573-574) is ill-conditioned


@pytest.fixture(scope="module")
def hip():
    import fldr_hip
    fldr_hip.lib()
    return fldr_hip


@pytest.fixture(scope="module")
def models(dev):
    """(the default model and args, the --testgetflowout model and args, one NativeModel for the module)."""
    import fldr_harness as Hn
    import fldr_model
    m, _, a = Hn.prepare_model(dev)
    af = Hn.args_config()
    af.testgetflowout = True
    mf, _, af = Hn.prepare_model(dev, args=af)
    nm = fldr_model.NativeModel.from_npz(Hn.DEFAULT_WEIGHTS, device=dev.index or 0)
    yield (m, a), (mf, af), nm
    nm.close()


def _flow_forward(mf, af, frames, t):
    """-> (frame, t-scaled level-0 flows of --testgetflowout, the level-0 flow itself: the pair cache's copy)."""
    import fldr_harness as Hn
    mf.pair_cache = True
    try:
        with torch.no_grad():
            pyr = Hn.build_pyramid(Hn.pad_frames(frames, af), af)
            out, flow = mf([None] * (af.S_tst + 1), t, normInput=pyr, is_training=False, validation=False)
        return out, flow, mf._pair_state["flow0"]
    finally:
        mf.pair_cache = False
        mf._pair_state = None


def _frame_errs(out, ref):
    """-> (max, mean, fraction of the values beyond 1e-4, PSNR of the rounded 8-bit frames, bounding box of the pixels beyond 1e-4)."""
    import fldr_harness as Hn
    err = (out.double() - ref.double()).abs()
    bad = (err > 1e-4).any(1)[0]
    ys, xs = torch.nonzero(bad, as_tuple=True)
    box = (int(ys.min()), int(ys.max()), int(xs.min()), int(xs.max())) if len(ys) else None
    return (err.max().item(), err.mean().item(), (err > 1e-4).double().mean().item(),
            Hn.psnr(Hn.to_uint8_image(ref[0]), Hn.to_uint8_image(out[0])), box)


def _tflow(f0):
    """The oracle's level-0 flow as --testgetflowout returns it (fLDRnet.py:407,535)."""
    return torch.cat([T * f0[:, 2:], (1 - T) * f0[:, :2]], 1).double()


def _cut_flow_bound(flow, want):
    """The level-0 flow check on a cut.  There the oracle does not determine its own level-0 flow to the flow bound 2e-4 + 1e-4 |ref|: its
    fp32 convolutions summed in another order move it — at 960x540, 1 vs 8 CPU threads put 473 values up to 3.1e-2 px apart, 16 vs 4
    threads 303 values up to 1.6e-2 px, and on another CPU 16 vs 4 threads agreed exactly — so a pointwise verdict would be set by the
    machine that runs the oracle.  Measured on MI355X: 0 (960x540) and 277 of 552,960 values (3840x2160, max 2.9e-2 px) beyond the
    bound.  The check: at most CUT_FLOW_FRAC of the values beyond the bound, and none beyond the bound + CUT_FLOW_MAX px (about 3 x the
    oracle's own largest disagreement).  -> (values beyond the bound, largest excess over it)."""
    tol = 2e-4 + 1e-4 * want.abs()
    excess = ((flow - want).abs() - tol).clamp(min=0)
    return int((excess > 0).sum()), float(excess.max())


def _patch_allowance(oracle, box, n_ill, keep_own, shape):
    """pan 960x540 (measured on MI355X: 1.03e-3 of the values beyond 1e-4, all in a 40 x 45 px patch, rows 41-80, columns 25-69; max
    1.24e-2, mean 5.3e-7, 90.1 dB; the oracle reports [0, 1, 0, 0, 4] ill-conditioned feature-splat cells).  The level-0 stages, compared
    with the oracle's on the GPU's own level-0 flow, agree to 1.5e-5 except ONE pixel of flowback_0 (row 64, column 49: 28.8 px against 0),
    where the backward warp's mask value is 2.3e-5 from its hard threshold 0.999 (fLDRnet.py:573-574); the UNet spreads that pixel over
    its receptive field.  The allowance is that of test_4k_strong_nonrigid_motion_matches_oracle's FLDR_PCA_F32=0 branch — every value
    beyond 1e-4 inside one patch of at most 64 x 64 px, and >= 1 ill-conditioned cell in the oracle's report — and the patch must hold a
    pixel whose mask value, for either flowback (oracle on the GPU's level-0 flow), lies within BWARP_BAND of the threshold."""
    assert n_ill >= 1, "differences beyond 1e-4 without any ill-conditioned splat cell"
    assert box[1] - box[0] < 64 and box[3] - box[2] < 64, "differences beyond 1e-4 outside one 64 x 64 patch: %s" % (box,)
    t = torch.tensor(T)
    near = []
    for flo in ((1 - t) * keep_own["flow_01"], t * keep_own["flow_10"]):         # the flows flowback_0 / flowback_1 warp with
        m = oracle.bwarp_mask_value(shape, flo.float())[0, 0]
        near.append(float((m[box[0]:box[1] + 1, box[2]:box[3] + 1] - oracle.BWARP_MASK_THRESHOLD).abs().min()))
    print("  patch %s: closest backward-warp mask value to the threshold in the patch (flowback_0, flowback_1): %.2e, %.2e" % (box, *near))
    assert min(near) < BWARP_BAND, "no backward-warp mask value within %.0e of its threshold in the patch" % BWARP_BAND


def _stripes_bound(own, self_diff):
    """5 px full-contrast stripes: given the GPU's own level-0 flow, the oracle's z0 / z1 and image splats still differ from the GPU's by up
    to 3.8e-4 (the upsampled flows differ by fp32 rounding, <= 1.5e-5 px, and the stripes amplify it), so the frame misses the whole-frame
    bound (measured on MI355X against the oracle's synthesis on the GPU's flow: 2.2e-4 of the values beyond 1e-4, max 4.8e-4, mean 1.9e-6,
    84.2 dB).  The oracle misses it against itself: its run with fp64-accumulated convolutions (oracle.forward(conv_f64=True): another
    fp32-class result, the same on every CPU) differs from the default run by 1.2e-3 of the values beyond 1e-4, max 7.6e-4, mean 5.2e-6,
    79.9 dB (1 vs 8 CPU threads: 2.0e-3, 7.8e-4, 7.4e-6, 78.3 dB).  The frame must be no further from the oracle's synthesis on the GPU's
    flow than the oracle's two runs are from each other, in every one of the four measures."""
    mx, mean, frac, p, _ = own
    smx, smean, sfrac, sp, _ = self_diff
    assert mx <= smx and mean <= smean and frac <= sfrac and p >= sp, (own[:4], self_diff[:4])


@pytest.mark.timeout(600)
@pytest.mark.parametrize("case,H,W,kind", RUNS)
def test_content_forward_matches_oracle(hip, dev, oracle, weights, models, case, H, W, kind):
    import fldr_harness as Hn
    (m, a), (mf, af), nm = models
    u8 = C.pair(case, H, W, seed=SEED)
    frames = Hn.frames_from_uint8(u8)
    t = torch.tensor([[T]])
    fd, td, u8d = frames.to(dev), t.to(dev), u8.to(dev)[None]

    out, flow, flow0 = _flow_forward(mf, af, fd, td)
    out = out[..., :H, :W]
    if H >= 2160:                                                       # (5) determinism of the whole forward at 4K
        out2, flow2, _ = _flow_forward(mf, af, fd, td)
        assert torch.equal(out2[..., :H, :W], out) and torch.equal(flow2, flow), "a second 4K forward differs"
        del out2, flow2
    ref8, _ = Hn.interpolate_u8(m, a, u8d, td)                          # (4) the native library's bytes
    got8 = nm.interpolate_u8(u8d, [T])
    torch.cuda.synchronize()
    status = hip.device_status(reset=False)                              # (3) status words of every forward above
    hip.check_range()
    assert status == 0, "status words after the forwards: %d" % status
    assert got8.shape == ref8.shape == (1, 3, H, W) and torch.equal(got8, ref8), \
        "libfldr_model.so differs from interpolate_u8 at %d values" % int((got8 != ref8).sum())
    out, flow, flow0 = out.double().cpu(), flow.double().cpu(), flow0.cpu()
    assert out.shape == (1, 3, H, W) and torch.isfinite(out).all() and torch.isfinite(flow).all()

    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    pyr = oracle.pad_and_pyramid(frames)
    keep = {}
    with torch.no_grad():
        ref = oracle.forward(weights, pyr, t, keep=keep, conditioning=True)[:, :, :H, :W]
        if kind == "self_bound":
            ref_b = oracle.forward(weights, pyr, t, conv_f64=True)[:, :, :H, :W]
        if kind != "full":
            keep_own = {}
            ref_own = oracle.synthesis_level0(weights, flow0, pyr[0], t.view(1, 1, 1, 1), keep=keep_own)[:, :, :H, :W]
    want = _tflow(keep["flows"][0])
    assert flow.shape == want.shape
    n_ill = sum(keep["ill_conditioned_splat_cells"])
    fbad, fexcess = _cut_flow_bound(flow, want)
    errs = _frame_errs(out, ref)
    print("%s %dx%d t=%g: frame max|err| %.2e mean %.2e, %.2e of the values beyond 1e-4 (bounding box y0, y1, x0, x1: %s), PSNR(8-bit) "
          "%.1f dB; level-0 flow max|err| %.2e (max |flow| %.1f px, %d beyond 2e-4 + 1e-4 |ref|); ill-conditioned feature-splat cells per "
          "level (oracle, eps %.0e, +-%.0e px): %s" % (case, W, H, T, errs[0], errs[1], errs[2], errs[4], errs[3],
                                                        (flow - want).abs().max().item(), want.abs().max().item(),
                                                        int(((flow - want).abs() > 2e-4 + 1e-4 * want.abs()).sum()),
                                                        oracle.SPLAT_COND_EPS, oracle.SPLAT_COND_DELTA, keep["ill_conditioned_splat_cells"]))
    if kind != "full":
        own = _frame_errs(out, ref_own)
        print("  against the oracle's synthesis on the GPU's level-0 flow: max|err| %.2e mean %.2e, %.2e of the values beyond 1e-4, "
              "PSNR(8-bit) %.1f dB" % own[:4])
    if kind == "self_bound":
        self_diff = _frame_errs(ref_b, ref)
        print("  the oracle with fp64-accumulated convolutions against the default run: max %.2e mean %.2e, %.2e beyond 1e-4, %.1f dB"
              % self_diff[:4])
    if case == "cut":                                                   # (2) the level-0 flows
        assert fbad <= CUT_FLOW_FRAC * want.numel() and fexcess <= CUT_FLOW_MAX, (fbad, fexcess)
    else:
        assert fbad == 0, "level-0 flows off the oracle's at %d values" % fbad
    if kind == "self_bound":                                            # (1) the frame
        _stripes_bound(own, self_diff)
        return
    mx, mean, frac, p, box = own if kind == "own_flow" else errs
    if kind == "patch" and frac > 1e-6:
        _patch_allowance(oracle, box, n_ill, keep_own, (1, 1) + tuple(pyr[0].shape[-2:]))
        frac = 0.0
    assert frac <= 1e-6 and mean <= 1e-6 and p >= 90.0, "frame: %.2e of the values beyond 1e-4, mean %.2e, %.1f dB" % (frac, mean, p)
