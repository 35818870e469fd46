"""CPU checks of tests/content_pairs.py: every generator is deterministic for a seed and has the property its case names (the zeros,
the bars, the shift, the saturation, the grain), and the oracle is well defined on every case — a finite frame, and a PCA min/max
spread > 0 at every pyramid level (the global rescale of fLDRnet.py:146 divides by it).  The conditioning report printed here is
what tests/test_gpu_content.py compares the kernels against at larger sizes."""
import pytest
import torch

import content_pairs as C

H, W = 192, 320
SIZES = [(192, 320), (540, 960), (541, 963)]


@pytest.mark.parametrize("case", sorted(C.CASES))
def test_generator_is_deterministic_for_a_seed(case):
    a = C.pair(case, H, W, seed=3)
    assert a.shape == (2, 3, H, W) and a.dtype == torch.uint8 and a.is_contiguous()
    assert torch.equal(a, C.pair(case, H, W, seed=3))
    if case not in ("black", "flat"):                                    # the only cases without a texture
        assert not torch.equal(a, C.pair(case, H, W, seed=4))


def test_black_flat_and_fades():
    assert not C.black(H, W).any()
    f = C.flat(H, W)
    for c, v in enumerate(C.FLAT_BGR):
        assert (f[:, c] == v).all()
    fi = C.fade_in(H, W, seed=1)
    assert not fi[0].any() and fi[1].min() == 0 and fi[1].max() == 255
    fd = C.fade(H, W, seed=1)
    assert torch.equal(fd[1], (fd[0].double() * 0.6).round().to(torch.uint8))
    assert fd[0].max() == 255 and fd[1].max() == 153


def test_cut_frames_are_unrelated():
    """No shift of up to 16 px explains I1 by I0: the mean absolute difference stays large at every one."""
    c = C.cut(H, W, seed=1).double()
    m = 16
    mads = [float((c[1, :, m:H - m, m:W - m] - c[0, :, m + dy:H - m + dy, m + dx:W - m + dx]).abs().mean())
            for dy in range(-m, m + 1, 4) for dx in range(-m, m + 1, 4)]
    assert min(mads) > 25.0, min(mads)


@pytest.mark.parametrize("size", [(192, 320), (540, 960), (1080, 1920), (2160, 3840)])
def test_letterbox_bars(size):
    Hs, Ws = size
    top, bottom = C.letterbox_rows(Hs, Ws)
    assert top >= 1 and bottom in (top, top + 1) and abs((Ws / (Hs - top - bottom)) - C.LETTERBOX_ASPECT) < 0.01
    assert top % 8 and (Hs - bottom) % 8, "a bar edge on a multiple of 8 rows"
    if size == (1080, 1920):
        assert (top, bottom) == (138, 139)
    if size == (2160, 3840):
        assert (top, bottom) == (276, 277)
    if Hs > 600:
        return                                                           # the bar geometry only: the 4K pair is built on the GPU box
    lb = C.letterbox(Hs, Ws, seed=2)
    bars = torch.cat([lb[:, :, :top], lb[:, :, Hs - bottom:]], 2)
    assert (bars == C.LETTERBOX_LEVEL).all()
    pic = lb[:, :, top:Hs - bottom]
    assert (pic != C.LETTERBOX_LEVEL).float().mean() > 0.9                # texture, not bar, between the bars ...
    dx, dy = C.SHIFT
    assert torch.equal(pic[1, :, :-dy, :-dx], pic[0, :, dy:, dx:])       # ... moving (6, 4) px


@pytest.mark.parametrize("size", SIZES)
def test_clipped_saturates_a_fifth_at_each_end(size):
    cl = C.clipped(*size, seed=2)
    for f in cl:
        assert (f == 0).float().mean() >= 0.2 and (f == 255).float().mean() >= 0.2
    dx, dy = C.SHIFT
    assert torch.equal(cl[1, :, :-dy, :-dx], cl[0, :, dy:, dx:])


def test_grain_differs_between_the_frames():
    g = C.grain(H, W, seed=2).double()
    dx, dy = C.SHIFT
    d = g[1, :, :-dy, :-dx] - g[0, :, dy:, dx:]                          # the texture cancels in the overlap: the two frames' noise
    assert 12.0 < float(d.std()) < 16.0                                  # sqrt(2) x 10 levels, a little less where 0 / 255 clip it
    assert abs(float(d.mean())) < 0.5


@pytest.mark.parametrize("size", SIZES + [(2160, 3840)])
def test_pan_is_the_shifted_texture(size):
    Hs, Ws = size
    dx, dy = C.pan_shift(Hs, Ws)
    assert (dx, dy) == (Ws // 12, Hs // 12)
    if size == (2160, 3840):
        assert (dx, dy) == (320, 180)
        return                                                           # the shift only: the 4K pair is built on the GPU box
    p = C.pan(Hs, Ws, seed=2)
    assert torch.equal(p[1, :, :Hs - dy, :Ws - dx], p[0, :, dy:, dx:])
    assert not torch.equal(p[0], p[1])


def test_stripes_are_periodic_full_contrast_and_move_3px():
    s = C.stripes(H, W, seed=2)
    on = (torch.arange(W) % C.STRIPE_PERIOD) < C.STRIPE_ON
    a = s[0].double()
    assert float(a[:, :, on].mean() - a[:, :, ~on].mean()) > 0.75 * 255   # full contrast: the stripes dominate ...
    assert float(a[:, :, on].std()) > 5.0                                 # ... over a texture that is still there
    d = C.STRIPE_SHIFT
    assert torch.equal(s[1, :, :, :-d], s[0, :, :, d:])


def test_object_moves_40px_on_a_flat_background():
    o = C.pair("object", H, W, seed=2)
    y0, x0 = C.object_box(H, W)
    n, d = C.OBJECT_SIZE, C.OBJECT_SHIFT
    assert torch.equal(o[1, :, y0:y0 + n, x0 + d:x0 + d + n], o[0, :, y0:y0 + n, x0:x0 + n])
    for k, x in ((0, x0), (1, x0 + d)):
        bg = torch.ones(H, W, dtype=torch.bool)
        bg[y0:y0 + n, x:x + n] = False
        for c, v in enumerate(C.OBJECT_BG_BGR):
            assert (o[k, c][bg] == v).all()


@pytest.mark.parametrize("case", sorted(C.CASES))
def test_oracle_is_well_defined_on_the_case(oracle, weights, case):
    """The oracle at 192x320, t = 0.5, with the conditioning report: a finite frame, finite features, and a min/max spread > 0 of
    the raw PCA projections at every level (a zero spread would make the rescale divide by zero)."""
    import fldr_harness as Hn
    frames = Hn.frames_from_uint8(C.pair(case, H, W, seed=1))
    pyr = oracle.pad_and_pyramid(frames)
    keep = {}
    with torch.no_grad():
        out = oracle.forward(weights, pyr, torch.tensor([[0.5]]), keep=keep, conditioning=True)[:, :, :H, :W]
    assert out.shape == (1, 3, H, W) and torch.isfinite(out).all()
    spreads = []
    for x in pyr:
        h, w = x.shape[-2:]
        raw = oracle.pca_project_raw(x.reshape(6, h, w), weights["Mean8"], weights["EV8"], weights["meanVec8"])
        spreads.append(float(raw.max() - raw.min()))
    assert all(s > 0 for s in spreads), spreads
    assert all(torch.isfinite(p).all() for p in keep["pca"]) and all(torch.isfinite(f).all() for f in keep["flows"].values())
    fmax = [float(keep["flows"][l].abs().max()) for l in sorted(keep["flows"])]
    print("%s: ill-conditioned feature-splat cells per level (coarse to fine, eps %.0e, +-%.0e px): %s; PCA spread per level %s; "
          "max |flow| per level (fine to coarse, px of that level) %s"
          % (case, oracle.SPLAT_COND_EPS, oracle.SPLAT_COND_DELTA, keep["ill_conditioned_splat_cells"],
             ["%.3g" % s for s in spreads], ["%.1f" % f for f in fmax]))
