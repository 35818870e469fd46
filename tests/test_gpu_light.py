"""The linear-light API (libfldr_light.so through fldr_light) on the GPU.  Every comparison is byte for byte against
tests/light_oracle.py fed the table the library returned: accumulate / resolve / mix, fldr_light_forward on the planar frames read back
from its workspace, and the converter against shutter_oracle.outputs with every output the linear mean of its points."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import light_oracle as LO
import rate_frames as RF
import shutter_oracle as SO
from test_gpu_shutter import _fmt, _host, _pair, _random_frames, _rows_with_gaps, _same, _spliced, _to_dev

pytestmark = pytest.mark.gpu

CURVES = ("gamma24", "pq", "hlg", "table")
_curves = {}


def _caller_table(depth):
    """A table no built-in curve gives: random strictly increasing steps from 3 up to below S."""
    n = 1 << depth
    g = np.random.default_rng(depth)
    return (3 + np.concatenate([[0], np.cumsum(g.integers(1, 2 * (LO.S // n) - 8, n - 1))])).astype(np.uint32)


def _curve(name, depth, dev):
    """(the device curve, the table it holds — what the oracle is fed); one per transfer and depth for the whole module."""
    import fldr_light as L
    key = (name, depth, dev.index or 0)
    if key not in _curves:
        c = L.Curve(table_=_caller_table(depth), depth=depth, device=dev.index or 0) if name == "table" else L.Curve(name, depth, device=dev.index or 0)
        assert int(c.lin[-1]) <= LO.S and (np.diff(c.lin.astype(np.int64)) > 0).all()
        _curves[key] = c
    return _curves[key], _curves[key].lin


def _edges(H, W, layout, depth, seed):
    """Hard edges: blocks of the extreme luma and chroma values the container can hold."""
    import fldr_video
    g = np.random.default_rng(seed)
    dt, top = (np.uint16, 1023) if depth == 10 else (np.uint8, 255)
    sh = 6 if (depth == 10 and layout == "nv12") else 0
    out = []
    for r, c in fldr_video.plane_shapes(layout, H, W):
        coarse = g.integers(0, 2, ((r + 7) // 8, (c + 7) // 8))
        out.append(((np.kron(coarse, np.ones((8, 8), np.int64))[:r, :c] * top) << sh).astype(dt))
    return tuple(out)


def _flat(H, W, layout, depth, luma):
    """A frame whose R'G'B' codes are all 0 (luma 0) or all max (luma max): neutral chroma, limited range clamps the rest."""
    import fldr_video
    dt, top, mid = (np.uint16, 1023, 512) if depth == 10 else (np.uint8, 255, 128)
    sh = 6 if (depth == 10 and layout == "nv12") else 0
    return tuple(np.full(s, ((top if luma else 0) if q == 0 else mid) << sh, dt) for q, s in enumerate(fldr_video.plane_shapes(layout, H, W)))


def _check_all_three(dev, curve, lin, frames, weights, layout, depth, **kw):
    """accumulate + resolve and mix of device copies of `frames` against the oracle; -> the oracle's frame."""
    import fldr_light as L
    fmt = _fmt(layout, depth)
    H, W = frames[0][0].shape
    d = [_to_dev(f, dev, **kw) for f in frames]
    want = LO.mix(frames, weights, lin, layout, depth)
    scratch = torch.empty(L.scratch_bytes(H, W, fmt), dtype=torch.uint8, device=dev)
    acc = L.accumulate(curve, d, weights, fmt, scratch=scratch)
    got = L.resolve(curve, acc, sum(weights), H, W, fmt, scratch=scratch)
    fused = L.mix(curve, d, weights, fmt, scratch=scratch)
    torch.cuda.synchronize()
    assert _same(_host(got), want), "accumulate + resolve"
    assert _same(_host(fused), want), "mix"
    return want


# ---- the kernels ----------------------------------------------------------------------------------------------------------------------------
SIZES = [(2, 2, "gamma24"), (3, 5, "pq"), (17, 31, "gamma24"), (17, 31, "pq"), (17, 31, "hlg"), (17, 31, "table"), (16, 48, "gamma24"),
         (16, 48, "pq"), (16, 48, "hlg"), (16, 48, "table"), (270, 480, "hlg"), (270, 480, "table"), (1079, 1917, "pq")]


@pytest.mark.parametrize("layout,depth", RF.FORMATS)
@pytest.mark.parametrize("H,W,name", SIZES)
def test_kernels_equal_the_oracle(dev, H, W, name, layout, depth):
    """Noise (dirt in the unused bits included), hard edges and noise again, two and three frames: the register mix and the one through
    the accumulator.  (17, 31) and (3, 5) put the pair's second frame off 16 bytes (the per-sample form), (16, 48) and (270, 480) keep it
    aligned (the wide form); all but (16, 48) leave a tail behind the last whole group."""
    curve, lin = _curve(name, depth, dev)
    frames = [_random_frames(1, H, W, layout, depth, seed=H * W)[0], _edges(H, W, layout, depth, 1), _random_frames(1, H, W, layout, depth, seed=7)[0]]
    want = _check_all_three(dev, curve, lin, frames, [1, 250, 4], layout, depth)
    _check_all_three(dev, curve, lin, frames[:2], [3, 2], layout, depth)
    if depth == 10:
        for p in want:                                                  # dirt in, clean words out
            assert not (p & (0x3f if layout == "nv12" else 0xfc00)).any()


@pytest.mark.parametrize("layout,depth,name", [("nv12", 8, "gamma24"), ("nv12", 10, "pq")])
def test_kernels_equal_the_oracle_at_4k(dev, layout, depth, name):
    curve, lin = _curve(name, depth, dev)
    frames = _random_frames(2, 2160, 3840, layout, depth, seed=4)
    _check_all_three(dev, curve, lin, frames, [2, 3], layout, depth)


@pytest.mark.parametrize("layout,depth", RF.FORMATS)
@pytest.mark.parametrize("name", CURVES)
def test_black_and_white_frames_and_the_accumulator_at_its_bound(dev, name, layout, depth):
    """All-max codes under weights totalling 255: every accumulator word is 255 lin[max] (255 S for the built-in curves), the codes come
    back as max; all-0 codes come back as 0; half and half is the oracle's."""
    import fldr_light as L
    H, W = 33, 47
    fmt = _fmt(layout, depth)
    curve, lin = _curve(name, depth, dev)
    mx = (1 << depth) - 1
    black, white = _flat(H, W, layout, depth, 0), _flat(H, W, layout, depth, 1)
    assert (LO.to_codes(black, layout, depth) == 0).all() and (LO.to_codes(white, layout, depth) == mx).all()
    dw, db = _to_dev(white, dev), _to_dev(black, dev)
    acc = L.accumulate(curve, [dw, dw, dw], [100, 100, 55], fmt)
    torch.cuda.synchronize()
    words = acc.cpu().numpy().view(np.uint32)[:3 * H * W]
    assert (words == 255 * int(lin[-1])).all()
    if name != "table":
        assert int(lin[-1]) >= LO.S - 1 and int(words[0]) >= 255 * (LO.S - 1)
    assert _same(_host(L.resolve(curve, acc, 255, H, W, fmt)), LO.mix([white], [1], lin, layout, depth))
    assert _same(_host(L.mix(curve, [db, db], [255 - 7, 7], fmt)), LO.mix([black], [1], lin, layout, depth))
    _check_all_three(dev, curve, lin, [black, white], [128, 127], layout, depth)
    _check_all_three(dev, curve, lin, [black, white, black], [1, 1, 253], layout, depth)


@pytest.mark.parametrize("layout,depth", RF.FORMATS)
@pytest.mark.parametrize("H,W,pad,offset,only", [(64, 96, 32, 0, None), (201, 333, 13, 0, None), (270, 480, 0, 1, 0), (270, 480, 0, 1, 1),
                                                 (270, 480, 0, 1, 2), (201, 333, 48, 1, None)])
def test_kernels_with_pitches_and_misaligned_planes(dev, H, W, pad, offset, only, layout, depth):
    """Pitches wider than the row and plane addresses one sample off — each single plane in turn — on the sources and on the output; the
    output's gap bytes keep their sentinel."""
    import fldr_light as L
    import fldr_video
    if only is not None:
        only = min(only, len(fldr_video.plane_shapes(layout, H, W)) - 1)
    b = 2 if depth == 10 else 1
    pad, offset = pad * b, offset * b
    fmt = _fmt(layout, depth)
    curve, lin = _curve("gamma24", depth, dev)
    frames = _random_frames(3, H, W, layout, depth, seed=7 + H)
    weights = [3, 1, 4]
    want = _check_all_three(dev, curve, lin, frames, weights, layout, depth, pad=pad, offset=offset, only=only, fill=0xA5)
    d = [_to_dev(f, dev) for f in frames]
    dt = fldr_video.plane_dtype(fmt, numpy=True)
    for n in (2, 3):                                                      # the register mix, and accumulate + resolve
        ref = want if n == 3 else LO.mix(frames[:2], weights[:2], lin, layout, depth)
        out = _to_dev([np.zeros(s, dt) for s in fldr_video.plane_shapes(fmt, H, W)], dev, pad=pad + 6 * b, fill=0x5A, offset=offset, only=only)
        if n == 2:
            L.mix(curve, d[:2], weights[:2], fmt, out=out)
        else:
            L.resolve(curve, L.accumulate(curve, d, weights, fmt), sum(weights), H, W, fmt, out=out)
        torch.cuda.synchronize()
        assert _same(_host(out), ref), n
        for q, o in enumerate(out):
            gaps = _rows_with_gaps(o)[:, o.shape[1] * o.element_size():]
            if only is None or only == q:
                assert gaps.numel() and bool((gaps == 0x5A).all()), "a gap byte of an output plane was written"


@pytest.mark.parametrize("layout,depth", RF.FORMATS)
@pytest.mark.parametrize("n", [1, 2, 5, 66, 67, 140])
def test_any_number_of_frames(dev, n, layout, depth):
    """A mix takes 1 .. 66 frames; an accumulate any number, over several launches, while the weights total at most 255."""
    import fldr_light as L
    import fldr_shutter as T
    H, W = 33, 47
    fmt = _fmt(layout, depth)
    curve, lin = _curve("hlg", depth, dev)
    base = _random_frames(min(n, 7), H, W, layout, depth, seed=n)
    frames = [base[k % len(base)] for k in range(n)]
    weights = [1] * n
    weights[0] = 255 - (n - 1) if n <= 66 else 3
    d = [_to_dev(f, dev) for f in base]
    d = [d[k % len(d)] for k in range(n)]
    want = LO.mix(frames, weights, lin, layout, depth)
    got = L.resolve(curve, L.accumulate(curve, d, weights, fmt), sum(weights), H, W, fmt)
    torch.cuda.synchronize()
    assert _same(_host(got), want)
    if n <= T.LAUNCH_FRAMES:
        assert _same(_host(L.mix(curve, d, weights, fmt)), want)
        if n == 1:                                                        # one frame alone: its own R'G'B' codes
            assert _same(want, LO.from_codes(LO.to_codes(frames[0], layout, depth), layout, depth))
    else:
        with pytest.raises(L.LightError) as e:
            L.mix(curve, d, weights, fmt)
        assert e.value.code == L.E_ARG
    # two calls equal one
    if n == 5:
        acc = L.accumulate(curve, d[:2], weights[:2], fmt)
        L.accumulate(curve, d[2:], weights[2:], fmt, acc=acc, first=False)
        assert _same(_host(L.resolve(curve, acc, sum(weights), H, W, fmt)), want)


def test_kernels_are_capturable_and_refused_calls_enqueue_nothing(dev):
    import fldr_light as L
    import fldr_video as V
    H, W = 270, 480
    fmt = _fmt("nv12", 8)
    curve, lin = _curve("gamma24", 8, dev)
    deep_curve, _ = _curve("gamma24", 10, dev)
    frames = _random_frames(3, H, W, "nv12", 8, seed=2)
    d = [_to_dev(f, dev) for f in frames]
    weights = [1, 2, 3]
    acc = torch.full((L.acc_bytes(H, W),), 0x44, dtype=torch.uint8, device=dev)
    scratch = torch.full((L.scratch_bytes(H, W, fmt),), 0x66, dtype=torch.uint8, device=dev)
    out = tuple(p.fill_(0x77) for p in V.empty_frame(fmt, H, W, dev))
    out2 = tuple(p.fill_(0x77) for p in V.empty_frame(fmt, H, W, dev))
    for call, code in ((lambda: L.accumulate(curve, d, [1, 2, 256], fmt, acc=acc, scratch=scratch), L.E_WEIGHT),
                       (lambda: L.accumulate(curve, d, [100, 100, 56], fmt, acc=acc, scratch=scratch), L.E_WEIGHT),
                       (lambda: L.accumulate(curve, d, weights, fmt, acc=acc[64:], scratch=scratch), L.E_ACC),
                       (lambda: L.accumulate(curve, d, weights, fmt, acc=acc, scratch=scratch[16:]), L.E_ACC),
                       (lambda: L.accumulate(deep_curve, d, weights, fmt, acc=acc, scratch=scratch), L.E_CURVE),
                       (lambda: L.resolve(curve, acc, 0, H, W, fmt, out=out, scratch=scratch), L.E_WEIGHT),
                       (lambda: L.resolve(curve, acc, 256, H, W, fmt, out=out, scratch=scratch), L.E_WEIGHT),
                       (lambda: L.resolve(deep_curve, acc, 6, H, W, fmt, out=out, scratch=scratch), L.E_CURVE),
                       (lambda: L.mix(curve, d, [0, 1, 1], fmt, out=out, scratch=scratch), L.E_WEIGHT),
                       (lambda: L.mix(deep_curve, d, weights, fmt, out=out, scratch=scratch), L.E_CURVE)):
        with pytest.raises(L.LightError) as e:
            call()
        assert e.value.code == code
    short = V.frame_struct(out)
    short.pitch[1] = W - 2
    w3 = (ctypes.c_int32 * 3)(1, 2, 3)
    arr = (V.Frame * 3)(*[V.frame_struct(f) for f in d])
    sp = L._stream_ptr(dev, None)
    assert L.lib().fldr_light_mix(H, W, ctypes.byref(fmt), curve._h, arr, w3, 3, ctypes.byref(short), scratch.data_ptr(), sp) == V.E_PITCH
    assert L.lib().fldr_light_resolve(H, W, ctypes.byref(fmt), curve._h, acc.data_ptr(), 6, ctypes.byref(short), scratch.data_ptr(), sp) == V.E_PITCH
    assert L.lib().fldr_light_mix(H, W, ctypes.byref(fmt), None, arr, w3, 3, ctypes.byref(V.frame_struct(out)), scratch.data_ptr(), sp) == L.E_ARG
    torch.cuda.synchronize()
    assert bool((acc == 0x44).all()) and bool((scratch == 0x66).all()) and all(bool((p == 0x77).all()) for p in out)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        L.accumulate(curve, d, weights, fmt, acc=acc, scratch=scratch)    # warm
        L.resolve(curve, acc, 6, H, W, fmt, out=out, scratch=scratch)
        L.mix(curve, d[:2], weights[:2], fmt, out=out2, scratch=scratch)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        L.accumulate(curve, d[:1], weights[:1], fmt, acc=acc, scratch=scratch)
        L.accumulate(curve, d[1:], weights[1:], fmt, acc=acc, first=False, scratch=scratch)
        L.resolve(curve, acc, 6, H, W, fmt, out=out, scratch=scratch)
        L.mix(curve, d[:2], weights[:2], fmt, out=out2, scratch=scratch)
    for rep in range(2):
        d[0][0].copy_(torch.from_numpy(frames[rep + 1][0]).to(dev))      # new samples in a captured plane
        first = (frames[rep + 1][0], frames[0][1])
        acc.fill_(0x99)
        g.replay()
        torch.cuda.synchronize()
        assert _same(_host(out), LO.mix([first, frames[1], frames[2]], weights, lin, "nv12", 8)), rep
        assert _same(_host(out2), LO.mix([first, frames[1]], weights[:2], lin, "nv12", 8)), rep


def test_linear_light_is_brighter_than_the_code_value_mean(dev):
    """Frames that alternate all-black and all-white, full range, BT.709: the 2-point linear mix gives luma 191 (766 at depth 10, the
    oracle's), fldr_shutter_mix gives 128 (512) on the same frames."""
    import fldr_light as L
    import fldr_shutter as T
    H, W = 34, 50
    for layout, depth, lum, code_mean in (("i420", 8, 191, 128), ("nv12", 8, 191, 128), ("nv12", 10, 766, 512), ("i420", 10, 766, 512)):
        fmt = _fmt(layout, depth, "bt709", "full")
        curve, lin = _curve("gamma24", depth, dev)
        black, white = _flat(H, W, layout, depth, 0), _flat(H, W, layout, depth, 1)
        d = [_to_dev(black, dev), _to_dev(white, dev)]
        got = _host(L.mix(curve, d, [1, 1], fmt))
        want = LO.mix([black, white], [1, 1], lin, layout, depth, "bt709", "full")
        assert _same(got, want)
        assert (SO.value(got[0], layout, depth) == lum).all()
        assert (LO.to_codes(got, layout, depth, "bt709", "full") == lum).all()
        flat = _host(T.mix(d, [1, 1], fmt))
        assert (SO.value(flat[0], layout, depth) == code_mean).all()


# ---- fldr_light_forward -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nl(dev):
    import fldr_harness as Hn
    import fldr_light
    import fldr_model
    nm = fldr_model.NativeModel.from_npz(Hn.DEFAULT_WEIGHTS, device=dev.index or 0)
    yield fldr_light.NativeLight(nm)
    nm.close()


@pytest.mark.parametrize("layout,depth", RF.FORMATS)
@pytest.mark.parametrize("w0,w1", [(1, 0), (1, 1), (0, 0), (2, 3)])
def test_forward_is_the_linear_mix_of_the_planar_points(nl, dev, layout, depth, w0, w1):
    import fldr_video
    H, W = 270, 480
    fmt = _fmt(layout, depth)
    curve, lin = _curve("pq" if depth == 10 else "gamma24", depth, dev)
    pair = _pair(H, W, layout, depth)
    frames = [_to_dev(p, dev, pad=6 * (2 if depth == 10 else 1), fill=0x11) for p in pair]
    t = [0.25, 0.5, 0.75]
    w = [1, 2, 1]
    dt = fldr_video.plane_dtype(fmt, numpy=True)
    out = _to_dev([np.zeros(s, dt) for s in fldr_video.plane_shapes(fmt, H, W)], dev, pad=10, fill=0x5A)
    ws = nl.workspace(H, W, 3)
    nl.forward(curve, frames, t, (w0, w1, w), fmt, out=out, ws=ws)
    torch.cuda.synchronize()
    planar_pair, planar_outs = nl.planar(ws, H, W, 3, depth, depth)
    points = [planar_pair[0].cpu().numpy(), planar_pair[1].cpu().numpy()] + [o.cpu().numpy() for o in planar_outs]
    # the points are the converted inputs and the model's planar outputs of fldr_video_forward on the same pair
    for f in range(2):
        assert np.array_equal(points[f], LO.to_codes(pair[f], layout, depth))
    nv = fldr_video.NativeVideo(nl.model)
    ws2 = nv.workspace(H, W, 3)
    nv.forward(frames, t, fmt, fmt, ws=ws2)
    torch.cuda.synchronize()
    for a, b in zip(points[2:], nv.planar(ws2, H, W, 3, depth, depth)[1]):
        assert np.array_equal(a, b.cpu().numpy())
    src = [p for p, wt in zip(points[:2], (w0, w1)) if wt] + points[2:]
    wts = [wt for wt in (w0, w1) if wt] + w
    assert _same(_host(out), LO.mix_codes(src, wts, lin, layout, depth))
    for o in out:
        gaps = _rows_with_gaps(o)[:, o.shape[1] * o.element_size():]
        assert gaps.numel() and bool((gaps == 0x5A).all()), "a gap byte of the output was written"


def test_forward_graph_replay_follows_rewritten_times_and_bad_calls_enqueue_nothing(nl, dev):
    import fldr_light as L
    import fldr_video as V
    H, W = 270, 480
    layout, depth = "nv12", 8
    fmt = _fmt(layout, depth)
    curve, lin = _curve("gamma24", 8, dev)
    deep_curve, _ = _curve("gamma24", 10, dev)
    pair = _pair(H, W, layout, depth)
    frames = [_to_dev(p, dev) for p in pair]
    t = torch.tensor([0.25, 0.75], device=dev)
    ws = nl.workspace(H, W, 2).fill_(0x33)
    out = tuple(p.fill_(0x77) for p in V.empty_frame(fmt, H, W, dev))

    def call(mutate=lambda io: None, ws_=ws, c=curve, w0=1, w1=1, w=(2, 2)):
        io = nl.make_io(frames, t, fmt, fmt, [out], H, W)
        io.n_t = 2
        mutate(io)
        return nl.forward_io(io, c, w0, w1, w, ws_)
    assert call(lambda io: setattr(io.out_format, "layout", 1)) == L.E_FORMAT
    assert call(lambda io: io.out[0].pitch.__setitem__(1, W - 2)) == V.E_PITCH
    assert call(w0=256) == L.E_WEIGHT and call(w=(0, 1)) == L.E_WEIGHT and call(w0=200, w1=52) == L.E_WEIGHT
    assert call(c=None) == L.E_ARG and call(c=deep_curve) == L.E_CURVE
    assert call(ws_=ws[:ws.numel() - 256]) == V.E_WORKSPACE and call(ws_=ws[1:]) == V.E_WORKSPACE
    torch.cuda.synchronize()
    assert bool((ws == 0x33).all()), "a refused call wrote the workspace"
    assert all(bool((p == 0x77).all()) for p in out), "a refused call wrote the output"
    al = lambda v: (v + 255) // 256 * 256
    assert nl.workspace_bytes(H, W, 2) == (al(V.NativeVideo(nl.model).workspace_bytes(H, W, 2)) + L.acc_bytes(H, W)
                                           + L.scratch_bytes(H, W, _fmt(layout, 10)))
    weights = (1, 1, [2, 2])
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        nl.forward(curve, frames, t, weights, fmt, out=out, ws=ws)       # warm
    s.synchronize()
    eager = _host(out)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        nl.forward(curve, frames, t, weights, fmt, out=out, ws=ws)
    for tv in ((0.25, 0.75), (0.5, 0.9)):
        t.copy_(torch.tensor(tv))
        g.replay()
        torch.cuda.synchronize()
        got = _host(out)
        planar_pair, planar_outs = nl.planar(ws, H, W, 2, depth, depth)
        pts = [planar_pair[0].cpu().numpy(), planar_pair[1].cpu().numpy()] + [o.cpu().numpy() for o in planar_outs]
        assert _same(got, LO.mix_codes(pts, [1, 1, 2, 2], lin, layout, depth)), tv
        if tv == (0.25, 0.75):
            assert _same(got, eager)
        else:
            assert not _same(got, eager)


# ---- the converter ---------------------------------------------------------------------------------------------------------------------------
def _run_converter(nl, dev, curve, lin, frames, in_rate, out_rate, shutter, sub, scene, fmt, expect_cuts):
    """Push every frame, then flush; the infos against shutter_oracle.outputs under the cuts the converter measured, every output
    against the oracle's linear mean of its points (the interpolated ones from NativeVideo.forward at the float times of their push),
    a lone input frame against its own bytes; -> (infos, forwards the plan needs)."""
    import fldr_light as L
    import fldr_shutter as T
    import fldr_video
    H, W = frames[0][0].shape
    layout, depth = fmt.name, fmt.bits
    c = L.Converter(nl.model, curve, H, W, fmt, in_rate, out_rate, shutter, sub, scene=scene)
    assert c.max_out == T.max_out(in_rate, out_rate)
    got, infos, cuts = [], [], []
    for n in range(len(frames) + 1):
        outs = c.push(frames[n]) if n < len(frames) else c.flush()
        if n < len(frames) and c.last_scene["cut"]:
            cuts.append(n)
        got.append(outs)
        infos.append(c.last_info)
    assert c.flush() == [] and c.last_info == []
    c.close()
    assert cuts == list(expect_cuts)
    want = LO.outputs(len(frames), in_rate, out_rate, shutter, sub, cuts)
    assert [(i["j"], i["points"], i["truncated"], i["interpolated"]) for p in infos for i in p] == \
        [(o["j"], len(o["points"]), int(o["truncated"]), sum(1 for i, k, src in o["points"] if k and src is None)) for o in want]
    assert [len(p) for p in got] == [sum(1 for o in want if o["push"] == n) for n in range(len(frames) + 1)]
    nv = fldr_video.NativeVideo(nl.model)
    interp, n_forwards = {}, 0
    for n in range(1, len(frames)):                                      # the one forward of push n, at its float times
        ks = sorted(set(k for o in want for i, k, src in o["points"] if k and src is None and i == n - 1))
        if ks:
            pair = [_to_dev(frames[n - 1], dev), _to_dev(frames[n], dev)]
            tt = [float(np.float32(k) / np.float32(sub)) for k in ks]
            for k, o in zip(ks, nv.forward(pair, tt, fmt, fmt)):
                interp[(n - 1, k)] = _host(o)
            torch.cuda.synchronize()
            n_forwards += 1
    flat = [o for p in got for o in p]
    point = lambda i, k, src: frames[i] if k == 0 else frames[src] if src is not None else interp[(i, k)]
    for o, frame in zip(want, flat):
        assert _same(frame, LO.output_frame(o, point, lin, layout, depth)), o["j"]
        # no output mixes two scenes
        used = set()
        for i, k, src in o["points"]:
            used.update([i] if k == 0 else [src] if src is not None else [i, i + 1])
        assert len(set(sum(1 for cc in cuts if cc <= i) for i in used)) == 1, o
    return [i for p in infos for i in p], n_forwards, want, flat


def test_converter_120_to_24_is_the_linear_mean_of_input_frames(nl, dev):
    H, W = 270, 480
    fmt = _fmt("i420", 8)
    curve, lin = _curve("gamma24", 8, dev)
    frames = _spliced(H, W)
    infos, n_forwards, want, outs = _run_converter(nl, dev, curve, lin, frames, 120, 24, 1, 1, True, fmt, expect_cuts=[6])
    assert n_forwards == 0 and all(i["interpolated"] == 0 for i in infos)
    # frames 0 .. 4; 5 alone (6 .. 9 lie behind the cut): its own bytes; 10, 11 (the flush)
    assert [(i["j"], i["points"], i["truncated"]) for i in infos] == [(0, 5, 0), (1, 1, 1), (2, 2, 1)]
    assert want[1]["unchanged"] == 5 and _same(outs[1], frames[5])
    assert not _same(outs[1], LO.mix([frames[5]], [1], lin, "i420", 8)), "the clip cannot tell the frame from its trip through R'G'B'"
    assert not _same(outs[0], SO.mix(frames[:5], [1] * 5, "i420", 8)), "linear light and code values agree on this clip"


def test_converter_60_to_24_with_four_grid_points_per_interval(nl, dev):
    H, W = 270, 480
    fmt = _fmt("i420", 8)
    curve, lin = _curve("gamma24", 8, dev)
    frames = _spliced(H, W)
    infos, n_forwards, _, _ = _run_converter(nl, dev, curve, lin, frames, 60, 24, (1, 2), 4, True, fmt, expect_cuts=[6])
    assert [i["j"] for i in infos] == [0, 1, 2, 3, 4]
    assert infos[0] == {"j": 0, "points": 5, "interpolated": 3, "truncated": 0}
    assert n_forwards >= 4


@pytest.mark.parametrize("layout,depth,name", [("nv12", 10, "pq"), ("i420", 10, "hlg"), ("nv12", 8, "table")])
def test_converter_in_the_other_formats_and_a_flushed_lone_frame(nl, dev, layout, depth, name):
    H, W = 270, 480
    curve, lin = _curve(name, depth, dev)
    frames = _spliced(H, W, layout, depth, 2, 4)                        # 120 -> 24, s = 1/2, sub 2: grid 0 .. 4 and 10 .. 14; (1, 2) is a cut
    infos, _, want, outs = _run_converter(nl, dev, curve, lin, frames, 120, 24, (1, 2), 2, True, _fmt(layout, depth), expect_cuts=[2])
    assert infos[0] == {"j": 0, "points": 3, "interpolated": 1, "truncated": 1}
    # six frames end at grid point 10: the flush returns window 1 with the one point it has, frame 5, unchanged
    assert infos[1] == {"j": 1, "points": 1, "interpolated": 0, "truncated": 1} and len(infos) == 2
    assert want[1]["unchanged"] == 5 and _same(outs[1], frames[5])
