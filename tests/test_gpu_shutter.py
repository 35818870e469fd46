"""The shutter API (libfldr_shutter.so through fldr_shutter) on the GPU.  Every comparison is exact: accumulate / resolve / mix give
the bytes of the numpy statement in tests/shutter_oracle.py, fldr_shutter_forward gives the oracle mix of the input frames and of
fldr_video_forward's frames, and the converter returns what fldr_shutter.schedule() says, each frame the oracle average of its points."""
import functools

import numpy as np
import pytest
import torch

import rate_frames as RF
import shutter_oracle as SO
import yuv_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ns(dev):
    import fldr_harness as Hn
    import fldr_model
    import fldr_shutter
    nm = fldr_model.NativeModel.from_npz(Hn.DEFAULT_WEIGHTS, device=dev.index or 0)
    s = fldr_shutter.NativeShutter(nm)
    yield s
    nm.close()


def _fmt(layout, depth=8, mat="bt709", rng="limited"):
    import fldr_video
    return fldr_video.Format(layout, mat, rng, depth)


def _to_dev(planes, dev, pad=0, fill=0, offset=0, only=None):
    """Device copies of host planes (uint8 or uint16); pad / offset in BYTES: each plane a view into a byte buffer whose rows are `pad`
    bytes longer (gap bytes = fill), starting `offset` bytes into it; only: the one plane pad and offset apply to (None: all)."""
    out = []
    for q, p in enumerate(planes):
        r, c = p.shape
        b = p.dtype.itemsize
        pd, of = (pad, offset) if only is None or only == q else (0, 0)
        pitch = c * b + pd
        buf = torch.full((r * pitch + of + pitch + 256,), fill, dtype=torch.uint8, device=dev)
        view = buf[of:of + r * pitch].view(r, pitch)[:, :c * b]
        view.copy_(torch.from_numpy(np.ascontiguousarray(p).view(np.uint8).reshape(r, c * b)).to(dev))
        out.append(view.view(torch.uint16) if b == 2 else view)
    return tuple(out)


def _host(frame):
    return tuple(p.cpu().numpy() for p in frame)


def _rows_with_gaps(p):
    """The bytes of a plane view with the gap bytes of every row: uint8 [rows, pitch]."""
    b = p.view(torch.uint8) if p.dtype != torch.uint8 else p
    return b.as_strided((b.shape[0], b.stride(0)), b.stride())


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _random_frames(n, H, W, layout, depth, seed, kind="noise"):
    """n host frames of the container.  Depth 10 noise fills all 16 bits of every word: P010's low six and yuv420p10le's high six bits
    are dirt the kernels must ignore."""
    import fldr_video
    g = np.random.default_rng(seed)
    dt = np.uint16 if depth == 10 else np.uint8
    top = 65536 if depth == 10 else 256
    frames = []
    for _ in range(n):
        if kind == "noise":
            frames.append(tuple(g.integers(0, top, s).astype(dt) for s in fldr_video.plane_shapes(layout, H, W)))
        else:                                                           # every sample at the maximum (all bits set)
            frames.append(tuple(np.full(s, top - 1, dt) for s in fldr_video.plane_shapes(layout, H, W)))
    return frames


def _check_all_three(dev, frames, weights, layout, depth, **kw):
    """accumulate + resolve and mix of device copies of `frames` against the oracle; -> the oracle's frame."""
    import fldr_shutter as T
    fmt = _fmt(layout, depth)
    H, W = frames[0][0].shape
    d = [_to_dev(f, dev, **kw) for f in frames]
    want = SO.mix(frames, weights, layout, depth)
    acc = T.accumulate(d, weights, fmt)
    got = T.resolve(acc, sum(weights), H, W, fmt)
    fused = T.mix(d, weights, fmt)
    torch.cuda.synchronize()
    assert _same(_host(got), want), "accumulate + resolve"
    assert _same(_host(fused), want), "mix"
    return want


# ---- the kernels ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,depth", RF.FORMATS)
@pytest.mark.parametrize("H,W", [(2, 2), (3, 5), (17, 31), (16, 48), (270, 480), (1079, 1917), (1080, 1920)])
def test_kernels_equal_the_oracle_at_every_size(dev, H, W, layout, depth):
    frames = _random_frames(3, H, W, layout, depth, seed=H * W)
    want = _check_all_three(dev, frames, [1, 255, 7], layout, depth)
    if depth == 10:
        for p in want:                                                  # dirt in, clean words out
            assert not (p & (0x3f if layout == "nv12" else 0xfc00)).any()


@pytest.mark.parametrize("layout,depth", [("nv12", 8), ("nv12", 10)])
def test_kernels_equal_the_oracle_at_4k(dev, layout, depth):
    frames = _random_frames(5, 2160, 3840, layout, depth, seed=4)
    _check_all_three(dev, frames, [1, 2, 3, 4, 5], layout, depth)


@pytest.mark.parametrize("layout,depth", RF.FORMATS)
@pytest.mark.parametrize("H,W,pad,offset,only", [(64, 96, 32, 0, None), (201, 333, 13, 0, None), (270, 480, 0, 1, 0), (270, 480, 0, 1, 1),
                                                 (270, 480, 0, 1, 2), (201, 333, 48, 1, None), (1080, 1920, 256, 4096, None)])
def test_kernels_with_pitches_and_misaligned_planes(dev, H, W, pad, offset, only, layout, depth):
    """Pitches wider than the row, and plane addresses one sample off a 16-byte boundary — each single plane in turn — where the
    per-sample form runs; the output's gap bytes keep their sentinel in both forms."""
    import fldr_shutter as T
    import fldr_video
    if only is not None:
        only = min(only, len(fldr_video.plane_shapes(layout, H, W)) - 1)      # NV12 has two planes
    b = 2 if depth == 10 else 1
    pad, offset = pad * b, offset * b                                     # depth 10: even pitches and addresses
    fmt = _fmt(layout, depth)
    frames = _random_frames(4, H, W, layout, depth, seed=7 + H)
    weights = [3, 1, 4, 1]
    want = _check_all_three(dev, frames, weights, layout, depth, pad=pad, offset=offset, only=only, fill=0xA5)
    # sources aligned, the output padded / misaligned: resolve and mix write nothing but the rows
    d = [_to_dev(f, dev) for f in frames]
    dt = fldr_video.plane_dtype(fmt, numpy=True)
    for use_mix in (False, True):
        out = _to_dev([np.zeros(s, dt) for s in fldr_video.plane_shapes(fmt, H, W)], dev, pad=pad + 6 * b, fill=0x5A, offset=offset, only=only)
        if use_mix:
            T.mix(d, weights, fmt, out=out)
        else:
            T.resolve(T.accumulate(d, weights, fmt), sum(weights), H, W, fmt, out=out)
        torch.cuda.synchronize()
        assert _same(_host(out), want), use_mix
        for q, o in enumerate(out):
            gaps = _rows_with_gaps(o)[:, o.shape[1] * o.element_size():]
            if only is None or only == q:
                assert gaps.numel() and bool((gaps == 0x5A).all()), "a gap byte of an output plane was written"


@pytest.mark.parametrize("layout,depth", RF.FORMATS)
@pytest.mark.parametrize("n", [1, 2, 4, 5, 8, 9, 66, 67, 140])
def test_any_number_of_frames(dev, n, layout, depth):
    """n from one frame to more than two launches hold; a mix takes what one launch takes."""
    import fldr_shutter as T
    H, W = 33, 47
    fmt = _fmt(layout, depth)
    frames = _random_frames(min(n, 9), H, W, layout, depth, seed=n)
    frames = [frames[k % len(frames)] for k in range(n)]
    g = np.random.default_rng(n)
    weights = [int(v) for v in g.integers(1, 256, n)]
    weights[0] = 255
    d = [_to_dev(f, dev) for f in frames[:9]]
    d = [d[k % len(d)] for k in range(n)]
    want = SO.mix(frames, weights, layout, depth)
    got = T.resolve(T.accumulate(d, weights, fmt), sum(weights), H, W, fmt)
    torch.cuda.synchronize()
    assert _same(_host(got), want)
    if n <= T.LAUNCH_FRAMES:
        assert _same(_host(T.mix(d, weights, fmt)), want)
    else:
        with pytest.raises(T.ShutterError) as e:
            T.mix(d, weights, fmt)
        assert e.value.code == T.E_ARG


@pytest.mark.parametrize("layout,depth", RF.FORMATS)
def test_the_accumulator_at_its_bound(dev, layout, depth):
    """All-maximum samples under weights totalling 65535 (257 frames of weight 255, in one call): acc = max * 65535 exactly, the
    quotient is the maximum; and the largest total with noise."""
    import fldr_shutter as T
    H, W = 33, 47
    fmt = _fmt(layout, depth)
    mx = 1023 if depth == 10 else 255
    top = _random_frames(1, H, W, layout, depth, 0, kind="max")[0]
    d = _to_dev(top, dev)
    acc = T.accumulate([d] * 257, [255] * 257, fmt)
    torch.cuda.synchronize()
    words = acc.cpu().numpy().view(np.uint32)
    samples = sum(p.size for p in top)
    assert (words[:samples] == mx * 65535).all()
    got = _host(T.resolve(acc, 65535, H, W, fmt))
    assert _same(got, SO.mix([top], [1], layout, depth))
    assert all((SO.value(p, layout, depth) == mx).all() for p in got)
    noise = _random_frames(3, H, W, layout, depth, 1)
    dn = [_to_dev(f, dev) for f in noise]
    frames, weights = [noise[k % 3] for k in range(257)], [255] * 257
    acc = T.accumulate([dn[k % 3] for k in range(257)], weights, fmt)
    assert _same(_host(T.resolve(acc, 65535, H, W, fmt)), SO.mix(frames, weights, layout, depth))


@pytest.mark.parametrize("layout,depth", RF.FORMATS)
def test_accumulator_behaviour(dev, layout, depth):
    import fldr_shutter as T
    H, W = 201, 333
    fmt = _fmt(layout, depth)
    frames = _random_frames(6, H, W, layout, depth, seed=11)
    weights = [5, 1, 9, 2, 255, 3]
    d = [_to_dev(f, dev) for f in frames]
    want = SO.mix(frames, weights, layout, depth)
    # first = 1 ignores what the accumulator held
    stale = torch.full((T.acc_bytes(H, W, fmt),), 0xEE, dtype=torch.uint8, device=dev)
    one = T.accumulate(d, weights, fmt, acc=stale, first=True)
    assert _same(_host(T.resolve(one, sum(weights), H, W, fmt)), want)
    # two calls equal one: the same accumulator words, the same frame
    two = T.accumulate(d[:2], weights[:2], fmt)
    T.accumulate(d[2:], weights[2:], fmt, acc=two, first=False)
    torch.cuda.synchronize()
    used = 4 * sum(p.size for p in frames[0])                         # behind it: the rounding to 256, never written
    assert torch.equal(one[:used], two[:used]) and bool((one[used:] == 0xEE).all())
    assert _same(_host(T.resolve(two, sum(weights), H, W, fmt)), want)
    # a single frame at weight 1 (or any weight) comes back as its own values
    for w in (1, 255):
        back = _host(T.mix([d[0]], [w], fmt))
        for p, q in zip(back, frames[0]):
            assert np.array_equal(SO.value(p, layout, depth), SO.value(q, layout, depth))
    # the output may be one of the sources
    T.mix(d, weights, fmt, out=d[3])
    assert _same(_host(d[3]), want)


def test_kernels_are_capturable_and_refused_calls_enqueue_nothing(dev):
    import fldr_shutter as T
    import fldr_video as V
    H, W = 270, 480
    fmt = _fmt("nv12", 8)
    frames = _random_frames(3, H, W, "nv12", 8, seed=2)
    d = [_to_dev(f, dev) for f in frames]
    weights = [1, 2, 3]
    acc = torch.full((T.acc_bytes(H, W, fmt),), 0x44, dtype=torch.uint8, device=dev)
    out = tuple(p.fill_(0x77) for p in V.empty_frame(fmt, H, W, dev))
    with pytest.raises(T.ShutterError) as e:
        T.accumulate(d, [1, 2, 256], fmt, acc=acc)
    assert e.value.code == T.E_WEIGHT
    with pytest.raises(T.ShutterError) as e:
        T.accumulate(d, weights, fmt, acc=acc[64:])
    assert e.value.code == T.E_ACC
    with pytest.raises(T.ShutterError) as e:
        T.resolve(acc, 0, H, W, fmt, out=out)
    assert e.value.code == T.E_WEIGHT
    with pytest.raises(T.ShutterError) as e:
        T.mix(d, [0, 1, 1], fmt, out=out)
    assert e.value.code == T.E_WEIGHT
    short = V.frame_struct(out)
    short.pitch[1] = W - 2
    w3 = (T.ctypes.c_int32 * 3)(1, 2, 3)
    arr = (V.Frame * 3)(*[V.frame_struct(f) for f in d])
    assert T.lib().fldr_shutter_mix(H, W, T.ctypes.byref(fmt), arr, w3, 3, T.ctypes.byref(short), T._stream_ptr(dev, None)) == V.E_PITCH
    assert T.lib().fldr_shutter_resolve(H, W, T.ctypes.byref(fmt), acc.data_ptr(), 6, T.ctypes.byref(short), T._stream_ptr(dev, None)) == V.E_PITCH
    torch.cuda.synchronize()
    assert bool((acc == 0x44).all()) and all(bool((p == 0x77).all()) for p in out)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        T.accumulate(d, weights, fmt, acc=acc)                           # warm
        T.resolve(acc, 6, H, W, fmt, out=out)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        T.accumulate(d[:1], weights[:1], fmt, acc=acc)
        T.accumulate(d[1:], weights[1:], fmt, acc=acc, first=False)
        T.resolve(acc, 6, H, W, fmt, out=out)
    for rep in range(2):
        d[0][0].copy_(torch.from_numpy(frames[rep + 1][0]).to(dev))      # new samples in a captured plane
        want = SO.mix([(frames[rep + 1][0], frames[0][1]), frames[1], frames[2]], weights, "nv12", 8)
        acc.fill_(0x99)
        g.replay()
        torch.cuda.synchronize()
        assert _same(_host(out), want), rep


# ---- fldr_shutter_forward -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _pair(H, W, layout, depth):
    import fldr_harness as Hn
    u8 = Hn.synthetic_pair(H, W, seed=3).numpy()
    return tuple(RF.planes_of_bgr(u8[i], layout, depth) for i in range(2))


@pytest.mark.parametrize("layout,depth", RF.FORMATS)
@pytest.mark.parametrize("w0,w1", [(1, 0), (1, 1), (0, 0), (2, 3)])
def test_forward_is_the_mix_of_the_inputs_and_the_video_forward(ns, dev, layout, depth, w0, w1):
    import fldr_video
    H, W = 255, 447
    fmt = _fmt(layout, depth)
    pair = _pair(H, W, layout, depth)
    frames = [_to_dev(p, dev, pad=6 * (2 if depth == 10 else 1), fill=0x11) for p in pair]
    t = [0.25, 0.5, 0.75]
    w = [1, 2, 1]
    dt = fldr_video.plane_dtype(fmt, numpy=True)
    out = _to_dev([np.zeros(s, dt) for s in fldr_video.plane_shapes(fmt, H, W)], dev, pad=10, fill=0x5A)
    ns.forward(frames, t, (w0, w1, w), fmt, out=out)
    torch.cuda.synchronize()
    subs = [_host(o) for o in fldr_video.NativeVideo(ns.model).forward(frames, t, fmt, fmt)]
    torch.cuda.synchronize()
    src = [f for f, wt in zip(pair, (w0, w1)) if wt] + subs
    wts = [wt for wt in (w0, w1) if wt] + w
    assert _same(_host(out), SO.mix(src, wts, layout, depth))
    for o in out:
        gaps = _rows_with_gaps(o)[:, o.shape[1] * o.element_size():]
        assert gaps.numel() and bool((gaps == 0x5A).all()), "a gap byte of the output was written"


def test_forward_graph_replay_follows_rewritten_times(ns, dev):
    import fldr_video
    H, W = 256, 448
    layout, depth = "nv12", 8
    fmt = _fmt(layout, depth)
    pair = _pair(H, W, layout, depth)
    frames = [_to_dev(p, dev) for p in pair]
    t = torch.tensor([0.25, 0.75], device=dev)
    ws = ns.workspace(H, W, 2)
    out = fldr_video.empty_frame(fmt, H, W, dev)
    weights = (1, 1, [2, 2])
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ns.forward(frames, t, weights, fmt, out=out, ws=ws)              # warm
    s.synchronize()
    eager = _host(out)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ns.forward(frames, t, weights, fmt, out=out, ws=ws)
    nv = fldr_video.NativeVideo(ns.model)
    for tv in ((0.25, 0.75), (0.5, 0.9)):
        t.copy_(torch.tensor(tv))
        g.replay()
        torch.cuda.synchronize()
        got = _host(out)
        subs = [_host(o) for o in nv.forward(frames, list(tv), fmt, fmt)]
        torch.cuda.synchronize()
        assert _same(got, SO.mix(list(pair) + subs, [1, 1, 2, 2], layout, depth)), tv
        if tv == (0.25, 0.75):
            assert _same(got, eager)


def test_bad_forward_calls_enqueue_nothing(ns, dev):
    import fldr_shutter as T
    import fldr_video as V
    H, W = 256, 256
    fmt = _fmt("nv12", 8)
    pair = _pair(H, W, "nv12", 8)
    frames = [_to_dev(p, dev) for p in pair]
    t = torch.tensor([0.5], device=dev)
    ws = ns.workspace(H, W).fill_(0x33)
    out = tuple(p.fill_(0x77) for p in V.empty_frame(fmt, H, W, dev))

    def call(mutate=lambda io: None, ws_=ws, w0=1, w1=1, w=(1,)):
        io = ns.make_io(frames, t, fmt, fmt, [out], H, W)
        mutate(io)
        return ns.forward_io(io, w0, w1, w, ws_)
    assert call(lambda io: setattr(io.out_format, "layout", 1)) == T.E_FORMAT
    assert call(lambda io: io.out[0].pitch.__setitem__(1, W - 2)) == V.E_PITCH
    assert call(w0=256) == T.E_WEIGHT and call(w=(0,)) == T.E_WEIGHT
    assert call(ws_=ws[:ws.numel() - 256]) == V.E_WORKSPACE              # room for the video forward, not for the sub-frame
    assert call(ws_=ws[1:]) == V.E_WORKSPACE
    torch.cuda.synchronize()
    assert bool((ws == 0x33).all()), "a refused call wrote the workspace"
    assert all(bool((p == 0x77).all()) for p in out), "a refused call wrote the output"
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((out[0] == 0x77).all())
    al = lambda v: (v + 255) // 256 * 256
    assert ns.workspace_bytes(H, W, 3) == al(V.NativeVideo(ns.model).workspace_bytes(H, W, 3)) + 3 * al(2 * (H * W + H * W // 2))


# ---- the converter ---------------------------------------------------------------------------------------------------------------------------
def _clip(H, W, n, seed):
    """n frames of a texture moving 4 px down and 6 px right per frame (BGR planar numpy)."""
    import fldr_harness as Hn
    base = Hn.synthetic_pair(H + 4 * n, W + 6 * n, seed=seed).numpy()[0]
    return [np.ascontiguousarray(base[:, 4 * k:4 * k + H, 6 * k:6 * k + W]) for k in range(n)]


@functools.lru_cache(maxsize=8)
def _spliced(H, W, layout="i420", depth=8, n_a=6, n_b=6):
    """n_a frames of one moving texture, then n_b of another, darker one — a cut at frame n_a."""
    a, b = _clip(H, W, n_a, seed=5), _clip(H, W, n_b, seed=11)
    b = [(f.astype(np.float64) * 0.35).round().astype(np.uint8) for f in b]
    if (layout, depth) == ("i420", 8):
        return [O.bgr_to_yuv420(f, "bt709", "limited") for f in a + b]
    return [RF.planes_of_bgr(f, layout, depth) for f in a + b]


def _run_converter(ns, dev, frames, in_rate, out_rate, shutter, sub, scene, fmt, expect_cuts):
    """Push every frame, then flush; every output against schedule() under the cuts the converter measured and the oracle average of
    its points, the interpolated ones from NativeVideo.forward at the float times of the push; -> (converter, infos, forwards run)."""
    import fldr_shutter as T
    import fldr_video
    H, W = frames[0][0].shape
    layout, depth = fmt.name, fmt.bits
    c = T.Converter(ns.model, H, W, fmt, in_rate, out_rate, shutter, sub, scene=scene)
    assert c.max_out == T.max_out(in_rate, out_rate)
    got, infos, cuts = [], [], []
    for n in range(len(frames) + 1):
        outs = c.push(frames[n]) if n < len(frames) else c.flush()
        if n < len(frames) and c.last_scene["cut"]:
            cuts.append(n)
        if n == 0 or not scene:
            assert n == len(frames) or c.last_scene == {"sad": 0, "hist_dist": 0, "cut": 0}
        got.append(outs)
        infos.append(c.last_info)
    assert c.flush() == [] and c.last_info == []                          # a second flush returns nothing
    assert cuts == list(expect_cuts)
    sched = T.schedule(len(frames), in_rate, out_rate, shutter, sub, cuts)
    assert [o for p in sched for o in p] == [{k: o[k] for k in ("j", "points", "truncated")}
                                             for o in SO.outputs(len(frames), in_rate, out_rate, shutter, sub, cuts)]
    nv = fldr_video.NativeVideo(ns.model)
    every = [o for p in sched for o in p]
    n_forwards = 0
    for n, (outs, want) in enumerate(zip(got, sched)):
        assert [i["j"] for i in infos[n]] == [o["j"] for o in want], (n, infos[n], want)
        # the one forward of this push serves every window it touches, those a later push returns included
        ks = sorted(set(k for o in every for i, k, src in o["points"] if k and src is None and i == n - 1))
        sub_frames = {}
        if ks:                                                           # the one forward of this push, at its float times
            pair = [_to_dev(frames[n - 1], dev), _to_dev(frames[n], dev)]
            tt = [float(np.float32(k) / np.float32(sub)) for k in ks]
            for k, o in zip(ks, nv.forward(pair, tt, fmt, fmt)):
                sub_frames[k] = _host(o)
            torch.cuda.synchronize()
            n_forwards += 1
        for o in every:                                                  # remembered on the output until a push returns it
            for i, k, src in o["points"]:
                if k and src is None and i == n - 1:
                    o.setdefault("interp", {})[(i, k)] = sub_frames[k]
        for q, o in enumerate(want):
            src_frames = [frames[i] if k == 0 else frames[src] if src is not None else o["interp"][(i, k)] for i, k, src in o["points"]]
            ref = SO.mix(src_frames, [1] * len(src_frames), layout, depth)
            assert _same(outs[q], ref), (n, o["j"])
            info = infos[n][q]
            assert info["points"] == len(o["points"]) and info["truncated"] == int(o["truncated"])
            assert info["interpolated"] == sum(1 for i, k, src in o["points"] if k and src is None)
    return c, [i for p in infos for i in p], n_forwards


def test_converter_120_to_24_averages_input_frames_and_never_mixes_scenes(ns, dev):
    H, W = 256, 448
    fmt = _fmt("i420", 8)
    frames = _spliced(H, W)
    c, infos, n_forwards = _run_converter(ns, dev, frames, 120, 24, 1, 1, True, fmt, expect_cuts=[6])
    assert n_forwards == 0 and all(i["interpolated"] == 0 for i in infos)
    # frames 0 .. 4; 5 alone (6 .. 9 lie behind the cut); 10, 11 (the flush)
    assert [(i["j"], i["points"], i["truncated"]) for i in infos] == [(0, 5, 0), (1, 1, 1), (2, 2, 1)]
    # reset: a new stream from frame 0
    c.reset()
    for n in range(4):
        assert c.push(frames[n]) == []
    out = c.push(frames[4])
    assert len(out) == 1 and _same(out[0], SO.mix(frames[:5], [1] * 5, "i420", 8))
    assert c.flush() == []
    c.close()
    # the detector off: output 1 mixes the two scenes
    c, infos, _ = _run_converter(ns, dev, frames, 120, 24, 1, 1, False, fmt, expect_cuts=[])
    assert [(i["j"], i["points"], i["truncated"]) for i in infos] == [(0, 5, 0), (1, 5, 0), (2, 2, 1)]
    c.close()


def test_converter_60_to_24_with_four_grid_points_per_interval(ns, dev):
    H, W = 256, 448
    fmt = _fmt("i420", 8)
    frames = _spliced(H, W)
    c, infos, n_forwards = _run_converter(ns, dev, frames, 60, 24, (1, 2), 4, True, fmt, expect_cuts=[6])
    assert [i["j"] for i in infos] == [0, 1, 2, 3, 4]
    assert infos[0] == {"j": 0, "points": 5, "interpolated": 3, "truncated": 0}
    assert n_forwards >= 4
    c.close()
    c, infos, _ = _run_converter(ns, dev, frames, 60, 24, (1, 2), 4, False, fmt, expect_cuts=[])
    assert all(i["points"] == 5 for i in infos[:-1])
    c.close()


def test_converter_up_conversion_24_to_60(ns, dev):
    H, W = 256, 448
    fmt = _fmt("i420", 8)
    frames = _spliced(H, W)[:5]
    c, infos, n_forwards = _run_converter(ns, dev, frames, 24, 60, 1, 8, True, fmt, expect_cuts=[])
    assert len(infos) == 11 and n_forwards == 4
    c.close()


@pytest.mark.parametrize("layout,depth", [("nv12", 8), ("nv12", 10), ("i420", 10)])
def test_converter_in_the_other_formats(ns, dev, layout, depth):
    H, W = 256, 448
    frames = _spliced(H, W, layout, depth, 2, 6)                        # grid 0 .. 4 and 10 .. 14; the pair (1, 2) is a cut
    c, infos, _ = _run_converter(ns, dev, frames, 120, 24, (1, 2), 2, True, _fmt(layout, depth), expect_cuts=[2])
    assert infos[0] == {"j": 0, "points": 3, "interpolated": 1, "truncated": 1}
    assert infos[1] == {"j": 1, "points": 5, "interpolated": 2, "truncated": 0} and len(infos) == 2
    c.close()
