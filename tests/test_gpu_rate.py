"""The rate API (libfldr_rate.so through fldr_rate) on the GPU.  Every comparison is exact: fldr_scene_measure gives the fields of
tests/scene_oracle.py, fldr_rate_forward gives fldr_video_forward's bytes on a pair that is no cut and copies of the input frames on
one that is, and the converter returns what fldr_rate.schedule() says, each frame the pushed bytes or the forward of its pair."""
import functools

import numpy as np
import pytest
import torch

import rate_frames as RF
import scene_oracle as S
import yuv_oracle as O

pytestmark = pytest.mark.gpu

import content_pairs as CP  # noqa: E402


@pytest.fixture(scope="module")
def nr(dev):
    import fldr_harness as Hn
    import fldr_model
    import fldr_rate
    nm = fldr_model.NativeModel.from_npz(Hn.DEFAULT_WEIGHTS, device=dev.index or 0)
    r = fldr_rate.NativeRate(nm)
    yield r
    nm.close()


def _fmt(layout, depth=8, mat="bt709", rng="limited"):
    import fldr_video
    return fldr_video.Format(layout, mat, rng, depth)


def _to_dev(planes, dev, pad=0, fill=0, offset=0):
    """Device copies of host planes (uint8 or uint16); pad / offset in BYTES: each plane a view into a byte buffer whose rows are `pad`
    bytes longer (gap bytes = fill), starting `offset` bytes into it."""
    out = []
    for p in planes:
        r, c = p.shape
        b = p.dtype.itemsize
        pitch = c * b + pad
        buf = torch.full((r * pitch + offset + pitch + 256,), fill, dtype=torch.uint8, device=dev)
        view = buf[offset:offset + r * pitch].view(r, pitch)[:, :c * b]
        view.copy_(torch.from_numpy(np.ascontiguousarray(p).view(np.uint8).reshape(r, c * b)).to(dev))
        out.append(view.view(torch.uint16) if b == 2 else view)
    return tuple(out)


def _host(frame):
    return tuple(p.cpu().numpy() for p in frame)


def _rows_with_gaps(p):
    """The bytes of a plane view with the gap bytes of every row: uint8 [rows, pitch]."""
    b = p.view(torch.uint8) if p.dtype != torch.uint8 else p
    return b.as_strided((b.shape[0], b.stride(0)), b.stride())


def _luma_frames(H, W, layout, depth, seed, kind="mixed", dirt=False):
    """Two frames of the container with a luma plane made for the measure: noise, flat runs and a flat band, so that every form of the
    histogram's combining runs; chroma is noise (never read)."""
    g = np.random.default_rng(seed)
    mx = 1023 if depth == 10 else 255
    frames = []
    for f in range(2):
        if kind == "mixed":
            y = g.integers(0, mx + 1, (H, W))
            y[:, W // 3:W // 2] = np.repeat(g.integers(0, mx + 1, (H, 1)), W // 2 - W // 3, 1)       # flat runs, another value per row
            y[H // 4:H // 2] = 16 + f                                                               # a flat band, 16 -> 17
            y[H // 2:3 * H // 4] = y[H // 2:3 * H // 4] if f == 0 else frames[0][0][H // 2:3 * H // 4]   # a band equal in both frames
        else:
            y = np.full((H, W), kind[f])
        ch, cw = (H + 1) // 2, (W + 1) // 2
        u, v = g.integers(0, mx + 1, (ch, cw)), g.integers(0, mx + 1, (ch, cw))
        frames.append((y, u, v))
    import yuv_hd_oracle as HD
    dt = np.uint16 if depth == 10 else np.uint8
    d = np.random.default_rng(seed + 1) if dirt else None
    return [HD.pack_planes(*(a.astype(dt) for a in fr), layout, depth, dirt=d) for fr in frames]


def _measure_and_check(dev, planes, fmt, params=None, **kw):
    import fldr_rate as R
    frames = [_to_dev(p, dev, **kw) for p in planes]
    got = R.scene_measure(frames, fmt, params)
    want = S.measure(planes[0], planes[1], fmt, params)
    assert got == want, (got, want)
    return got


# ---- fldr_scene_measure -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,depth", RF.FORMATS)
@pytest.mark.parametrize("case", list(CP.CASES))
def test_measure_equals_the_oracle_on_every_content_case(dev, case, layout, depth):
    H, W = 270, 480
    planes = RF.content(case, H, W, 0, layout, depth)
    got = _measure_and_check(dev, planes, _fmt(layout, depth))
    assert got["cut"] == (1 if case in RF.CUT_CASES else 0)


@pytest.mark.parametrize("layout,depth", RF.FORMATS)
@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (3, 5), (17, 31), (1080, 1920), (2160, 3840), (2159, 3837)])
def test_measure_equals_the_oracle_at_every_size(dev, H, W, layout, depth):
    planes = _luma_frames(H, W, layout, depth, seed=H * W)
    _measure_and_check(dev, planes, _fmt(layout, depth))
    _measure_and_check(dev, planes, _fmt(layout, depth), params=(1, 1))
    _measure_and_check(dev, planes, _fmt(layout, depth), params=(1000, 1000))


@pytest.mark.parametrize("layout,depth", RF.FORMATS)
@pytest.mark.parametrize("H,W,pad,offset", [(64, 96, 32, 0), (201, 333, 13, 0), (201, 333, 0, 1), (270, 480, 48, 1), (1080, 1920, 256, 4096)])
def test_measure_with_pitches_and_offset_planes(dev, H, W, pad, offset, layout, depth):
    """Pitches wider than the row (gap bytes of either fill change nothing) and plane addresses one sample off a 16-byte boundary, where
    the per-sample form of the kernel runs."""
    b = 2 if depth == 10 else 1
    pad, offset = pad * b, offset * b                                     # depth 10: even pitches and addresses
    planes = _luma_frames(H, W, layout, depth, seed=7 + H)
    a = _measure_and_check(dev, planes, _fmt(layout, depth), pad=pad, offset=offset, fill=0xA5)
    c = _measure_and_check(dev, planes, _fmt(layout, depth), pad=pad, offset=offset, fill=0x00)
    assert a == c


@pytest.mark.parametrize("layout,depth", RF.FORMATS)
def test_measure_extremes_and_ignored_bits(dev, layout, depth):
    H, W = 1080, 1920
    mx = 1023 if depth == 10 else 255
    fmt = _fmt(layout, depth)
    got = _measure_and_check(dev, _luma_frames(H, W, layout, depth, 1, kind=(0, mx)), fmt)
    assert got == {"sad": 255 * H * W, "hist_dist": 2 * H * W, "cut": 1}      # black against white: both maxima
    planes = _luma_frames(H, W, layout, depth, 2)
    got = _measure_and_check(dev, [planes[0], planes[0]], fmt)
    assert got == {"sad": 0, "hist_dist": 0, "cut": 0}                        # identical frames
    if depth == 10:
        # P010 words with noise in the low six bits, yuv420p10le words with noise above bit 9: the same measure as the clean words
        clean = _luma_frames(H, W, layout, depth, 3)
        dirty = _luma_frames(H, W, layout, depth, 3, dirt=True)
        assert not np.array_equal(clean[0][0], dirty[0][0])
        assert _measure_and_check(dev, dirty, fmt) == _measure_and_check(dev, clean, fmt)


def test_measure_is_repeatable_capturable_and_needs_no_prepared_state(dev):
    import fldr_rate as R
    H, W = 1080, 1920
    fmt = _fmt("nv12", 8)
    planes = RF.content("cut", H, W, 0, "nv12", 8)
    frames = [_to_dev(p, dev) for p in planes]
    want = S.measure(planes[0], planes[1], fmt)
    states = []
    for fill in (0x00, 0xFF, 0x5A):                                        # garbage left in the state beforehand changes nothing
        st = R.scene_state(dev).fill_(fill)
        R.scene_measure(frames, fmt, state=st, read=False)
        torch.cuda.synchronize()
        states.append(st.cpu().numpy().copy())
    st = R.scene_state(dev).fill_(0x33)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        R.scene_measure(frames, fmt, state=st, read=False)                 # warm
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        R.scene_measure(frames, fmt, state=st, read=False)
    for _ in range(2):
        st.fill_(0x77)
        g.replay()
        torch.cuda.synchronize()
        states.append(st.cpu().numpy().copy())
    for b in states[1:]:
        assert np.array_equal(b, states[0])                                # all FLDR_SCENE_STATE_BYTES, not only the result
    assert R.read_result(torch.from_numpy(states[0])) == want
    assert not states[0][16:64].any()                                      # reserved words and the bytes behind the result: zero


def test_two_measures_in_flight_on_two_streams(dev):
    import fldr_rate as R
    H, W = 2160, 3840
    fmt = _fmt("i420", 8)
    pairs = [_luma_frames(H, W, "i420", 8, seed=20 + k) for k in range(2)]
    frames = [[_to_dev(p, dev) for p in pr] for pr in pairs]
    want = [S.measure(pr[0], pr[1], fmt) for pr in pairs]
    assert want[0] != want[1]
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    states = [R.scene_state(dev) for _ in range(2)]
    torch.cuda.synchronize()
    for rep in range(4):
        for k in range(2):
            with torch.cuda.stream(streams[k]):
                R.scene_measure(frames[k], fmt, state=states[k], read=False)
    torch.cuda.synchronize()
    for k in range(2):
        assert R.read_result(states[k]) == want[k], k


def test_bad_measure_calls_enqueue_nothing(dev):
    import fldr_rate as R
    import fldr_video as V
    H, W = 64, 96
    fmt = _fmt("nv12", 8)
    frames = [_to_dev(p, dev) for p in _luma_frames(H, W, "nv12", 8, 0)]
    st = R.scene_state(dev).fill_(0x44)
    fs = [V.frame_struct(f) for f in frames]
    sp = R._stream_ptr(dev, None)
    assert R.scene_measure_raw(H, W, fmt, fs, R.SceneParams(2000, 0), st.data_ptr(), sp) == R.E_ARG
    assert R.scene_measure_raw(H, W, fmt, fs, None, st.data_ptr() + 64, sp) == R.E_STATE
    fs[1].pitch[0] = W - 1
    assert R.scene_measure_raw(H, W, fmt, fs, None, st.data_ptr(), sp) == V.E_PITCH
    torch.cuda.synchronize()
    assert bool((st == 0x44).all())


# ---- fldr_rate_forward ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _pairs(H, W, layout, depth):
    """(a pair that is no cut, a pair that is one), by the oracle under the default thresholds."""
    import fldr_harness as Hn
    u8 = Hn.synthetic_pair(H, W, seed=3).numpy()
    calm = tuple(RF.planes_of_bgr(u8[i], layout, depth) for i in range(2))
    cut = RF.content("fade", H, W, 0, layout, depth)
    fmt = (layout, depth)
    assert S.measure(calm[0], calm[1], fmt)["cut"] == 0 and S.measure(cut[0], cut[1], fmt)["cut"] == 1
    return calm, cut


@pytest.mark.parametrize("layout,depth", RF.FORMATS)
def test_forward_on_a_pair_that_is_no_cut_is_the_video_forward(nr, dev, layout, depth):
    import fldr_video
    H, W = 256, 448
    fmt = _fmt(layout, depth)
    calm, _ = _pairs(H, W, layout, depth)
    frames = [_to_dev(p, dev) for p in calm]
    t = [0.25, 0.5, 0.75]
    outs, scene = nr.forward(frames, t, fmt)
    torch.cuda.synchronize()
    ref = fldr_video.NativeVideo(nr.model).forward(frames, t, fmt, fmt)
    torch.cuda.synchronize()
    assert scene == S.measure(calm[0], calm[1], fmt) and scene["cut"] == 0
    for k in range(3):
        for a, b in zip(outs[k], ref[k]):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), k


@pytest.mark.parametrize("layout,depth", RF.FORMATS)
def test_forward_on_a_cut_copies_the_nearer_frame_and_leaves_the_gaps(nr, dev, layout, depth):
    import fldr_video
    H, W = 255, 447                                                     # odd: chroma planes ceil(W / 2) wide
    fmt = _fmt(layout, depth)
    _, cut = _pairs(H, W, layout, depth)
    dirt = np.random.default_rng(5)
    if layout == "nv12" and depth == 10:                                # P010: the low six bits are copied as they are
        cut = tuple(tuple(p | dirt.integers(0, 64, p.shape).astype(np.uint16) for p in fr) for fr in cut)
    frames = [_to_dev(cut[0], dev, pad=6, fill=0x11), _to_dev(cut[1], dev, pad=34, fill=0x22, offset=2)]
    t = [0.25, 0.5, 0.75, 0.49999997, 0.0, 1.0]
    shapes = fldr_video.plane_shapes(fmt, H, W)
    dt = fldr_video.plane_dtype(fmt, numpy=True)
    outs = [_to_dev([np.zeros(s, dt) for s in shapes], dev, pad=10 + 6 * k, fill=0x5A, offset=2 * (k % 2)) for k in range(len(t))]
    _, scene = nr.forward(frames, t, fmt, outs=outs)
    torch.cuda.synchronize()
    assert scene == S.measure(cut[0], cut[1], fmt) and scene["cut"] == 1
    for k, tv in enumerate(t):
        src = cut[0 if np.float32(tv) < np.float32(0.5) else 1]
        for p, (o, w) in enumerate(zip(outs[k], src)):
            assert np.array_equal(o.cpu().numpy(), w), (k, p)
            gaps = _rows_with_gaps(o)[:, o.shape[1] * o.element_size():]
            assert gaps.numel() and bool((gaps == 0x5A).all()), "a gap byte of an output plane was written"


def test_forward_graph_replay_follows_rewritten_times_and_pairs(nr, dev):
    import fldr_video
    H, W = 256, 448
    layout, depth = "i420", 8
    fmt = _fmt(layout, depth)
    calm, cut = _pairs(H, W, layout, depth)
    frames = [_to_dev(p, dev) for p in cut]
    calm_dev = [_to_dev(p, dev) for p in calm]
    t = torch.tensor([0.25, 0.75], device=dev)
    ws = nr.workspace(H, W, 2)
    outs = [fldr_video.empty_frame(fmt, H, W, dev) for _ in range(2)]
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        nr.forward(frames, t, fmt, outs=outs, ws=ws, read=False)         # warm
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        nr.forward(frames, t, fmt, outs=outs, ws=ws, read=False)
    for tv in ((0.25, 0.75), (0.75, 0.25), (0.6, 0.9)):
        t.copy_(torch.tensor(tv))
        g.replay()
        torch.cuda.synchronize()
        for k in range(2):
            for o, w in zip(outs[k], cut[0 if tv[k] < 0.5 else 1]):
                assert np.array_equal(o.cpu().numpy(), w), (tv, k)
    # the captured planes now hold a pair that is no cut: the same graph interpolates
    for f in range(2):
        for dst, src in zip(frames[f], calm_dev[f]):
            dst.copy_(src)
    g.replay()
    torch.cuda.synchronize()
    ref = fldr_video.NativeVideo(nr.model).forward(calm_dev, [0.6, 0.9], fmt, fmt)
    torch.cuda.synchronize()
    import fldr_rate as R
    assert R.read_result(nr.state_of(ws, H, W, 2))["cut"] == 0
    for k in range(2):
        for a, b in zip(outs[k], ref[k]):
            assert torch.equal(a, b), k


def test_bad_forward_calls_enqueue_nothing(nr, dev):
    import fldr_rate as R
    import fldr_video as V
    H, W = 256, 256
    fmt = _fmt("nv12", 8)
    calm, _ = _pairs(H, W, "nv12", 8)
    frames = [_to_dev(p, dev) for p in calm]
    t = torch.tensor([0.5], device=dev)
    ws = nr.workspace(H, W).fill_(0x33)
    outs = [tuple(p.fill_(0x77) for p in V.empty_frame(fmt, H, W, dev))]

    def call(mutate, ws_=ws, params=None):
        io = nr.make_io(frames, t, fmt, fmt, outs, H, W)
        mutate(io)
        return nr.forward_io(io, ws_, params)
    assert call(lambda io: setattr(io.out_format, "layout", 1)) == R.E_FORMAT
    assert call(lambda io: setattr(io.out_format, "depth", 10)) == R.E_FORMAT
    assert call(lambda io: io.out[0].pitch.__setitem__(1, W - 2)) == V.E_PITCH
    assert call(lambda io: setattr(io, "n_t", 0)) == V.E_ARG
    assert call(lambda io: None, params=R.SceneParams(0, 1001)) == R.E_ARG
    assert call(lambda io: None, ws_=ws[:ws.numel() - 256]) == V.E_WORKSPACE   # room for the video forward, not for the scene state
    assert call(lambda io: None, ws_=ws[1:]) == V.E_WORKSPACE
    torch.cuda.synchronize()
    assert bool((ws == 0x33).all()), "a refused call wrote the workspace"
    for p in outs[0]:
        assert bool((p == 0x77).all()), "a refused call wrote an output"
    assert call(lambda io: None) == 0
    torch.cuda.synchronize()
    assert not bool((outs[0][0] == 0x77).all())
    assert nr.workspace_bytes(H, W, 3) == (V.NativeVideo(nr.model).workspace_bytes(H, W, 3) + 255) // 256 * 256 + R.SCENE_STATE_BYTES


# ---- the converter ---------------------------------------------------------------------------------------------------------------------------
def _clip(H, W, n, seed):
    """n frames of a texture moving 4 px down and 6 px right per frame (BGR planar numpy)."""
    import fldr_harness as Hn
    base = Hn.synthetic_pair(H + 4 * n, W + 6 * n, seed=seed).numpy()[0]
    return [np.ascontiguousarray(base[:, 4 * k:4 * k + H, 6 * k:6 * k + W]) for k in range(n)]


@functools.lru_cache(maxsize=1)
def _spliced(H, W):
    """12 I420 frames: six of one moving texture, then six of another, darker one — a cut at frame 6."""
    a, b = _clip(H, W, 6, seed=5), _clip(H, W, 6, seed=11)
    b = [(f.astype(np.float64) * 0.35).round().astype(np.uint8) for f in b]
    return [O.bgr_to_yuv420(f, "bt709", "limited") for f in a + b]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _run_converter(nr, dev, frames, in_rate, out_rate, scene, fmt):
    """Push every frame, then flush; check count, order and bytes of everything returned against schedule() and the forwards of the
    pairs; -> the list of scene dicts per push."""
    import fldr_rate as R
    import fldr_video
    H, W = frames[0][0].shape
    c = R.Converter(nr.model, H, W, fmt, in_rate, out_rate, scene=scene)
    assert c.max_out == R.max_out(in_rate, out_rate)
    sched = R.schedule(len(frames), in_rate, out_rate)
    nv = fldr_video.NativeVideo(nr.model)
    scenes, n_forwards = [], 0
    for n in range(len(frames) + 1):
        outs = c.push(frames[n]) if n < len(frames) else c.flush()
        want = sched[n]
        assert len(outs) == len(want), (n, len(outs), want)
        if n < len(frames):
            scenes.append(c.last_scene)
        if n == 0 or n == len(frames):
            assert all(r == 0 for _, _, r, _ in want)
        measured = S.measure(frames[n - 1], frames[n], fmt) if 0 < n < len(frames) else None
        if 0 < n < len(frames):
            assert c.last_scene == (measured if scene else {"sad": 0, "hist_dist": 0, "cut": 0}), n
        inter = [(k, r, b) for k, (_, _, r, b) in enumerate(want) if r]
        ref = None
        if inter and not (scene and measured["cut"]):
            tt = [float(np.float32(r) / np.float32(b)) for _, r, b in inter]
            pair = [_to_dev(frames[n - 1], dev), _to_dev(frames[n], dev)]
            ref = [_host(o) for o in nv.forward(pair, tt, fmt, fmt)]
            torch.cuda.synchronize()
            n_forwards += 1
        q = 0
        for k, (j, i, r, b) in enumerate(want):
            if r == 0:
                assert _same(outs[k], frames[i]), (n, j)                 # the pushed bytes
            elif ref is None:
                assert i == n - 1 and _same(outs[k], frames[i] if r * 2 < b else frames[i + 1]), (n, j)   # a cut: the nearer frame
                q += 1
            else:
                assert i == n - 1 and _same(outs[k], ref[q]), (n, j)     # the forward of its pair at its t
                q += 1
    assert c.flush() == []                                              # a second flush returns nothing
    return c, scenes, n_forwards


def test_converter_24_to_60_repeats_frames_at_the_cut_and_interpolates_elsewhere(nr, dev):
    H, W = 256, 448
    fmt = _fmt("i420", 8)
    frames = _spliced(H, W)
    c, scenes, _ = _run_converter(nr, dev, frames, 24, 60, True, fmt)
    assert [s["cut"] for s in scenes] == [0] * 6 + [1] + [0] * 5         # the pair (5, 6) only
    # reset: a new stream from frame 0; three frames end exactly on an output, which the flush returns
    import fldr_rate as R
    c.reset()
    assert c.push(frames[0]) == []
    got = c.push(frames[1])
    assert len(got) == 3 and _same(got[0], frames[0])
    assert len(c.push(frames[2])) == 2
    last = c.flush()
    assert len(last) == 1 and _same(last[0], frames[2]) and c.flush() == []
    assert R.schedule(3, 24, 60)[3] == [(5, 2, 0, 5)]
    c.close()
    # the same run with the detector off interpolates the pair (5, 6) too
    c, scenes, _ = _run_converter(nr, dev, frames, 24, 60, False, fmt)
    assert all(s["cut"] == 0 for s in scenes)
    c.close()


def test_converter_10_bit_nv12(nr, dev):
    H, W = 256, 448
    fmt = _fmt("nv12", 10)
    a, b = _clip(H, W, 3, seed=5), _clip(H, W, 2, seed=11)
    b = [(f.astype(np.float64) * 0.35).round().astype(np.uint8) for f in b]
    frames = [RF.planes_of_bgr(f, "nv12", 10) for f in a + b]
    c, scenes, _ = _run_converter(nr, dev, frames, 25, 60, True, fmt)
    assert [s["cut"] for s in scenes] == [0, 0, 0, 1, 0]
    c.close()


def test_converter_60_to_24_runs_a_forward_only_for_the_kept_pairs(nr, dev):
    import fldr_rate as R
    H, W = 256, 448
    fmt = _fmt("i420", 8)
    frames = _spliced(H, W)
    sched = R.schedule(12, 60, 24)
    assert [len(p) for p in sched] == [0, 1, 0, 1, 0, 0, 1, 0, 1, 0, 0, 1, 0]
    c, scenes, n_forwards = _run_converter(nr, dev, frames, 60, 24, True, fmt)
    assert n_forwards == 2                                              # outputs 1 and 3, at 2.5 and 7.5; every pair is measured all the same
    assert [s["cut"] for s in scenes] == [0] * 6 + [1] + [0] * 5
    c.close()
    c, _, _ = _run_converter(nr, dev, frames, 30, 30, True, fmt)       # the identity: every frame once, no forward at all
    c.close()
