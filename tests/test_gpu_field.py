"""The field API (libfldr_field.so through fldr_field) on the GPU.  Every comparison is exact: fldr_field_weave gives the bytes of
tests/field_oracle.py, gap bytes included; fldr_field_forward's temporal frame is fldr_video_forward's output at t = 0.5 on copies of
the two field views and its output the oracle's weave of it; the stream returns what the schedule says, each frame the forward or the
INTRA weave of the frames the plan names."""
import functools

import numpy as np
import pytest
import torch

import field_frames as FF
import field_oracle as F
import rate_frames as RF
import scene_oracle as S

pytestmark = pytest.mark.gpu

SIZES = [(4, 1), (4, 2), (4, 3), (8, 15), (8, 16), (8, 17), (12, 33), (16, 64), (20, 65), (36, 130), (64, 257)]
FILL = 0x5A


@pytest.fixture(scope="module")
def nf(dev):
    import fldr_field
    import fldr_harness as Hn
    import fldr_model
    nm = fldr_model.NativeModel.from_npz(Hn.DEFAULT_WEIGHTS, device=dev.index or 0)
    f = fldr_field.NativeField(nm)
    yield f
    nm.close()


def _fmt(layout, depth=8):
    import fldr_video
    return fldr_video.Format(layout, "bt709", "limited", depth)


def _to_dev(planes, dev, pad=0, fill=0, offsets=(0, 0, 0), pitch16=False):
    """Device copies of host planes (uint8 or uint16); pad / offsets in BYTES: each plane a view into a byte buffer whose rows are `pad`
    bytes longer (gap bytes = fill), plane p starting offsets[p] bytes into its (256-byte aligned) buffer.  pitch16: every pitch is then
    rounded up to a multiple of 16."""
    out = []
    for q, p in enumerate(planes):
        r, c = p.shape
        b = p.dtype.itemsize
        pitch = c * b + pad
        if pitch16:
            pitch = (pitch + 15) // 16 * 16
        off = offsets[q]
        buf = torch.full((r * pitch + off + pitch + 256,), fill, dtype=torch.uint8, device=dev)
        view = buf[off:off + r * pitch].view(r, pitch)[:, :c * b]
        view.copy_(torch.from_numpy(np.ascontiguousarray(p).view(np.uint8).reshape(r, c * b)).to(dev))
        out.append(view.view(torch.uint16) if b == 2 else view)
    return tuple(out)


def _host(frame):
    return tuple(p.cpu().numpy() for p in frame)


def _rows_with_gaps(p):
    """The bytes of a plane view with the gap bytes of every row: uint8 [rows, pitch]."""
    b = p.view(torch.uint8) if p.dtype != torch.uint8 else p
    return b.as_strided((b.shape[0], b.stride(0)), b.stride())


def _blank_out(layout, depth, H, W, dev, pad, offsets, pitch16=False):
    dt = np.uint16 if depth == 10 else np.uint8
    return _to_dev([np.zeros(s, dt) for s in FF.plane_shapes(layout, H, W)], dev, pad=pad, fill=FILL, offsets=offsets, pitch16=pitch16)


def _check_out(out, want):
    """Every byte of the output planes: the rows are the oracle's, the bytes between a row's end and its pitch were never written."""
    for o, w in zip(out, want):
        got = _rows_with_gaps(o).cpu().numpy()
        rb = w.shape[1] * w.dtype.itemsize
        assert np.array_equal(got[:, :rb], np.ascontiguousarray(w).view(np.uint8).reshape(w.shape[0], rb))
        assert (got[:, rb:] == FILL).all()


def _untouched(out):
    """A _blank_out frame nobody wrote: zero rows, FILL between a row's end and its pitch."""
    for o in out:
        got = _rows_with_gaps(o).cpu().numpy()
        rb = o.shape[1] * o.element_size()
        if got[:, :rb].any() or not (got[:, rb:] == FILL).all():
            return False
    return True


def _weave_and_check(dev, layout, depth, cur, prev, nxt, temporal, parity, mode, still=None, slack=None, pad=0, offsets=(0, 0, 0), intra_if=None,
                     want_mode=None, pitch16=False):
    import fldr_field as K
    H, W = cur[0].shape
    d = lambda fr, k: None if fr is None else _to_dev(fr, dev, pad=pad + 16 * k if pad else 0, fill=0x11 * (k + 1), offsets=offsets, pitch16=pitch16)
    frames = [d(cur, 0), d(prev, 1), d(nxt, 2), d(temporal, 3)]
    out = _blank_out(layout, depth, H, W, dev, pad, offsets, pitch16)
    params = None if still is None and slack is None else (F.defaults(depth)[0] if still is None else still, F.defaults(depth)[1] if slack is None else slack)
    K.weave(frames[0], frames[1], frames[2], frames[3], _fmt(layout, depth), parity, mode, intra_if, params, out)
    torch.cuda.synchronize()
    want = F.weave(cur, prev, nxt, temporal, layout, depth, parity, mode if want_mode is None else want_mode, still, slack)
    _check_out(out, want)
    return want


def _noise_set(seed, layout, depth, H, W, dirty=False):
    rng = np.random.default_rng(seed)
    cur, prev, nxt = (FF.noise(rng, layout, depth, H, W, dirty) for _ in range(3))
    return cur, prev, nxt, FF.noise(rng, layout, depth, H // 2, W, dirty)


# ---- the kernel alone -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,depth", FF.FORMATS)
@pytest.mark.parametrize("H,W", SIZES)
def test_weave_equals_the_oracle_at_every_size(dev, H, W, layout, depth):
    cur, prev, nxt, temporal = _noise_set(H * 1000 + W, layout, depth, H, W)
    near = tuple(FF.pack(np.clip(F.value(p, layout, depth) + np.random.default_rng(1).integers(-3, 4, p.shape), 0, F.mx(depth)), layout, depth)
                 for p in prev)                                                # next close to prev: the static rule decides per sample
    for parity in (0, 1):
        _weave_and_check(dev, layout, depth, cur, None, None, None, parity, F.INTRA)
        _weave_and_check(dev, layout, depth, cur, prev, nxt, temporal, parity, F.MOTION)
        _weave_and_check(dev, layout, depth, cur, prev, near, temporal, parity, F.MOTION)


@pytest.mark.parametrize("layout,depth", FF.FORMATS)
@pytest.mark.parametrize("H,W,pad,misaligned", [(8, 17, 15, None), (20, 65, 16, None), (36, 130, 48, 0), (36, 130, 32, 1), (64, 257, 16, 2), (16, 64, 0, 1)])
def test_weave_with_pitches_and_offset_planes(dev, H, W, pad, misaligned, layout, depth):
    """Padded pitches (16-byte aligned or not) and one plane off by a sample, so that the per-sample form runs beside the 16-byte one in
    the same launch."""
    b = 2 if depth == 10 else 1
    if depth == 10:
        pad -= pad % 2
    n_planes = 2 if layout == "nv12" else 3
    offsets = [0, 0, 0]
    if misaligned is not None:
        offsets[min(misaligned, n_planes - 1)] = b
    cur, prev, nxt, temporal = _noise_set(5, layout, depth, H, W, dirty=True)
    for parity in (0, 1):
        for mode in (F.INTRA, F.MOTION):
            _weave_and_check(dev, layout, depth, cur, prev, nxt, temporal, parity, mode, still=3, slack=9, pad=pad, offsets=tuple(offsets))


@pytest.mark.parametrize("access", ["aligned", "offset"])
@pytest.mark.parametrize("layout,depth", FF.FORMATS)
@pytest.mark.parametrize("H,W", [(4, 70001), (2052, 3)])
def test_weave_of_long_rows_and_of_many_rows(dev, H, W, layout, depth, access):
    """The split of a work item into row and group, as the interlacing library's test of the same name walks it.  (4, 70001): thousands
    of groups in a row, the last one partial, so the multiply-high does the dividing; (2052, 3): one group per row, the path without
    the multiply, and more than a thousand own rows.  Every plane aligned and every pitch a multiple of 16 (the 16-byte form) or every
    plane one sample into its buffer (the per-sample form); every byte against the oracle, the bytes between a row's end and its pitch
    untouched."""
    b = 2 if depth == 10 else 1
    cur, prev, nxt, temporal = _noise_set(H + W + depth, layout, depth, H, W)
    for parity in (0, 1):
        for mode in (F.MOTION, F.INTRA):
            _weave_and_check(dev, layout, depth, cur, prev, nxt, temporal, parity, mode, pad=16, offsets=(0, 0, 0) if access == "aligned" else (b, b, b),
                             pitch16=True)


@pytest.mark.parametrize("layout,depth", FF.FORMATS)
def test_weave_static_threshold_at_the_edges_and_in_a_neighbour_column(dev, layout, depth):
    H, W = 8, 40                                                       # luma: three 16-byte groups at depth 8, five at depth 10
    rng = np.random.default_rng(9)
    cur = FF.noise(rng, layout, depth, H, W)
    prev = tuple(FF.pack(np.clip(F.value(p, layout, depth), 40, F.mx(depth) - 40), layout, depth) for p in FF.noise(rng, layout, depth, H, W))
    temporal = FF.noise(rng, layout, depth, H // 2, W)
    still = F.defaults(depth)[0]
    ns = 16 if depth == 8 else 8
    seen = set()
    for p in range(len(cur)):
        comp = F.components(layout, p)
        row = prev[p].shape[1]
        # the first and last column of each component, both sides of every group boundary
        xs = sorted(set([0, comp - 1, row - comp, row - 1] + [x for g in range(ns, row, ns) for x in (g - comp, g - 1, g, g + comp - 1) if x < row]))
        for parity in (0, 1):
            y = 1 - parity + 2
            for x in xs:
                outs = []
                for delta in (still, still + 1, -still, -still - 1):
                    nxt = FF.add(prev, layout, depth, p, y, x, delta)
                    outs.append(_weave_and_check(dev, layout, depth, cur, prev, nxt, temporal, parity, F.MOTION, slack=0))
                seen.add(all(np.array_equal(a, b) for a, b in zip(outs[0], outs[1])))
    assert seen == {False}                                             # one code more than `still` changes the output: the test can tell


@pytest.mark.parametrize("layout,depth", FF.FORMATS)
def test_weave_code_range_ends_slack_and_still_extremes(dev, layout, depth):
    H, W = 12, 33
    top = F.mx(depth)
    cur, prev, nxt, temporal = _noise_set(21, layout, depth, H, W)
    zero, full = FF.flat(layout, depth, H, W, 0), FF.flat(layout, depth, H, W, top)
    t0, t1 = FF.flat(layout, depth, H // 2, W, 0), FF.flat(layout, depth, H // 2, W, top)
    for parity in (0, 1):
        for c in (zero, full):                                         # both ends of the clamp meet the code range
            for t in (t0, t1, temporal):
                for slack in (0, 5, top):
                    _weave_and_check(dev, layout, depth, c, prev, nxt, t, parity, F.MOTION, still=-1, slack=slack)
            _weave_and_check(dev, layout, depth, c, zero, full, temporal, parity, F.MOTION, still=top, slack=0)      # d = mx is still static
            _weave_and_check(dev, layout, depth, c, None, None, None, parity, F.INTRA)
        for still, slack in ((-1, 0), (-1, top), (top, 0), (top, top), (0, 0)):
            _weave_and_check(dev, layout, depth, cur, prev, nxt, temporal, parity, F.MOTION, still=still, slack=slack)
        want = _weave_and_check(dev, layout, depth, cur, prev, nxt, temporal, parity, F.MOTION, still=-1, slack=top)
        for w, t in zip(want, temporal):                               # slack = mx with the static rule off returns temporal
            assert np.array_equal(w[1 - parity::2], t)
        _weave_and_check(dev, layout, depth, cur, prev, prev, temporal, parity, F.MOTION)                           # prev == next: static
        want = _weave_and_check(dev, layout, depth, cur, cur, cur, temporal, parity, F.MOTION)                      # a still woven picture
        assert all(np.array_equal(w, c) for w, c in zip(want, cur))


@pytest.mark.parametrize("layout", ["nv12", "i420"])
def test_weave_ignores_dirty_bits_and_writes_canonical_words(dev, layout):
    H, W = 20, 65
    clean = _noise_set(33, layout, 10, H, W)
    rng = np.random.default_rng(34)
    dirty = tuple(tuple(FF.pack(F.value(p, layout, 10), layout, 10, rng.integers(1, 64, p.shape)) for p in fr) for fr in clean)
    for parity in (0, 1):
        for mode in (F.INTRA, F.MOTION):
            a = _weave_and_check(dev, layout, 10, clean[0], clean[1], clean[2], clean[3], parity, mode)
            b = _weave_and_check(dev, layout, 10, dirty[0], dirty[1], dirty[2], dirty[3], parity, mode)
            for p, (x, y) in enumerate(zip(a, b)):
                assert np.array_equal(x[1 - parity::2], y[1 - parity::2])                        # computed rows: canonical, the same
                assert np.array_equal(y[parity::2], dirty[0][p][parity::2])                      # own rows: the input's bytes as they are
                assert not np.array_equal(x[parity::2], y[parity::2])


def test_weave_intra_if_and_graph_replay_follow_the_device_word(dev):
    import fldr_field as K
    layout, depth, H, W, parity = "nv12", 8, 36, 130, 1
    fmt = _fmt(layout, depth)
    cur, prev, nxt, temporal = _noise_set(41, layout, depth, H, W)
    want = {m: F.weave(cur, prev, nxt, temporal, layout, depth, parity, m) for m in (F.MOTION, F.INTRA)}
    assert not all(np.array_equal(a, b) for a, b in zip(want[F.MOTION], want[F.INTRA]))
    word = torch.zeros(4, dtype=torch.int32, device=dev)
    for v, m in ((0, F.MOTION), (1, F.INTRA), (0x80000000 - 1, F.INTRA)):
        word[0] = v
        _weave_and_check(dev, layout, depth, cur, prev, nxt, temporal, parity, F.MOTION, intra_if=word, want_mode=m)
    word[0] = 0
    _weave_and_check(dev, layout, depth, cur, prev, nxt, temporal, parity, F.INTRA, intra_if=word)      # the mode of the call holds without the word
    frames = [_to_dev(f, dev) for f in (cur, prev, nxt, temporal)]
    out = _blank_out(layout, depth, H, W, dev, 16, (0, 0, 0))
    s = torch.cuda.Stream(device=dev)                                  # one stream, no parallel branches
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        K.weave(*frames, fmt, parity, K.MOTION, word, None, out)       # warm
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        K.weave(*frames, fmt, parity, K.MOTION, word, None, out)
    for v, m in ((1, F.INTRA), (0, F.MOTION), (1, F.INTRA)):
        word[0] = v
        for o in out:
            _rows_with_gaps(o).fill_(FILL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        _check_out(out, want[m])


def test_bad_weave_calls_enqueue_nothing(dev):
    import fldr_field as K
    import fldr_video as V
    layout, depth, H, W = "i420", 8, 16, 64
    fmt = _fmt(layout, depth)
    cur, prev, nxt, temporal = (V.frame_struct(_to_dev(f, dev)) for f in _noise_set(51, layout, depth, H, W))
    out_t = _blank_out(layout, depth, H, W, dev, 16, (0, 0, 0))
    out = V.frame_struct(out_t)
    sp = K._stream_ptr(dev, None)
    call = lambda **kw: K.weave_raw(kw.get("H", H), W, fmt, cur, kw.get("prev", prev), nxt, temporal, kw.get("parity", 0), kw.get("mode", K.MOTION), None,
                                    kw.get("params"), kw.get("out", out), sp)
    assert call(H=18) == K.E_SIZE and call(parity=2) == K.E_ARG and call(mode=2) == K.E_ARG and call(prev=None) == K.E_ARG
    assert call(params=K.Params(256, 0)) == K.E_ARG and call(params=K.Params(0, -1)) == K.E_ARG
    bad = V.frame_struct(out_t)
    bad.pitch[1] = W // 2 - 1
    assert call(out=bad) == V.E_PITCH
    torch.cuda.synchronize()
    assert _untouched(out_t)
    assert call() == 0
    torch.cuda.synchronize()
    assert not _untouched(out_t)


# ---- the forward ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def _woven(H, W, layout, depth):
    """(prev, cur, next): three woven frames of a moving scene, and `far`, a frame of another picture."""
    a, b = FF.pictures(H, W, layout, depth)
    c = RF.content("cut", H, W, 0, layout, depth)[1]
    return FF.interlace(a, b), FF.interlace(a, a), FF.interlace(b, a), FF.interlace(c, c)


def _field_copies(frame, parity, dev):
    return _to_dev(tuple(np.ascontiguousarray(p) for p in F.field_view(frame, parity)), dev)


@pytest.mark.parametrize("layout,depth", FF.FORMATS)
@pytest.mark.parametrize("H,W", [(400, 301), (512, 384)])
def test_forward_is_the_video_forward_on_the_field_views_then_the_weave(nf, dev, H, W, layout, depth):
    import fldr_video
    fmt = _fmt(layout, depth)
    prev, cur, nxt, far = _woven(H, W, layout, depth)
    parity = 1 if H == 400 else 0
    views = (F.field_view(prev, 1 - parity), F.field_view(nxt, 1 - parity))
    assert S.measure(views[0], views[1], (layout, depth))["cut"] == 0
    d = [_to_dev(f, dev, pad=16 * k, fill=0x22) for k, f in enumerate((cur, prev, nxt))]
    ws = nf.workspace(H, W)
    out = _blank_out(layout, depth, H, W, dev, 48, (0, 0, 0))
    nf.forward(d[0], d[1], d[2], fmt, parity, scene=True, out=out, ws=ws)
    torch.cuda.synchronize()
    temporal = nf.temporal(ws, H, W, fmt)
    for q, p in enumerate(temporal):
        assert p.data_ptr() % 256 == 0 and (p.stride(0) * p.element_size()) % 256 == 0, q
    ref = fldr_video.NativeVideo(nf.model).forward((_field_copies(prev, 1 - parity, dev), _field_copies(nxt, 1 - parity, dev)), [0.5], fmt, fmt)[0]
    torch.cuda.synchronize()
    for a, b in zip(temporal, ref):
        assert torch.equal(a.contiguous().view(torch.uint8), b.view(torch.uint8))
    _check_out(out, F.weave(cur, prev, nxt, _host(temporal), layout, depth, parity, F.MOTION))
    assert nf.scene_result(ws, H, W) == S.measure(views[0], views[1], (layout, depth))
    # two different pictures before and after: INTRA with the measure, MOTION without
    d[2] = _to_dev(far, dev)
    views = (views[0], F.field_view(far, 1 - parity))
    assert S.measure(views[0], views[1], (layout, depth))["cut"] == 1
    want_intra = F.weave(cur, None, None, None, layout, depth, parity, F.INTRA)
    for scene in (True, False):
        for o in out:
            _rows_with_gaps(o).fill_(FILL)
        nf.forward(d[0], d[1], d[2], fmt, parity, scene=scene, out=out, ws=ws)
        torch.cuda.synchronize()
        want_motion = F.weave(cur, prev, far, _host(nf.temporal(ws, H, W, fmt)), layout, depth, parity, F.MOTION)
        assert not all(np.array_equal(a, b) for a, b in zip(want_motion, want_intra))
        _check_out(out, want_intra if scene else want_motion)
        if scene:
            r = nf.scene_result(ws, H, W)
            assert r["cut"] == 1 and r == S.measure(views[0], views[1], (layout, depth))


def test_bad_forward_calls_enqueue_nothing_and_small_fields_are_refused(nf, dev):
    import fldr_field as K
    import fldr_model as M
    import fldr_video as V
    layout, depth, H, W = "nv12", 8, 400, 301
    fmt = _fmt(layout, depth)
    prev, cur, nxt, _ = _woven(H, W, layout, depth)
    d = [_to_dev(f, dev) for f in (cur, prev, nxt)]
    out = _blank_out(layout, depth, H, W, dev, 16, (0, 0, 0))
    ws = nf.workspace(H, W).fill_(0x33)
    need = nf.workspace_bytes(H, W)
    io = lambda **kw: nf.make_io(d[0], d[1], d[2], fmt, kw.get("parity", 0), True, kw.get("scene_params"), kw.get("params"), out)
    assert nf.forward_io(io(), ws[256:]) == K.E_WORKSPACE and nf.forward_io(io(), ws[16:]) == K.E_WORKSPACE
    assert nf.forward_io(io(), ws[:need - 256]) == K.E_WORKSPACE and nf.forward_io(io(), None) == K.E_WORKSPACE
    assert nf.forward_io(io(), ws, model=False) == K.E_ARG
    assert nf.forward_io(io(parity=2), ws) == K.E_ARG and nf.forward_io(io(params=(256, 0)), ws) == K.E_ARG
    assert nf.forward_io(io(scene_params=(1001, 0)), ws) == -200
    bad = io()
    bad.next.pitch[0] = W - 1
    assert nf.forward_io(bad, ws) == V.E_PITCH
    # the model's reflect padding needs pad < size: a field of 128 rows is refused, before anything is enqueued
    small = [_to_dev(FF.noise(np.random.default_rng(k), layout, depth, 256, W), dev) for k in range(3)]
    sio = nf.make_io(small[0], small[1], small[2], fmt, 0, True, None, None, _blank_out(layout, depth, 256, W, dev, 0, (0, 0, 0)))
    assert nf.forward_io(sio, ws) == M.E_SHAPE
    assert K.lib().fldr_field_workspace_bytes(nf.model._h, 256, W) == M.E_SHAPE
    torch.cuda.synchronize()
    assert bool((ws == 0x33).all()) and _untouched(out)


# ---- the stream -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _sequence(H, W, layout, depth, tff):
    a, b = FF.pictures(H, W, layout, depth)
    c, e = FF.pictures(H, W, layout, depth, seed=8)
    return [FF.interlace(a, b, tff), FF.interlace(b, a, tff), FF.interlace(a, a, tff), FF.interlace(c, e, tff), FF.interlace(e, c, tff),
            FF.interlace(c, c, tff)]


@pytest.mark.parametrize("tff", [True, False])
@pytest.mark.parametrize("rate", [1, 2])
@pytest.mark.parametrize("layout,depth,H,W", [("i420", 8, 400, 301), ("nv12", 10, 400, 302)])      # chroma rows of 151 bytes: no multiple of 16
def test_stream_returns_what_the_plan_says(nf, dev, tff, rate, layout, depth, H, W):
    import fldr_field as K
    fmt = _fmt(layout, depth)
    frames = _sequence(H, W, layout, depth, tff)
    N = len(frames)
    dframes = [_to_dev(f, dev) for f in frames]
    stream = K.Stream(nf.model, H, W, fmt, tff=tff, rate=rate, scene=True)
    assert stream.max_out == rate
    ws = nf.workspace(H, W)

    def run():
        got = []
        for n in range(N):
            got.append((stream.push(frames[n]), stream.last_reports))
        got.append((stream.flush(), stream.last_reports))
        assert stream.flush() == []                                    # a second flush returns none
        return got
    got = run()
    want = F.stream_outputs(N, tff, rate)
    assert [len(o) for o, _ in got] == [len(w) for w in want]
    for n, (outs, reports) in enumerate(got):
        for k, (p, mode) in enumerate(want[n]):
            rep = reports[k]
            assert (rep["field"], rep["parity"]) == (p["field"], p["parity"]) and p["parity"] == F.par(p["field"], tff)
            if mode == F.INTRA:
                ref = F.weave(frames[p["cur"]], None, None, None, layout, depth, p["parity"], F.INTRA)
                assert rep["mode_used"] == K.INTRA and rep["cut"] == 0 and rep["scene"] == {"sad": 0, "hist_dist": 0, "cut": 0}
            else:
                ref = _host(nf.forward(dframes[p["cur"]], dframes[p["prev"]], dframes[p["next"]], fmt, p["parity"], scene=True, ws=ws))
                scene = nf.scene_result(ws, H, W)
                views = [F.field_view(frames[p[w]], 1 - p["parity"]) for w in ("prev", "next")]
                assert rep["scene"] == scene == S.measure(views[0], views[1], (layout, depth))
                assert rep["cut"] == scene["cut"] and rep["mode_used"] == (K.INTRA if scene["cut"] else K.MOTION)
            for a, b in zip(outs[k], ref):
                assert np.array_equal(a, b), (n, k)
    cuts = [r["cut"] for _, reps in got for r in reps]
    assert 1 in cuts and 0 in cuts[1:-1]                               # the sequence changes scene once; elsewhere the model runs
    # reset starts over: the same stream again gives the same frames
    stream.reset()
    again = run()
    for (o1, r1), (o2, r2) in zip(got, again):
        assert r1 == r2 and len(o1) == len(o2)
        for f1, f2 in zip(o1, o2):
            assert all(np.array_equal(a, b) for a, b in zip(f1, f2))
    stream.close()


@pytest.mark.parametrize("rate", [1, 2])
def test_stream_returns_a_still_picture_for_every_interior_output(nf, dev, rate):
    import fldr_field as K
    layout, depth, H, W = "nv12", 8, 400, 301
    picture = FF.pictures(H, W, layout, depth)[0]
    stream = K.Stream(nf.model, H, W, _fmt(layout, depth), tff=True, rate=rate, scene=True)
    outs, modes = [], []
    for n in range(6):
        outs += stream.push(picture)
        modes += [r["mode_used"] for r in stream.last_reports]
    outs += stream.flush()
    modes += [r["mode_used"] for r in stream.last_reports]
    assert len(outs) == 6 * rate and modes == [K.INTRA] + [K.MOTION] * (len(outs) - rate) + [K.INTRA] * (rate - 1)
    for o, m in zip(outs, modes):
        if m == K.MOTION:
            assert all(np.array_equal(a, b) for a, b in zip(o, picture))
    stream.close()
