"""The interlace API (libfldr_interlace.so through fldr_interlace) on the GPU.  Every comparison is exact.  fldr_interlace_weave gives
the bytes of tests/interlace_oracle.py at every size, format, filter, choice of sources and access form, and leaves the rows of an absent
parity and all pitch padding alone.  fldr_interlace_forward leaves in its temporaries what fldr_rate.NativeRate / fldr_video.NativeVideo
give for the pair, and weaves them as the oracle does.  A stream returns, push by push, the oracle's weave of outputs 2k and 2k + 1 of a
fldr_rate.Converter at the doubled rate — which tests/test_gpu_rate.py holds to its schedule and forwards — and reports the library's
plan.  The stream's frames are those of tests/cadence_frames.py: a moving texture of 256 x 448 with one cut, made by rate_frames."""
import numpy as np
import pytest
import torch

import cadence_frames as CF
import interlace_oracle as O

pytestmark = pytest.mark.gpu

FORMATS = [("nv12", 8), ("i420", 8), ("nv12", 10), ("i420", 10)]
SIZES = [(4, 1), (4, 2), (4, 3), (8, 15), (8, 16), (8, 17), (12, 33), (16, 64), (20, 65), (36, 130), (64, 257)]
FILTERS = (O.NONE, O.LINEAR, O.COMPLEX)
FILL = 0x5A


def _fmt(layout, depth=8):
    import fldr_video
    return fldr_video.Format(layout, "bt709", "limited", depth)


def _noise_frame(layout, depth, H, W, g):
    """Noise over the whole code range; P010 with noise in the low six bits, yuv420p10le with noise in the high six."""
    import fldr_video as V
    out = []
    for s in V.plane_shapes(layout, H, W):
        if depth == 8:
            out.append(g.integers(0, 256, s).astype(np.uint8))
        else:
            out.append(g.integers(0, 65536, s).astype(np.uint16))
    return tuple(out)


def _plane_to_dev(p, dev, offset=0, pad=16, fill=FILL):
    """A device view of a host plane `offset` bytes into a buffer, with a pitch of the row bytes rounded up to 16, plus `pad`.
    offset 0 and pad a multiple of 16: the 16-byte accesses; anything else: the per-sample form.  -> (view, buffer, mask of row bytes)."""
    r, c = p.shape
    b = p.dtype.itemsize
    pitch = (c * b + 15) // 16 * 16 + pad
    buf = torch.full((r * pitch + offset + 256,), fill, dtype=torch.uint8, device=dev)
    view = buf[offset:offset + r * pitch].view(r, pitch)[:, :c * b]
    view.copy_(torch.from_numpy(np.ascontiguousarray(p).view(np.uint8).reshape(r, c * b)).to(dev))
    mask = np.zeros(buf.numel(), bool)
    mask[offset:offset + r * pitch].reshape(r, pitch)[:, :c * b] = True
    return (view.view(torch.uint16) if b == 2 else view), buf, mask


def _frame_to_dev(frame, dev, access="aligned"):
    b = frame[0].dtype.itemsize
    kw = dict(offset=0, pad=16) if access == "aligned" else dict(offset=b, pad=16 + 3 * b)
    parts = [_plane_to_dev(p, dev, **kw) for p in frame]
    for view, _, _ in parts:
        aligned = view.data_ptr() % 16 == 0 and (view.stride(0) * b) % 16 == 0
        assert aligned == (access == "aligned")
    return parts


def _np(view):
    a = (view.view(torch.int16) if view.dtype == torch.uint16 else view).cpu().numpy()
    return a.view(np.uint16) if view.dtype == torch.uint16 else a


def _check_weave(dev, host_even, host_odd, layout, depth, access, filters=FILTERS, sources=("both", "even", "odd")):
    """The weave of two host frames on the device against the oracle; the outputs start filled with FILL, which the rows of an absent
    parity, the gaps and the bytes around every plane keep."""
    import fldr_interlace as K
    fmt = _fmt(layout, depth)
    even = tuple(v for v, _, _ in _frame_to_dev(host_even, dev, access))
    odd = tuple(v for v, _, _ in _frame_to_dev(host_odd, dev, access))
    blank = tuple(np.full_like(p, FILL | (FILL << 8) if depth == 10 else FILL) for p in host_even)
    for filt in filters:
        for src in sources:
            outs = _frame_to_dev(blank, dev, access)
            out = tuple(v for v, _, _ in outs)
            K.weave(even if src != "odd" else None, odd if src != "even" else None, out, fmt, filt)
            torch.cuda.synchronize()
            want = O.weave(host_even if src != "odd" else None, host_odd if src != "even" else None, layout, depth, filt, out=blank)
            for p, (view, buf, mask) in enumerate(outs):
                got = _np(view)
                assert np.array_equal(got, want[p]), (filt, src, p, np.argwhere(got != want[p])[:4])
                assert (buf.cpu().numpy()[~mask] == FILL).all(), (filt, src, p)
            if src == "even":
                assert all((w[1::2] == b[1::2]).all() for w, b in zip(want, blank))            # the oracle itself left the odd rows alone


# ---- fldr_interlace_weave -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("access", ["aligned", "offset"])
@pytest.mark.parametrize("layout,depth", FORMATS)
@pytest.mark.parametrize("H,W", SIZES)
def test_weave_equals_the_oracle_and_leaves_the_rest_alone(dev, H, W, layout, depth, access):
    g = np.random.default_rng(H * 1000 + W + depth)
    _check_weave(dev, _noise_frame(layout, depth, H, W, g), _noise_frame(layout, depth, H, W, g), layout, depth, access)


@pytest.mark.parametrize("access", ["aligned", "offset"])
@pytest.mark.parametrize("layout,depth", FORMATS)
@pytest.mark.parametrize("H,W", [(4, 70001), (2052, 3)])
def test_weave_of_long_rows_and_of_many_rows(dev, H, W, layout, depth, access):
    """(4, 70001): thousands of groups in a row, the last one partial; (2052, 3): one group per row and more than two thousand rows."""
    g = np.random.default_rng(H + W + depth)
    _check_weave(dev, _noise_frame(layout, depth, H, W, g), _noise_frame(layout, depth, H, W, g), layout, depth, access,
                 sources=("both", "odd"))


@pytest.mark.parametrize("layout,depth", [("nv12", 8), ("i420", 10)])
def test_one_plane_off_a_16_byte_boundary_takes_the_per_sample_path(dev, layout, depth):
    """Every other plane stays aligned: the access form is decided per plane.  Offsets 1 .. 15 bytes (even ones at depth 10) of a source
    plane and of an output plane, and a pitch that is no multiple of 16."""
    import fldr_interlace as K
    H, W = 8, 37
    b = 2 if depth == 10 else 1
    fmt = _fmt(layout, depth)
    g = np.random.default_rng(depth)
    he, ho = _noise_frame(layout, depth, H, W, g), _noise_frame(layout, depth, H, W, g)
    blank = tuple(np.full_like(p, FILL | (FILL << 8) if depth == 10 else FILL) for p in he)
    want = {f: O.weave(he, ho, layout, depth, f) for f in FILTERS}
    for off in range(b, 16, b):
        for where in ("source", "out", "pitch"):
            which = off % len(he)                                           # the plane that is moved
            ev = [_plane_to_dev(p, dev, offset=off if (where, q) == ("source", which) else 0) for q, p in enumerate(he)]
            od = [_plane_to_dev(p, dev, pad=16 + (off if (where, q) == ("pitch", which) else 0)) for q, p in enumerate(ho)]
            for filt in FILTERS:
                outs = [_plane_to_dev(p, dev, offset=off if (where, q) == ("out", which) else 0) for q, p in enumerate(blank)]
                K.weave(tuple(v for v, _, _ in ev), tuple(v for v, _, _ in od), tuple(v for v, _, _ in outs), fmt, filt)
                torch.cuda.synchronize()
                for p, (view, buf, mask) in enumerate(outs):
                    assert np.array_equal(_np(view), want[filt][p]), (off, where, filt, p)
                    assert (buf.cpu().numpy()[~mask] == FILL).all(), (off, where, filt, p)


@pytest.mark.parametrize("layout,depth", FORMATS)
def test_code_range_ends_clamp_on_both_sides(dev, layout, depth):
    """Alternating and stepped rows of 0 and mx: under COMPLEX the sums go below 0 and above 8 mx, and both clamps act."""
    import fldr_video as V
    H, W = 16, 40
    mx = 1023 if depth == 10 else 255
    word = (mx << 6) if (layout, depth) == ("nv12", 10) else mx
    dt = np.uint16 if depth == 10 else np.uint8
    shapes = V.plane_shapes(layout, H, W)

    def rows(pattern):
        return tuple(np.repeat(np.array([[word if pattern(y) else 0] for y in range(r)], dt), c, axis=1) for r, c in shapes)
    patterns = {"alternating": lambda y: y % 2 == 1, "pairs": lambda y: y % 4 >= 2, "step": lambda y: y >= 3, "one row": lambda y: y == 2,
                "one dark row": lambda y: y != 3, "full": lambda y: True}
    for name, pat in patterns.items():
        f = rows(pat)
        inv = rows(lambda y: not pat(y))
        _check_weave(dev, f, inv, layout, depth, "aligned", sources=("both",))
    s = O.value(rows(patterns["step"])[0], layout, depth)[:, 0]                # 0 0 0 mx mx ...: row 1 sees -mx alone, row 4 sees 9 mx
    raw = -s[2] + 2 * s[3] + 6 * s[4] + 2 * s[5] - s[6] + 4
    assert (raw >> 3) > mx and ((-s[0] + 2 * s[0] + 6 * s[1] + 2 * s[2] - s[3] + 4) >> 3) < 0          # both sides of the range are left


def test_p010_dirty_low_bits_are_copied_by_none_and_dropped_by_the_filters(dev):
    H, W = 12, 33
    g = np.random.default_rng(10)
    e, o = _noise_frame("nv12", 10, H, W, g), _noise_frame("nv12", 10, H, W, g)
    assert (e[0] & 63).any() and (o[1] & 63).any()
    none = O.weave(e, o, "nv12", 10, O.NONE)
    assert all(np.array_equal(n[0::2], a[0::2]) and np.array_equal(n[1::2], b[1::2]) for n, a, b in zip(none, e, o)) and (none[0] & 63).any()
    clean = tuple(p & 0xffc0 for p in e), tuple(p & 0xffc0 for p in o)
    for filt in (O.LINEAR, O.COMPLEX):
        w = O.weave(e, o, "nv12", 10, filt)
        assert not any((p & 63).any() for p in w)                           # canonical words
        assert all(np.array_equal(a, b) for a, b in zip(w, O.weave(clean[0], clean[1], "nv12", 10, filt)))      # the low bits were ignored
    _check_weave(dev, e, o, "nv12", 10, "aligned")                          # ... and the device does the same
    # yuv420p10le: the six high bits are ignored by the filters and come out zero
    e, o = _noise_frame("i420", 10, H, W, g), _noise_frame("i420", 10, H, W, g)
    assert (e[0] >> 10).any()
    w = O.weave(e, o, "i420", 10, O.COMPLEX)
    assert not any((p >> 10).any() for p in w)
    _check_weave(dev, e, o, "i420", 10, "offset")


@pytest.mark.parametrize("layout,depth", [("nv12", 8), ("nv12", 10), ("i420", 10)])
def test_a_weave_captured_once_follows_rewritten_sources(dev, layout, depth):
    import fldr_interlace as K
    H, W = 36, 130
    fmt = _fmt(layout, depth)
    g = np.random.default_rng(depth + 1)
    hosts = [(_noise_frame(layout, depth, H, W, g), _noise_frame(layout, depth, H, W, g)) for _ in range(3)]
    even = tuple(v for v, _, _ in _frame_to_dev(hosts[0][0], dev))
    odd = tuple(v for v, _, _ in _frame_to_dev(hosts[0][1], dev))
    out = tuple(v for v, _, _ in _frame_to_dev(tuple(np.zeros_like(p) for p in hosts[0][0]), dev))
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        K.weave(even, odd, out, fmt, K.COMPLEX)                             # warm
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        K.weave(even, odd, out, fmt, K.COMPLEX)
    for he, ho in hosts[1:] + hosts[:1]:
        for d, f in ((even, he), (odd, ho)):
            for t, p in zip(d, f):
                (t.view(torch.uint8) if depth == 10 else t).copy_(torch.from_numpy(np.ascontiguousarray(p).view(np.uint8).reshape(p.shape[0], -1)).to(dev))
        graph.replay()
        torch.cuda.synchronize()
        for o, w in zip(out, O.weave(he, ho, layout, depth, O.COMPLEX)):
            assert np.array_equal(_np(o), w)


def test_bad_weave_calls_leave_the_output_untouched(dev):
    import fldr_interlace as K
    import fldr_video as V
    H, W = 16, 64
    fmt = _fmt("nv12", 8)
    g = np.random.default_rng(0)
    even = tuple(torch.from_numpy(p).to(dev) for p in _noise_frame("nv12", 8, H, W, g))
    odd = tuple(torch.from_numpy(p).to(dev) for p in _noise_frame("nv12", 8, H, W, g))
    out = tuple(torch.full_like(p, 0x44) for p in even)
    fe, fo, fout = V.frame_struct(even), V.frame_struct(odd), V.frame_struct(out)
    sp = V._stream_ptr(dev, None)
    assert K.weave_raw(H, W, fmt, None, None, 0, fout, sp) == K.E_ARG
    assert K.weave_raw(H, W, fmt, fe, fo, 3, fout, sp) == K.E_ARG
    assert K.weave_raw(H - 2, W, fmt, fe, fo, 0, fout, sp) == K.E_ARG
    bad = _fmt("nv12", 8)
    bad.depth = 9
    assert K.weave_raw(H, W, bad, fe, fo, 0, fout, sp) == V.E_FORMAT
    short = V.frame_struct(out)
    short.pitch[1] = W - 1
    assert K.weave_raw(H, W, fmt, fe, fo, 0, short, sp) == V.E_PITCH
    both = V.frame_struct(out)
    both.plane[1] = even[0].data_ptr() + 8                                  # out's chroma inside a source's luma
    assert K.weave_raw(H, W, fmt, fe, fo, 0, both, sp) == K.E_ARG
    assert K.weave_raw(H, W, fmt, fout, fo, 1, fout, sp) == K.E_ARG         # out is a source
    torch.cuda.synchronize()
    assert all(bool((p == 0x44).all()) for p in out)
    assert K.weave_raw(H, W, fmt, fe, None, 1, fout, sp) == 0               # and a good call does write: the even rows alone
    torch.cuda.synchronize()
    assert bool((out[0][1::2] == 0x44).all()) and not bool((out[0][0::2] == 0x44).all())


# ---- fldr_interlace_forward -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nm(dev):
    import fldr_harness as Hn
    import fldr_model
    m = fldr_model.NativeModel.from_npz(Hn.DEFAULT_WEIGHTS, device=dev.index or 0)
    yield m
    m.close()


def _dev_frame(planes, dev):
    out = []
    for p in planes:
        t = torch.from_numpy(p.view(np.int16) if p.dtype == np.uint16 else p).to(dev)
        out.append(t.view(torch.uint16) if p.dtype == np.uint16 else t)
    return tuple(out)


def _host(frame):
    return tuple(_np(p) for p in frame)


@pytest.mark.parametrize("layout,depth", [("nv12", 8), ("i420", 10), ("nv12", 10)])
@pytest.mark.parametrize("scene", [True, False])
def test_forward_temporaries_are_the_rate_forward_and_the_rows_are_woven(nm, dev, layout, depth, scene):
    import fldr_interlace as K
    import fldr_rate as R
    import fldr_video as V
    H, W = CF.H, CF.W
    fmt = _fmt(layout, depth)
    real = CF.real_frames(layout, depth)
    ni = K.NativeInterlace(nm)
    t = [0.2, 0.6, 0.8]
    parity, target = [1, 0, 1], [0, 1, 1]                                   # field 0 -> odd rows of frame 0; fields 1, 2 -> frame 1
    for pair, is_cut in (((0, 1), 0), ((CF.CUT_AT - 1, CF.CUT_AT), 1)):
        frames = [_dev_frame(real[i], dev) for i in pair]
        if scene:
            ref, res = R.NativeRate(nm).forward(frames, t, fmt)
            assert res["cut"] == is_cut
        else:
            ref = V.NativeVideo(nm).forward(frames, t, fmt, fmt)
        torch.cuda.synchronize()
        ref = [_host(f) for f in ref]
        if scene and is_cut:                                                # the nearer frame, its bytes
            for k, tk in enumerate(t):
                assert all(np.array_equal(a, b) for a, b in zip(ref[k], real[pair[0] if tk < 0.5 else pair[1]]))
        blank = tuple(np.full_like(p, 0x3333 if depth == 10 else 0x33) for p in real[0])     # every byte 0x33
        woven = [_dev_frame(blank, dev) for _ in range(2)]
        for filt in (K.LINEAR, K.COMPLEX, K.NONE):
            for w in woven:
                for p in w:
                    (p.view(torch.uint8) if depth == 10 else p).fill_(0x33)
            outs, fields, got = ni.forward(frames, t, [woven[k] for k in target], parity, fmt, filt, scene)
            torch.cuda.synchronize()
            assert (got["cut"] == is_cut) if scene else got is None
            for k in range(3):
                assert all(np.array_equal(a, b) for a, b in zip(_host(fields[k]), ref[k])), (pair, filt, k)
            want0 = O.weave(None, ref[0], layout, depth, filt, out=blank)
            want1 = O.weave(ref[1], ref[2], layout, depth, filt)
            for got_f, want in ((woven[0], want0), (woven[1], want1)):
                assert all(np.array_equal(a, b) for a, b in zip(_host(got_f), want)), (pair, filt)


def test_bad_forward_calls_leave_the_outputs_untouched(nm, dev):
    import fldr_interlace as K
    import fldr_model
    import fldr_video as V
    H, W = CF.H, CF.W
    layout, depth = "nv12", 8
    fmt = _fmt(layout, depth)
    real = CF.real_frames(layout, depth)
    frames = [_dev_frame(real[i], dev) for i in (0, 1)]
    ni = K.NativeInterlace(nm)
    out = _dev_frame(tuple(np.full_like(p, 0x44) for p in real[0]), dev)
    ws = ni.workspace(H, W, 2)
    assert ws.numel() == ni.workspace_bytes(H, W, 2) > fldr_model.lib().fldr_model_workspace_bytes(nm._h, H, W, 2)
    tt = ni._t([0.25, 0.75])
    make = lambda **kw: ni.make_interlace_io(frames, tt, fmt, [out, out], kw.pop("parity", [0, 1]), kw.pop("filter", 1), True, None, H, W)
    assert ni.forward_raw(make(), ws, ws_bytes=ws.numel() - 1) == K.E_ARG                       # a short workspace
    assert ni.forward_raw(make(), ws[256:]) == K.E_ARG
    assert ni.forward_raw(make(), None) == K.E_ARG
    assert ni.forward_raw(make(), ws, model=False) == K.E_ARG
    assert ni.forward_raw(make(parity=[0, 2]), ws) == K.E_ARG and ni.forward_raw(make(filter=3), ws) == K.E_ARG
    io = make()
    io.reserved[2] = 1
    assert ni.forward_raw(io, ws) == K.E_ARG
    io = make()
    io.pair.H = H - 2                                                       # not a multiple of 4
    assert ni.forward_raw(io, ws) == K.E_ARG
    io = make()
    io.pair.out_format = _fmt("i420", 8)
    assert ni.forward_raw(io, ws) == K.E_FORMAT
    io = make()
    io._keep_out[1].pitch[1] = W - 2
    assert ni.forward_raw(io, ws) == V.E_PITCH
    inside = (ws[4096:4096 + H * W].view(H, W), ws[1 << 20:(1 << 20) + H * W // 2].view(H // 2, W))       # an output inside the workspace
    io = ni.make_interlace_io(frames, tt, fmt, [out, inside], [0, 1], 1, True, None, H, W)
    assert ni.forward_raw(io, ws) == K.E_ARG
    io = make()
    io.pair.H, io.pair.W = 4, 8                                             # too small for the model: the code of the libraries below, passed through
    rc = ni.forward_raw(io, ws)
    assert -200 < rc < 0, rc
    torch.cuda.synchronize()
    assert all(bool((p == 0x44).all()) for p in out)


# ---- the stream ----------------------------------------------------------------------------------------------------------------------------
def _same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for n, (a, b) in enumerate(zip(got, want)):
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and np.array_equal(x, y), "%s, frame %d" % (what, n)


def _reference(nm, frames, layout, depth, in_rate, out_rate, tff, filt, scene=True):
    """By the contract: a fldr_rate.Converter at the doubled rate pushed the same frames; output frame k is the oracle's weave of its
    outputs 2k and 2k + 1.  -> a list of len(frames) + 1 lists of (frame, report) — the pushes, then the flush."""
    import fldr_rate as R
    from fractions import Fraction
    double = 2 * (Fraction(*out_rate) if isinstance(out_rate, tuple) else Fraction(out_rate))
    fields, cuts, calls, done = [], [], [], 0
    first = 0 if tff else 1

    def frame_of(k, second, held=0):
        pair = (fields[2 * k], second) if tff else (second, fields[2 * k])
        p = O.plan(k, in_rate, out_rate, tff)
        rep = {"frame": k, "input": p["input"], "r": p["r"], "cut": [cuts[2 * k], 0 if held else cuts[2 * k + 1]], "held": held, "reserved": [0, 0, 0]}
        if held:
            rep["input"], rep["r"] = [p["input"][0], len(frames) - 1], [p["r"][0], 0]
        return O.weave(pair[0], pair[1], layout, depth, filt), rep
    if nm is None:                                                          # no field is interpolated: field m is frame m A (B == 1)
        step = O.field_step(in_rate, out_rate)
        assert step.denominator == 1
        per_push = [[] for _ in frames] + [[]]
        m = 0
        for n in range(1, len(frames)):
            while m * step < n:
                per_push[n].append(frames[int(m * step)])
                m += 1
        if m * step == len(frames) - 1:
            per_push[len(frames)].append(frames[-1])
        cut_of = [0] * (len(frames) + 1)
    else:
        c = R.Converter(nm, CF.H, CF.W, _fmt(layout, depth), in_rate, double, scene=scene)
        per_push, cut_of = [], []
        for f in frames:
            per_push.append(c.push(f))
            cut_of.append(c.last_scene["cut"])
        per_push.append(c.flush())
        cut_of.append(0)
        c.close()
    for n, outs in enumerate(per_push):
        for o in outs:
            m = len(fields)
            r = O.plan(m >> 1, in_rate, out_rate, tff)["r"][m & 1]
            fields.append(o)
            cuts.append(1 if (r and cut_of[n]) else 0)
        call = []
        while 2 * done + 1 < len(fields):
            call.append(frame_of(done, fields[2 * done + 1]))
            done += 1
        calls.append(call)
    if len(fields) & 1:                                                     # the flush completes the last frame from the last pushed frame
        cuts.append(0)
        calls[-1].append(frame_of(done, frames[-1], held=1))
    return calls


def _check_stream(c, frames, want):
    for n, f in enumerate(frames):
        got = c.push(f)
        _same(got, [w for w, _ in want[n]], "push %d" % n)
        assert c.last_reports == [r for _, r in want[n]], (n, c.last_reports, [r for _, r in want[n]])
        for rep in c.last_reports:                                          # reports equal the library's plan
            p = c.plan(rep["frame"])
            assert p["push"] == n and (p["input"], p["r"]) == (rep["input"], rep["r"]), (n, p, rep)
    got = c.flush()
    _same(got, [w for w, _ in want[-1]], "flush")
    assert c.last_reports == [r for _, r in want[-1]], (c.last_reports, [r for _, r in want[-1]])
    assert c.flush() == [] and c.last_reports == []                         # a second flush returns none


STREAMS = [("24 -> 30i", 24, 30, "nv12", 8, True, O.LINEAR, 7),
           ("23.976 -> 29.97i bff", (24000, 1001), (30000, 1001), "i420", 10, False, O.COMPLEX, 6),
           ("25 -> 25i", 25, 25, "i420", 10, True, O.COMPLEX, 6),
           ("25 -> 25i bff", 25, 25, "nv12", 8, False, O.NONE, 6),
           ("60 -> 25i", 60, 25, "nv12", 8, True, O.LINEAR, 8),
           ("60 -> 25i bff", 60, 25, "i420", 10, False, O.NONE, 7)]


@pytest.mark.parametrize("name,in_rate,out_rate,layout,depth,tff,filt,n", STREAMS, ids=[s[0] for s in STREAMS])
def test_stream_equals_the_converter_at_the_doubled_rate_woven(nm, name, in_rate, out_rate, layout, depth, tff, filt, n):
    import fldr_interlace as K
    frames = CF.real_frames(layout, depth)[:n]
    assert 0 < CF.CUT_AT < n - 1                                            # one cut inside
    want = _reference(nm, frames, layout, depth, in_rate, out_rate, tff, filt)
    c = K.Interlacer(nm, CF.H, CF.W, _fmt(layout, depth), in_rate, out_rate, tff, filt)
    assert c.max_out == O.max_out(in_rate, out_rate)
    for f in frames[2:4]:                                                   # two frames of some other stream, forgotten by the reset
        c.push(f)
    c.reset()
    _check_stream(c, frames, want)
    c.close()
    counts = [len(w) for w in want[:-1]]
    reports = [r for call in want for _, r in call]
    assert [r["frame"] for r in reports] == list(range(len(reports)))
    if name.startswith("24") or name.startswith("23"):
        assert 2 in counts and counts[0] == 0                               # a push that returns two frames
        assert any(r["cut"] != [0, 0] for r in reports) and any(r["cut"] == [0, 0] for r in reports)      # the cut pair's fields are marked
    if name.startswith("25"):
        assert counts == [0] + [1] * (n - 1) and all(r["r"] == [0, 1] for r in reports if not r["held"])
    # a stream of n frames at these rates ends with a lone first field exactly where the brute-force schedule says so
    assert [r["held"] for _, r in want[-1]] == [int(h) for _, h in O.stream_frames(n, in_rate, out_rate)[-1]]


@pytest.mark.parametrize("layout,depth,tff,filt,n", [("i420", 10, True, O.LINEAR, 6), ("nv12", 8, False, O.COMPLEX, 7)])
def test_stream_50_to_25i_needs_no_model(dev, layout, depth, tff, filt, n):
    """B == 1: every field is an input frame's own rows.  No model, no workspace, no forward.  An odd number of frames leaves a lone first
    field, which the flush completes from the same frame: held."""
    import fldr_interlace as K
    frames = CF.real_frames(layout, depth)[:n]
    want = _reference(None, frames, layout, depth, 50, 25, tff, filt)
    c = K.Interlacer(None, CF.H, CF.W, _fmt(layout, depth), 50, 25, tff, filt, device=dev.index or 0)
    assert c.max_out == 1
    _check_stream(c, frames, want)
    assert [len(w) for w in want[:-1]] == [0, 0, 1, 0, 1, 0, 1][:n]
    assert [r["held"] for _, r in want[-1]] == ([1] if n % 2 else [0])
    # after a flush and a reset the object is a fresh stream
    c.reset()
    _check_stream(c, frames[:3], _reference(None, frames[:3], layout, depth, 50, 25, tff, filt))
    c.close()
