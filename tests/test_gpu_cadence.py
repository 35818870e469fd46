"""The cadence API (libfldr_cadence.so through fldr_cadence) on the GPU.  Every comparison is exact.  fldr_repeat_measure gives the
words of tests/cadence_oracle.py at every size, sample form and access form.  A cadence stream returns, byte for byte and in order,
what fldr_rate.Converter — which tests/test_gpu_rate.py holds to its schedule and forwards — returns at the derived rate on the
survivors the oracle chooses, and reports what the oracle reports.  The streams are tests/cadence_frames.py's; that their perturbed
repeats leave the first instance of every run as the survivors is asserted on the CPU (tests/test_cadence_cpu.py)."""
import numpy as np
import pytest
import torch

import cadence_frames as CF
import cadence_oracle as C

pytestmark = pytest.mark.gpu

FORMS = [("nv12", 8), ("nv12", 10), ("i420", 10)]                           # byte, P010 (word >> 8), yuv420p10le ((word & 0x3ff) >> 2)
SIZES = [(1, 1), (1, 37), (33, 1), (32, 32), (33, 65), (64, 64), (31, 257), (70, 130)]


def _fmt(layout, depth=8):
    import fldr_video
    return fldr_video.Format(layout, "bt709", "limited", depth)


# ---- fldr_repeat_measure -----------------------------------------------------------------------------------------------------------------
def _words(y8, layout, depth, g):
    """A luma plane whose y8 is the given array; at depth 10 the bits y8 ignores are noise."""
    if depth == 8:
        return y8.astype(np.uint8)
    y = y8.astype(np.uint16)
    if layout == "nv12":
        return (y << 8) | g.integers(0, 256, y.shape).astype(np.uint16)                           # the low two bits of the sample and the six below it
    return (y << 2) | g.integers(0, 4, y.shape).astype(np.uint16) | (g.integers(0, 64, y.shape).astype(np.uint16) << 10)


def _plane_to_dev(p, dev, access):
    """A device view of a host plane: "aligned" — address and pitch multiples of 16 bytes (the 16-byte loads); "offset" — the address one
    sample off and a pitch that is no multiple of 16 (the per-sample form).  The gap bytes are 0xA5."""
    r, c = p.shape
    b = p.dtype.itemsize
    pitch = (c * b + 15) // 16 * 16 + 16 + (0 if access == "aligned" else 3 * b)
    offset = 0 if access == "aligned" else b
    buf = torch.full((r * pitch + offset + 256,), 0xA5, dtype=torch.uint8, device=dev)
    view = buf[offset:offset + r * pitch].view(r, pitch)[:, :c * b]
    view.copy_(torch.from_numpy(np.ascontiguousarray(p).view(np.uint8).reshape(r, c * b)).to(dev))
    view = view.view(torch.uint16) if b == 2 else view
    if access == "aligned":
        assert view.data_ptr() % 16 == 0 and (view.stride(0) * b) % 16 == 0
    else:
        assert view.data_ptr() % 16 == b and (view.stride(0) * b) % 16 != 0
    return view


def _frame_to_dev(y, layout, depth, dev, access):
    """The luma plane in the given access form; the chroma planes are there to be checked, never read."""
    import fldr_video as V
    H, W = y.shape
    chroma = [torch.zeros(s, dtype=torch.uint16 if depth == 10 else torch.uint8, device=dev) for s in V.plane_shapes(layout, H, W)[1:]]
    return (_plane_to_dev(y, dev, access),) + tuple(chroma)


def _contents(H, W, seed):
    """[(name, y8 of I0, y8 of I1, tile_sad_min)] for one size: every content the measure is held to."""
    g = np.random.default_rng(seed)
    ty, tx = -(-H // 32), -(-W // 32)
    n_tiles = ty * tx
    base = g.integers(0, 256, (H, W))
    out = [("equal", base, base.copy(), 0)]
    one = np.clip(base, 0, 200)
    other = one.copy()
    other[H - 1, W - 1] += 55                                               # one sample, in the last (partial) tile
    out.append(("one sample in the last tile", one, other, 0))
    out.append(("one sample, threshold 55", one, other, 55))
    out.append(("one sample, threshold 56", one, other, 56))
    out.append(("black against white", np.zeros((H, W), np.int64), np.full((H, W), 255), 0))
    out.append(("noise", base, g.integers(0, 256, (H, W)), 0))
    out.append(("noise, threshold 1", base, g.integers(0, 256, (H, W)), 1))
    out.append(("noise, threshold 261120", base, g.integers(0, 256, (H, W)), 261120))
    if n_tiles >= 2:
        # two tiles with the same maximum, reached differently where the later tile has two samples: the lower index is reported
        a = np.full((H, W), 10)
        b = a.copy()
        first, last = (0, 0), ((ty - 1) * 32, (tx - 1) * 32)                # the first sample of tile 0 and of the last tile
        b[first] += 200
        if W - last[1] >= 2:
            b[last[0], last[1]] += 100
            b[last[0], last[1] + 1] += 100
        else:
            b[last] += 200
        out.append(("two equal maxima", a, b, 0))
        out.append(("two equal maxima, later first in memory order", b, a, 200))
        # a tile exactly at the threshold and one just below it
        c = a.copy()
        c[first] += 199
        c[last] += 200
        out.append(("at and below the threshold", a, c, 200))
    return out


@pytest.mark.parametrize("access", ["aligned", "offset"])
@pytest.mark.parametrize("layout,depth", FORMS)
@pytest.mark.parametrize("H,W", SIZES)
def test_measure_equals_the_oracle(dev, H, W, layout, depth, access):
    import fldr_cadence as K
    fmt = _fmt(layout, depth)
    g = np.random.default_rng(H * 1000 + W)
    st = K.repeat_state(dev)
    seen = set()
    for name, y0, y1, tmin in _contents(H, W, seed=H * W + depth):
        planes = [(_words(y, layout, depth, g),) for y in (y0, y1)]
        want = C.measure(planes[0], planes[1], (layout, depth), tmin)
        assert want == C.measure((y0.astype(np.uint8),), (y1.astype(np.uint8),), ("nv12", 8), tmin), name      # the ignored bits are ignored
        frames = [_frame_to_dev(p[0], layout, depth, dev, access) for p in planes]
        st.fill_(0xEE)                                                      # the state needs no preparation
        got = K.repeat_measure(frames, fmt, tmin or None, state=st)
        assert got == dict(want, reserved=[0, 0]), (name, got, want)
        seen.add(name)
        if name == "equal":
            assert got["sad"] == 0 and got["max_tile"] == 0 and got["repeat"] == 1
        elif name == "one sample in the last tile":
            assert got["sad"] == got["max_tile_sad"] == 55 and got["max_tile"] == -(-H // 32) * -(-W // 32) - 1 and got["repeat"] == 1
        elif name == "one sample, threshold 55":
            assert got["moving_tiles"] == 1 and got["repeat"] == 0
        elif name == "one sample, threshold 56":
            assert got["moving_tiles"] == 0 and got["repeat"] == 1
        elif name == "black against white":
            assert got["sad"] == 255 * H * W and got["max_tile_sad"] == 255 * min(H, 32) * min(W, 32) and got["max_tile"] == 0
        elif name.startswith("two equal maxima"):
            assert got["max_tile_sad"] == 200 and got["max_tile"] == 0 and got["sad"] == 400
        elif name == "at and below the threshold":
            assert got["moving_tiles"] == 1 and got["max_tile"] == -(-H // 32) * -(-W // 32) - 1 and got["max_tile_sad"] == 200
    assert len(seen) == (11 if -(-H // 32) * -(-W // 32) >= 2 else 8)


@pytest.mark.parametrize("layout,depth", FORMS)
def test_measure_is_repeatable_capturable_and_follows_rewritten_frames(dev, layout, depth):
    import fldr_cadence as K
    H, W = 70, 130
    fmt = _fmt(layout, depth)
    g = np.random.default_rng(depth)
    ys = [g.integers(0, 256, (H, W)) for _ in range(4)]
    planes = [_words(y, layout, depth, g) for y in ys]
    frames = [_frame_to_dev(p, layout, depth, dev, "aligned") for p in planes[:2]]
    want = C.measure((planes[0],), (planes[1],), (layout, depth))
    states = []
    for fill in (0x00, 0xFF, 0x5A):                                        # garbage left in the state beforehand changes nothing
        st = K.repeat_state(dev).fill_(fill)
        K.repeat_measure(frames, fmt, state=st, read=False)
        torch.cuda.synchronize()
        states.append(st.cpu().numpy().copy())
    st = K.repeat_state(dev).fill_(0x33)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        K.repeat_measure(frames, fmt, state=st, read=False)                # warm
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        K.repeat_measure(frames, fmt, state=st, read=False)
    for _ in range(2):
        st.fill_(0x77)
        graph.replay()
        torch.cuda.synchronize()
        states.append(st.cpu().numpy().copy())
    for b in states[1:]:
        assert np.array_equal(b, states[0])                                # all FLDR_REPEAT_STATE_BYTES, not only the result
    assert K.read_result(torch.from_numpy(states[0])) == dict(want, reserved=[0, 0])
    # the frames rewritten in place: a replay measures the new samples
    for f, p in zip(frames, planes[2:]):
        dst = f[0].view(torch.uint8) if depth == 10 else f[0]
        dst.copy_(torch.from_numpy(np.ascontiguousarray(p).view(np.uint8).reshape(H, -1)).to(dev))
    st.fill_(0x11)
    graph.replay()
    torch.cuda.synchronize()
    want2 = C.measure((planes[2],), (planes[3],), (layout, depth))
    assert want2 != want and K.read_result(st) == dict(want2, reserved=[0, 0])


def test_two_measures_in_flight_on_two_streams(dev):
    import fldr_cadence as K
    H, W = 270, 480
    fmt = _fmt("i420", 8)
    g = np.random.default_rng(3)
    pairs = [[g.integers(0, 256, (H, W)).astype(np.uint8) for _ in range(2)] for _ in range(2)]
    frames = [[_frame_to_dev(y, "i420", 8, dev, "aligned") for y in pr] for pr in pairs]
    want = [C.measure((pr[0],), (pr[1],), ("i420", 8)) for pr in pairs]
    assert want[0] != want[1]
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    states = [K.repeat_state(dev) for _ in range(2)]
    torch.cuda.synchronize()
    for rep in range(4):
        for k in range(2):
            with torch.cuda.stream(streams[k]):
                K.repeat_measure(frames[k], fmt, state=states[k], read=False)
    torch.cuda.synchronize()
    for k in range(2):
        assert K.read_result(states[k]) == dict(want[k], reserved=[0, 0]), k


# ---- the stream ----------------------------------------------------------------------------------------------------------------------------
CONTAINER_RATE = {"3:2": 60, "2:2": 50, "4+1": 30}                          # -> 24, 25, 24 after the drops


@pytest.fixture(scope="module")
def nm(dev):
    import fldr_harness as Hn
    import fldr_model
    m = fldr_model.NativeModel.from_npz(Hn.DEFAULT_WEIGHTS, device=dev.index or 0)
    yield m
    m.close()


def _reference(nm, frames, kept, layout, depth, rate, out_rate, scene):
    """fldr_rate.Converter at `rate` pushed frames[k] for k in kept, then flushed -> ([(outs, cut)] per push, the flush's outs)."""
    import fldr_rate as R
    c = R.Converter(nm, CF.H, CF.W, _fmt(layout, depth), rate, out_rate, scene=scene)
    pushes = []
    for k in kept:
        outs = c.push(frames[k])
        pushes.append((outs, c.last_scene["cut"]))
    tail = c.flush()
    c.close()
    return pushes, tail


def _same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for q, (a, b) in enumerate(zip(got, want)):
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and np.array_equal(x, y), "%s, output %d" % (what, q)


def _check_stream(nm, c, frames, layout, depth, in_rate, out_rate, cycle, drop, scene, tile_sad_min=0):
    """Push `frames` through the cadence stream `c` and flush; hold every call to the oracle's survivors pushed through a Converter at
    the derived rate.  -> the oracle's reports with the cut_mask filled in."""
    import fldr_cadence as K
    ms = CF.measures(frames, layout, depth, tile_sad_min)
    kept, reports = C.survivors(ms, cycle, drop)
    pushes, tail = _reference(nm, frames, kept, layout, depth, K.inner_rate(in_rate, cycle, drop), out_rate, scene)
    by_frame = dict(zip(kept, pushes))
    for rep in reports:
        mine = [rep["first_frame"] + k for k in range(rep["n_frames"]) if not rep["dropped_mask"] >> k & 1]
        rep["cut_mask"] = sum(by_frame[n][1] << q for q, n in enumerate(mine))
        rep["outs"] = [o for n in mine for o in by_frame[n][0]]
    for n, f in enumerate(frames):
        outs = c.push(f)
        if (n + 1) % cycle:
            assert outs == [] and c.last_report is None, n                   # a push inside a cycle returns nothing
        else:
            rep = reports[n // cycle]
            _same(outs, rep["outs"], "cycle %d" % (n // cycle))
            assert c.last_report == {k: v for k, v in rep.items() if k != "outs"}, (n, c.last_report, rep)
    outs = c.flush()
    if len(frames) % cycle:
        rep = reports[-1]
        _same(outs, rep["outs"] + tail, "flush")
        assert c.last_report == {k: v for k, v in rep.items() if k != "outs"}
    else:
        _same(outs, tail, "flush")
        assert c.last_report is None
    assert c.flush() == []                                                  # a second flush returns none
    return reports


@pytest.mark.parametrize("scene", [True, False])
@pytest.mark.parametrize("layout,depth", CF.FORMATS)
@pytest.mark.parametrize("out_rate", [60, 120])
@pytest.mark.parametrize("pattern", list(CF.PATTERNS))
def test_stream_equals_the_converter_on_the_survivors(nm, pattern, out_rate, layout, depth, scene):
    import fldr_cadence as K
    cycle, drop, _ = CF.PATTERNS[pattern]
    in_rate = CONTAINER_RATE[pattern]
    frames, source = CF.stream(pattern, layout, depth, 3 * cycle if cycle == 5 else 6 * cycle)
    c = K.Cadence(nm, CF.H, CF.W, _fmt(layout, depth), in_rate, out_rate, cycle, drop, scene=scene)
    inner_max = -(-out_rate // int(K.inner_rate(in_rate, cycle, drop)))
    assert c.max_out == (cycle - drop) * inner_max + 1
    reports = _check_stream(nm, c, frames, layout, depth, in_rate, out_rate, cycle, drop, scene)
    c.close()
    assert all(r["moving_dropped"] == 0 and r["still_kept"] == 0 for r in reports)
    dropped = [r["first_frame"] + k for r in reports for k in range(r["n_frames"]) if r["dropped_mask"] >> k & 1]
    assert dropped == [n for n, (_, inst) in enumerate(source) if inst]     # exactly the repeats went
    # the cut (real frame CUT_AT) is kept, and with the detector on the inner converter saw it as one
    cuts = [r["first_frame"] + [k for k in range(r["n_frames"]) if not r["dropped_mask"] >> k & 1][q]
            for r in reports for q in range(16) if r["cut_mask"] >> q & 1]
    assert cuts == ([n for n, s in enumerate(source) if s == (CF.CUT_AT, 0)] if scene else [])
    if pattern == "3:2" and scene:
        assert source[8] == (CF.CUT_AT, 0) and reports[1]["cut_mask"] == 0b10 and reports[1]["dropped_mask"] == 0b10110   # in mid-cycle


def test_cycle_1_drop_0_is_the_converter_push_for_push(nm):
    import fldr_cadence as K
    import fldr_rate as R
    layout, depth = "nv12", 8
    frames = CF.real_frames(layout, depth)[:6]
    c = K.Cadence(nm, CF.H, CF.W, _fmt(layout, depth), 24, 60, 1, 0, scene=True)
    r = R.Converter(nm, CF.H, CF.W, _fmt(layout, depth), 24, 60, scene=True)
    assert c.max_out == r.max_out + 1
    counts = []
    for n, f in enumerate(frames):
        got, want = c.push(f), r.push(f)
        _same(got, want, "push %d" % n)
        counts.append(len(got))
        rep = c.last_report
        assert rep["first_frame"] == n and rep["n_frames"] == 1 and rep["dropped_mask"] == 0 and rep["cut_mask"] == r.last_scene["cut"]
        assert rep["measure"] == [C.ZERO if n == 0 else C.measure(frames[n - 1], frames[n], (layout, depth))]
    assert counts == [0, 3, 2, 3, 2, 3]
    _same(c.flush(), r.flush(), "flush")
    c.close()
    r.close()


def test_partial_last_cycle_and_reset_in_mid_cycle(nm):
    import fldr_cadence as K
    layout, depth = "nv12", 8
    frames, source = CF.stream("3:2", layout, depth, 13)                    # two cycles and A A A of a third: one of the three goes
    c = K.Cadence(nm, CF.H, CF.W, _fmt(layout, depth), 60, 60, 5, 3, scene=True)
    for f in frames[3:6]:                                                   # three frames of some other stream, forgotten by the reset
        assert c.push(f) == []
    c.reset()
    reports = _check_stream(nm, c, frames, layout, depth, 60, 60, 5, 3, True)
    assert reports[-1]["n_frames"] == 3 and reports[-1]["dropped_mask"] in (0b010, 0b100) and reports[-1]["still_kept"] == 1
    # after a flush the object goes on; a reset makes it a fresh stream again
    c.reset()
    _check_stream(nm, c, frames[:10], layout, depth, 60, 60, 5, 3, True)
    c.close()


def test_static_stretch_and_wrong_declaration(nm):
    import fldr_cadence as K
    layout, depth = "nv12", 8
    still = [CF.real_frames(layout, depth)[0]] * 10                         # ten equal frames: every key is (0, 0)
    c = K.Cadence(nm, CF.H, CF.W, _fmt(layout, depth), 60, 60, 5, 3, scene=True)
    reports = _check_stream(nm, c, still, layout, depth, 60, 60, 5, 3, True)
    assert [r["dropped_mask"] for r in reports] == [0b01110, 0b00111]       # the lower frame numbers first; frame 0 of the stream never
    assert [r["still_kept"] for r in reports] == [1, 2] and all(r["moving_dropped"] == 0 for r in reports)
    # 2:2 content declared as 5, 3: moving frames are dropped, and the report says so
    frames, source = CF.stream("2:2", layout, depth, 10)
    c.reset()
    reports = _check_stream(nm, c, frames, layout, depth, 60, 60, 5, 3, True)
    assert sum(r["moving_dropped"] for r in reports) >= 1
    c.close()


def test_output_bytes_between_a_rows_end_and_its_pitch_are_untouched(nm):
    import fldr_cadence as K
    import fldr_video as V
    layout, depth = "i420", 10
    fmt = _fmt(layout, depth)
    frames, _ = CF.stream("3:2", layout, depth, 12)
    c = K.Cadence(nm, CF.H, CF.W, fmt, 60, 120, 5, 3, scene=True)
    pad = 24                                                                # samples
    bufs = [[np.full((r, w + pad), 0x5A5A, np.uint16) for r, w in V.plane_shapes(layout, CF.H, CF.W)] for _ in range(c.max_out)]
    c._outs = [tuple(b[:, :b.shape[1] - pad] for b in fr) for fr in bufs]  # the frames the library writes into: rows with a gap behind them
    for k, (st, fr) in enumerate(zip(c._out_structs(), bufs)):            # the library is really handed the padded frames
        for p, b in enumerate(fr):
            assert st.plane[p] == b.ctypes.data and st.pitch[p] == b.strides[0] == 2 * b.shape[1] > 2 * (b.shape[1] - pad), (k, p)
    ref = K.Cadence(nm, CF.H, CF.W, fmt, 60, 120, 5, 3, scene=True)
    total = 0
    for f in frames:
        got, want = c.push(f), ref.push(f)
        _same(got, want, "push")
        total += len(got)
    _same(c.flush(), ref.flush(), "flush")
    assert total == 15                                                      # two cycles: survivors 0, 3, 5, 8 at 24 -> 120
    for fr in bufs:
        for b in fr:
            assert (b[:, b.shape[1] - pad:] == 0x5A5A).all()
    c.close()
    ref.close()
