"""The pulldown API (libfldr_pulldown.so through fldr_pulldown) on the GPU.  Every comparison is exact.  fldr_pulldown_measure gives the
words of tests/pulldown_oracle.py at every size, anchor, sample form and access form; fldr_pulldown_assemble gives the oracle's bytes
and leaves pitch padding alone.  A pulldown stream returns, byte for byte and in order, what fldr_rate.Converter — which
tests/test_gpu_rate.py holds to its schedule and forwards — returns at the derived rate on the matched survivors the oracle chooses,
and reports what the oracle reports.  The streams are tests/pulldown_frames.py's; that their survivors are the film frames is asserted
on the CPU (tests/test_pulldown_cpu.py)."""
import numpy as np
import pytest
import torch

import pulldown_frames as PF
import pulldown_oracle as O

pytestmark = pytest.mark.gpu

FORMS = [("nv12", 8), ("nv12", 10), ("i420", 10)]                           # byte, P010 (word >> 8), yuv420p10le ((word & 0x3ff) >> 2)
SIZES = [(4, 1), (4, 33), (8, 32), (32, 32), (36, 65), (64, 64), (68, 130), (128, 257)]


def _fmt(layout, depth=8):
    import fldr_video
    return fldr_video.Format(layout, "bt709", "limited", depth)


def _words(y8, layout, depth, g):
    """A luma plane whose y8 is the given array; at depth 10 the bits y8 ignores are noise."""
    if depth == 8:
        return y8.astype(np.uint8)
    y = y8.astype(np.uint16)
    if layout == "nv12":
        return (y << 8) | g.integers(0, 256, y.shape).astype(np.uint16)
    return (y << 2) | g.integers(0, 4, y.shape).astype(np.uint16) | (g.integers(0, 64, y.shape).astype(np.uint16) << 10)


def _plane_to_dev(p, dev, access, fill=0xA5):
    """A device view of a host plane: "aligned" — address and pitch multiples of 16 bytes (the 16-byte accesses); "offset" — the address
    one sample off and a pitch that is no multiple of 16 (the per-sample form).  -> (view, the whole buffer, a mask of its row bytes)."""
    r, c = p.shape
    b = p.dtype.itemsize
    pitch = (c * b + 15) // 16 * 16 + 16 + (0 if access == "aligned" else 3 * b)
    offset = 0 if access == "aligned" else b
    buf = torch.full((r * pitch + offset + 256,), fill, dtype=torch.uint8, device=dev)
    view = buf[offset:offset + r * pitch].view(r, pitch)[:, :c * b]
    view.copy_(torch.from_numpy(np.ascontiguousarray(p).view(np.uint8).reshape(r, c * b)).to(dev))
    mask = np.zeros(buf.numel(), bool)
    mask[offset:offset + r * pitch].reshape(r, pitch)[:, :c * b] = True
    view = view.view(torch.uint16) if b == 2 else view
    if access == "aligned":
        assert view.data_ptr() % 16 == 0 and (view.stride(0) * b) % 16 == 0
    else:
        assert view.data_ptr() % 16 == b and (view.stride(0) * b) % 16 != 0
    return view, buf, mask


def _luma_frame(y, layout, depth, dev, access):
    """The luma plane in the given access form; the chroma planes are there to be checked, never read."""
    import fldr_video as V
    H, W = y.shape
    chroma = [torch.zeros(s, dtype=torch.uint16 if depth == 10 else torch.uint8, device=dev) for s in V.plane_shapes(layout, H, W)[1:]]
    return (_plane_to_dev(y, dev, access)[0],) + tuple(chroma)


def _columns(H, W, g):
    """A picture that is constant down every column: any two of its rows weave without combing."""
    return np.repeat(g.integers(0, 256, (1, W)), H, axis=0)


def _weave(anchor_src, other_src, q):
    o = anchor_src.copy()
    o[1 - q::2] = other_src[1 - q::2]
    return o


def _contents(H, W, q, seed):
    """[(name, y8 of cur, prev, next, params)] for one size and anchor: every content the measure is held to."""
    g = np.random.default_rng(seed)
    noise = lambda: g.integers(0, 256, (H, W))
    a, b, c = _columns(H, W, g), _columns(H, W, g), _columns(H, W, g)
    out = [("noise", noise(), noise(), noise(), {}),
           ("noise, other thresholds", noise(), noise(), noise(), {"comb_thresh": 40, "comb_tile_min": 3, "tile_sad_min": 700}),
           ("C wins", a, b, c, {}),
           ("P wins", _weave(a, b, q), _weave(c, a, q), c, {}),
           ("N wins", _weave(a, b, q), c, _weave(c, a, q), {}),
           ("all three equal", a, a.copy(), a.copy(), {})]
    base = noise()
    out.append(("all three equal noise", base, base.copy(), base.copy(), {}))
    rows = np.zeros((H, W), np.int64)
    rows[1 - q::2] = 255                                                    # the anchor rows 0, the others 255
    out.append(("alternating rows", rows, rows.copy(), rows.copy(), {}))
    flat = np.full((H, W), 100)
    step = lambda d: _weave(flat, flat + d, q)
    out.append(("differences of exactly comb_thresh", step(-6), step(6), step(7), {}))
    out.append(("alternating rows, comb_thresh 255", rows, rows.copy(), rows.copy(), {"comb_thresh": 255}))
    moved = flat.copy()
    moved[q::2, W - 1] += 37                                                # the anchor rows of prev differ in the last column
    out.append(("anchor rows differ", flat, moved, flat.copy(), {"tile_sad_min": 37 * len(range(q, min(H, 32), 2))}))
    return out


@pytest.mark.parametrize("access", ["aligned", "offset"])
@pytest.mark.parametrize("layout,depth", FORMS)
@pytest.mark.parametrize("q", [0, 1])
@pytest.mark.parametrize("H,W", SIZES)
def test_measure_equals_the_oracle(dev, H, W, q, layout, depth, access):
    import fldr_pulldown as K
    fmt = _fmt(layout, depth)
    g = np.random.default_rng(H * 1000 + W)
    st = K.measure_state(dev)
    for name, cur, prev, nxt, params in _contents(H, W, q, seed=H * W + depth + q):
        planes = [(_words(y, layout, depth, g),) for y in (cur, prev, nxt)]
        frames = [_luma_frame(p[0], layout, depth, dev, access) for p in planes]
        masks = range(1, 8) if name == "noise" else [7]
        for allowed in masks:
            want = O.measure(planes[0], planes[1], planes[2], (layout, depth), q, allowed=allowed, **params)
            eight = O.measure(*[(y.astype(np.uint8),) for y in (cur, prev, nxt)], ("nv12", 8), q, allowed=allowed, **params)
            assert want == eight, name                                       # the ignored bits are ignored
            st.fill_(0xEE)                                                  # the state needs no preparation
            got = K.measure(frames[0], frames[1], frames[2], fmt, q, K.Params(allowed=allowed, **params), state=st)
            assert got == dict(want, reserved=[0] * 5), (name, allowed, got, want)
        if name == "noise":
            # a candidate without a frame is not measured, and without prev nothing repeats
            for allowed, pr, nx in ((1, None, None), (5, None, 2), (3, 1, None)):
                want = O.measure(planes[0], None if pr is None else planes[1], None if nx is None else planes[2], (layout, depth), q, allowed=allowed)
                got = K.measure(frames[0], None if pr is None else frames[1], None if nx is None else frames[2], fmt, q, K.Params(allowed=allowed), state=st)
                assert got == dict(want, reserved=[0] * 5), (allowed, got, want)
                if pr is None:
                    assert got["dup_sad"] == got["dup_max_tile_sad"] == got["dup_max_tile"] == got["dup_moving_tiles"] == 0 and got["comb"][1] == 0
        elif name in ("C wins", "P wins", "N wins"):
            k = "CPN".index(name[0])
            assert got["comb"][k] == 0 and got["combed"] == 0, (name, got)
            if H >= 8 and W >= 32:                                          # enough samples that the other two certainly comb
                assert got["match"] == k and all(got["comb"][j] > 0 for j in range(3) if j != k), (name, got)
        elif name.startswith("all three equal"):
            assert got["match"] == 0 and len(set(got["comb"])) == 1 and got["dup_sad"] == 0
        elif name == "alternating rows":
            rows_in = lambda t: len([y for y in range(32 * t, min(32 * t + 32, H)) if y % 2 != q and 1 <= y <= H - 2])
            assert got["max_tile_comb"] == [max(rows_in(t) for t in range(-(-H // 32))) * min(W, 32)] * 3
            assert got["comb"] == [(H // 2 - 1) * W] * 3 and got["combed"] == int(got["max_tile_comb"][0] >= 32)
            if H >= 64 and W >= 32:
                assert got["max_tile_comb"][0] == 512
        elif name == "differences of exactly comb_thresh":
            assert got["comb"] == [0, 0, (H // 2 - 1) * W] and got["match"] == 0
        elif name == "alternating rows, comb_thresh 255":
            assert got["comb"] == [0, 0, 0] and got["combed"] == 0          # 255 x 255 is not above 255 x 255
        elif name == "anchor rows differ":
            anchors = [len(range(32 * t + q, min(32 * t + 32, H), 2)) for t in range(-(-H // 32))]
            assert got["dup_sad"] == 37 * (H // 2) and got["dup_max_tile_sad"] == 37 * anchors[0] and got["dup_max_tile"] == -(-W // 32) - 1
            assert got["dup_moving_tiles"] == sum(1 for n in anchors if n >= anchors[0])


@pytest.mark.parametrize("H,W,layout,depth", [(2160, 3840, "nv12", 8), (2160, 3840, "nv12", 10), (65600, 34, "nv12", 8), (32800, 70, "i420", 10)])
def test_measure_of_large_frames_luma_only(dev, H, W, layout, depth):
    """2160 x 3840, and two tall frames with more tile rows than the grid has walkers of them: the strided walk runs.  Only the luma
    planes exist: the chroma pointers name them again, to be checked and never read."""
    import fldr_pulldown as K
    import fldr_video as V
    g = np.random.default_rng(H + W + depth)
    ys = [g.integers(0, 256, (H, W)) for _ in range(3)]
    ys[1][0::2] = ys[0][0::2]                                              # prev: the anchor rows repeat, but for one sample in the last tile
    ys[1][H - 2, W - 1] ^= 0x40
    planes = [_words(y, layout, depth, g) for y in ys]
    frames = []
    for p in planes:
        t = torch.from_numpy(p.view(np.int16) if depth == 10 else p).to(dev)
        t = t.view(torch.uint16) if depth == 10 else t
        frames.append((t,) * len(V.plane_shapes(layout, H, W)))
    want = O.measure((planes[0],), (planes[1],), (planes[2],), (layout, depth), 0)
    fr = [V.frame_struct(f) for f in frames]
    st = K.measure_state(dev)
    import ctypes
    assert K.measure_raw(H, W, _fmt(layout, depth), fr[0], fr[1], fr[2], 0, None, ctypes.c_void_p(st.data_ptr()), V._stream_ptr(dev, None)) == 0
    got = K.read_result(st)
    assert got == dict(want, reserved=[0] * 5)
    assert got["dup_sad"] == 0x40 and got["dup_max_tile"] == -(-H // 32) * -(-W // 32) - 1


# ---- fldr_pulldown_assemble -------------------------------------------------------------------------------------------------------------
ALL_FORMATS = [("nv12", 8), ("nv12", 10), ("i420", 8), ("i420", 10)]


def _noise_frame(layout, depth, H, W, g):
    import fldr_video as V
    out = []
    for s in V.plane_shapes(layout, H, W):
        if depth == 8:
            out.append(g.integers(0, 256, s).astype(np.uint8))
        elif layout == "nv12":
            out.append((g.integers(0, 1024, s) << 6 | g.integers(0, 64, s)).astype(np.uint16))     # P010 with noise in the low six bits
        else:
            out.append(g.integers(0, 1024, s).astype(np.uint16))
    return tuple(out)


@pytest.mark.parametrize("access", ["aligned", "offset"])
@pytest.mark.parametrize("layout,depth", ALL_FORMATS)
@pytest.mark.parametrize("H,W", [(4, 1), (36, 65), (68, 130), (4, 70001), (2052, 3)])
def test_assemble_equals_the_oracle_and_leaves_padding_alone(dev, H, W, layout, depth, access):
    """(4, 70001) has rows longer than the grid's walkers of a row cover at once, (2052, 3) more rows than its walkers of the rows."""
    import fldr_pulldown as K
    fmt = _fmt(layout, depth)
    g = np.random.default_rng(H * 7 + W + depth)
    host = [_noise_frame(layout, depth, H, W, g) for _ in range(3)]
    devs = [tuple(_plane_to_dev(p, dev, access)[0] for p in f) for f in host]
    decision = torch.zeros(64, dtype=torch.int32, device=dev)
    for q in (0, 1):
        for post in (K.POST_KEEP, K.POST_AVERAGE):
            for combed in (0, 1):
                for match in (0, 1, 2):
                    for from_device in (False, True):
                        want = O.assemble(host[0], host[1], host[2], (layout, depth), q, match, combed, post)
                        outs = [_plane_to_dev(np.zeros_like(p), dev, access, fill=0x5A) for p in host[0]]
                        for _, buf, _ in outs:
                            buf.fill_(0x5A)
                        out = tuple(o[0] for o in outs)
                        if from_device:
                            decision[:2] = torch.tensor([match, 5 * combed], dtype=torch.int32)       # any non-zero word is "combed"
                            K.assemble(devs[0], devs[1], devs[2], out, fmt, q, -1, 1 - combed, decision, post)
                        else:
                            K.assemble(devs[0], devs[1] if match == 1 else None, devs[2] if match == 2 else None, out, fmt, q, match, 3 * combed, None, post)
                        torch.cuda.synchronize()
                        what = (q, post, combed, match, from_device)
                        for p, (view, buf, mask) in enumerate(outs):
                            got = (view.view(torch.int16) if depth == 10 else view).cpu().numpy()
                            got = got.view(np.uint16) if depth == 10 else got
                            assert np.array_equal(got, want[p]), (what, p)
                            assert (buf.cpu().numpy()[~mask] == 0x5A).all(), (what, p)       # the gaps and the bytes around the plane
    if (H, W) == (36, 65):
        # P010: a kept row carries the low six bits along, an averaged row is canonical
        if (layout, depth) == ("nv12", 10):
            kept = O.assemble(host[0], host[1], host[2], (layout, depth), 0, 1, 1, K.POST_KEEP)
            avg = O.assemble(host[0], host[1], host[2], (layout, depth), 0, 1, 1, K.POST_AVERAGE)
            assert (kept[0][1::2] & 63).any() and not (avg[0][1::2] & 63).any() and np.array_equal(avg[0][0::2], host[0][0][0::2])


def test_assemble_with_a_device_word_outside_the_candidates_takes_cur(dev):
    import fldr_pulldown as K
    g = np.random.default_rng(9)
    host = [_noise_frame("i420", 8, 8, 40, g) for _ in range(3)]
    devs = [tuple(torch.from_numpy(p).to(dev) for p in f) for f in host]
    out = tuple(torch.zeros_like(p) for p in devs[0])
    for word in (3, -1, 2 ** 31 - 1):
        decision = torch.tensor([word, 0], dtype=torch.int32, device=dev)
        K.assemble(devs[0], None, None, out, _fmt("i420", 8), 0, -1, 0, decision)
        torch.cuda.synchronize()
        assert all(np.array_equal(o.cpu().numpy(), p) for o, p in zip(out, host[0])), word


# ---- graphs and streams ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,depth", FORMS)
def test_measure_and_assemble_captured_once_follow_rewritten_frames(dev, layout, depth):
    """One capture of measure + assemble on one stream, no parallel branches: the assembly reads the decision on the device, so a replay
    follows the frames as they are rewritten — each of C, P and N in turn."""
    import fldr_pulldown as K
    H, W, q = 68, 130, 0
    fmt = _fmt(layout, depth)
    g = np.random.default_rng(depth)
    pics = [_noise_frame(layout, depth, H, W, g) for _ in range(3)]
    col = lambda k: tuple(np.repeat(p[:1], p.shape[0], axis=0) for p in pics[k])        # constant down every column
    a, b, c = col(0), col(1), col(2)
    weave = lambda x, y: tuple(_weave(px, py, q) for px, py in zip(x, y))
    cases = [(a, b, c, 0), (weave(a, b), weave(c, a), c, 1), (weave(a, b), c, weave(c, a), 2), (weave(a, b), b, c, None)]
    devs = [tuple(_plane_to_dev(p, dev, "aligned")[0] for p in f) for f in cases[0][:3]]
    out = tuple(_plane_to_dev(np.zeros_like(p), dev, "aligned")[0] for p in a)
    st = K.measure_state(dev).fill_(0x33)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())

    def enqueue():
        K.measure(devs[0], devs[1], devs[2], fmt, q, state=st, read=False)
        K.assemble(devs[0], devs[1], devs[2], out, fmt, q, -1, 0, st, K.POST_AVERAGE)
    with torch.cuda.stream(s):
        enqueue()                                                           # warm
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        enqueue()
    states = []
    for cur, prev, nxt, winner in cases + cases[:1]:
        for d, f in zip(devs, (cur, prev, nxt)):
            for t, p in zip(d, f):
                (t.view(torch.uint8) if depth == 10 else t).copy_(torch.from_numpy(np.ascontiguousarray(p).view(np.uint8).reshape(p.shape[0], -1)).to(dev))
        st.fill_(0x77)
        graph.replay()
        torch.cuda.synchronize()
        want = O.measure(cur, prev, nxt, (layout, depth), q)
        got = K.read_result(st)
        assert got == dict(want, reserved=[0] * 5)
        if winner is None:
            assert got["combed"] == 1                                       # every candidate combs: the line average is written
        else:
            assert got["match"] == winner and got["combed"] == 0
        frame = O.assemble(cur, prev, nxt, (layout, depth), q, want["match"], want["combed"], O.AVERAGE)
        for o, w in zip(out, frame):
            got_p = (o.view(torch.int16) if depth == 10 else o).cpu().numpy()
            assert np.array_equal(got_p.view(np.uint16) if depth == 10 else got_p, w)
        states.append(st.cpu().numpy().copy())
    assert np.array_equal(states[0], states[-1])                            # all FLDR_PULLDOWN_STATE_BYTES, not only the result


def test_two_measures_in_flight_on_two_streams(dev):
    import fldr_pulldown as K
    H, W = 272, 480
    fmt = _fmt("i420", 8)
    g = np.random.default_rng(3)
    sets = [[g.integers(0, 256, (H, W)).astype(np.uint8) for _ in range(3)] for _ in range(2)]
    frames = [[_luma_frame(y, "i420", 8, dev, "aligned") for y in s] for s in sets]
    want = [O.measure((s[0],), (s[1],), (s[2],), ("i420", 8), k) for k, s in enumerate(sets)]
    assert want[0] != want[1]
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    states = [K.measure_state(dev) for _ in range(2)]
    torch.cuda.synchronize()
    for rep in range(4):
        for k in range(2):
            with torch.cuda.stream(streams[k]):
                K.measure(frames[k][0], frames[k][1], frames[k][2], fmt, k, state=states[k], read=False)
    torch.cuda.synchronize()
    for k in range(2):
        assert K.read_result(states[k]) == dict(want[k], reserved=[0] * 5), k


# ---- the stream ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nm(dev):
    import fldr_harness as Hn
    import fldr_model
    m = fldr_model.NativeModel.from_npz(Hn.DEFAULT_WEIGHTS, device=dev.index or 0)
    yield m
    m.close()


def _reference(nm, survivors, layout, depth, rate, out_rate, scene=True):
    """fldr_rate.Converter at `rate` pushed the frames `survivors`, then flushed -> ([(outs, cut)] per push, the flush's outs)."""
    import fldr_rate as R
    c = R.Converter(nm, PF.H, PF.W, _fmt(layout, depth), rate, out_rate, scene=scene)
    pushes = []
    for f in survivors:
        outs = c.push(f)
        pushes.append((outs, c.last_scene["cut"]))
    tail = c.flush()
    c.close()
    return pushes, tail


def _same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for n, (a, b) in enumerate(zip(got, want)):
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and np.array_equal(x, y), "%s, output %d" % (what, n)


def _check_stream(nm, c, frames, layout, depth, spec, post=O.KEEP):
    """Push `frames` through the pulldown stream `c` and flush; hold every call to the oracle's matched survivors pushed through a
    Converter at the derived rate.  -> (the oracle's reports with the cut_mask filled in, the kept frame numbers, the matched frames)."""
    cycle, drop = spec["cycle"], spec["drop"]
    results, matched = O.match_stream(frames, (layout, depth), spec["anchor"], post)
    kept, reports = O.survivors(results, cycle, drop)
    pushes, tail = _reference(nm, [matched[k] for k in kept], layout, depth, O.inner_rate(spec["in_rate"], cycle, drop), spec["out_rate"])
    by_frame = dict(zip(kept, pushes))
    for rep in reports:
        mine = [rep["first_frame"] + k for k in range(rep["n_frames"]) if not rep["dropped_mask"] >> k & 1]
        rep["cut_mask"] = sum(by_frame[n][1] << i for i, n in enumerate(mine))
        rep["outs"] = [o for n in mine for o in by_frame[n][0]]
    strip = lambda rep: {k: v for k, v in rep.items() if k != "outs"}
    for n, f in enumerate(frames):
        outs = c.push(f)
        if n == 0 or n % cycle:
            assert outs == [] and c.last_report is None, n                   # a push that completes no cycle returns nothing
        else:
            rep = reports[n // cycle - 1]
            _same(outs, rep["outs"], "cycle %d" % (n // cycle - 1))
            assert c.last_report == strip(rep), (n, c.last_report, strip(rep))
    outs = c.flush()
    rep = reports[-1]                                                       # the flush always ends a cycle: the last frame is matched there
    _same(outs, rep["outs"] + tail, "flush")
    assert c.last_report == strip(rep), (c.last_report, strip(rep))
    assert c.flush() == [] and c.last_report is None                        # a second flush returns none
    return reports, kept, matched


@pytest.mark.parametrize("layout,depth", PF.FORMATS)
@pytest.mark.parametrize("name", ["3:2 tff", "3:2 bff", "2:2 shifted", "3:2 tff perturbed"])
def test_stream_equals_the_converter_on_the_matched_survivors(nm, name, layout, depth):
    import fldr_pulldown as K
    frames, film, spec = PF.stream(name, layout, depth)
    c = K.Pulldown(nm, PF.H, PF.W, _fmt(layout, depth), spec["in_rate"], spec["out_rate"], spec["cycle"], spec["drop"], spec["anchor"])
    inner = K.inner_rate(spec["in_rate"], spec["cycle"], spec["drop"])
    assert inner == {"3": 24, "2": 25}[name[0]] and c.max_out == (spec["cycle"] - spec["drop"]) * -(-spec["out_rate"] // int(inner)) + 1
    reports, kept, matched = _check_stream(nm, c, frames, layout, depth, spec)
    c.close()
    assert len(kept) == len(film)
    if not name.endswith("perturbed"):
        assert all(np.array_equal(a, b) for k, f in zip(kept, film) for a, b in zip(matched[k], f))      # the film, exactly and in order
    assert all(r["combed_mask"] == 0 and r["moving_dropped"] == 0 for r in reports)
    assert [r["still_kept"] for r in reports] == ([0, 0] if name.startswith("3:2") else [0] * 6 + [1])      # 2:2: the film holds its last frame
    if name.startswith("3:2"):
        want = [0, 0, 2, 2, 0] if "bff" in name else [0, 0, 1, 1, 0]
        assert [r["match"] for r in reports] == [want, want] and [r["dropped_mask"] for r in reports] == ([0b10000] * 2 if "bff" in name else [0b00100] * 2)
        assert [r["cut_mask"] for r in reports] == [0b1000, 0]              # film frame 3 begins the second scene: the first cycle's fourth survivor
    else:
        assert [m for r in reports for m in r["match"]] == [0, 2, 2, 2, 2, 2, 0] and sum(r["cut_mask"] for r in reports) == 1


def test_cycle_1_drop_0_on_progressive_frames_is_the_converter_one_frame_late(nm):
    import fldr_pulldown as K
    import fldr_rate as R
    layout, depth = "nv12", 8
    frames = PF.progressive(layout, depth)
    c = K.Pulldown(nm, PF.H, PF.W, _fmt(layout, depth), 24, 60, 1, 0)
    r = R.Converter(nm, PF.H, PF.W, _fmt(layout, depth), 24, 60, scene=True)
    assert c.max_out == r.max_out + 1
    want = [r.push(f) for f in frames]
    assert c.push(frames[0]) == [] and c.last_report is None
    for n, f in enumerate(frames[1:]):
        _same(c.push(f), want[n], "push %d" % (n + 1))                      # the outputs of the converter's push n, at push n + 1
        rep = c.last_report
        assert rep["first_frame"] == n and rep["n_frames"] == 1 and rep["dropped_mask"] == 0 and rep["match"] == [0] and rep["combed_mask"] == 0
    _same(c.flush(), want[-1] + r.flush(), "flush")
    assert c.last_report["first_frame"] == len(frames) - 1
    c.close()
    r.close()


def test_partial_last_cycle_and_reset_in_mid_cycle(nm):
    import fldr_pulldown as K
    layout, depth = "nv12", 8
    frames, film, spec = PF.stream("3:2 tff", layout, depth)
    c = K.Pulldown(nm, PF.H, PF.W, _fmt(layout, depth), spec["in_rate"], spec["out_rate"], 5, 1, 0)
    for f in frames[3:6]:                                                   # three frames of some other stream, forgotten by the reset
        assert c.push(f) == []
    c.reset()
    reports, kept, _ = _check_stream(nm, c, frames[:7], layout, depth, spec)            # a cycle and two frames: floor(2 x 1 / 5) = 0 go
    assert [r["n_frames"] for r in reports] == [5, 2] and reports[1]["dropped_mask"] == 0 and kept == [0, 1, 3, 4, 5, 6]
    # after a flush the object goes on with a new stream; a reset makes it a fresh one again
    c.reset()
    _check_stream(nm, c, frames[:5], layout, depth, spec)
    c.close()


@pytest.mark.parametrize("layout,depth", PF.FORMATS)
def test_true_video_among_film_falls_back_to_the_line_average(nm, layout, depth):
    import fldr_pulldown as K
    frames, film, spec = PF.stream("video insert", layout, depth)
    c = K.Pulldown(nm, PF.H, PF.W, _fmt(layout, depth), spec["in_rate"], spec["out_rate"], 1, 0, 0, K.POST_AVERAGE)
    reports, kept, matched = _check_stream(nm, c, frames, layout, depth, spec, O.AVERAGE)
    c.close()
    assert kept == list(range(len(frames)))
    assert [r["combed_mask"] for r in reports] == [0, 0, 0, 1, 1, 1, 1, 0, 0, 0]
    for n, (m, f) in enumerate(zip(matched, film)):
        if reports[n]["combed_mask"]:
            assert all(np.array_equal(a[0::2], b[0::2]) and not np.array_equal(a, b) for a, b in zip(m, f))      # the anchor field kept, the other rebuilt
        else:
            assert all(np.array_equal(a, b) for a, b in zip(m, f))
