"""The probe API (libfldr_probe.so through fldr_probe) on the GPU.  Every comparison is exact.  fldr_probe_measure gives the words of
tests/probe_oracle.py at every size, sample form and access form, with either neighbour missing, at the largest per-tile words and at
the ends of the thresholds' ranges, and never writes a frame; its comb and field words are fldr_pulldown_measure's at both anchors on
the same device frames; two runs and a graph replay give the same state.  A probe stream holds the oracle's per-frame results and gives
the verdict tests/test_probe_cpu.py asserts of every stream of tests/probe_frames.py."""
import numpy as np
import pytest
import torch

import probe_frames as F
import probe_oracle as O
from test_gpu_pulldown import _fmt, _plane_to_dev, _words

pytestmark = pytest.mark.gpu

FORMS = [("nv12", 8), ("nv12", 10), ("i420", 8), ("i420", 10)]             # NV12, P010 with dirty low bits, I420, yuv420p10le with junk high bits
SIZES = [(4, 1), (4, 33), (8, 31), (36, 32), (64, 64), (68, 97)]
ZERO_RESERVED = [0] * 12


def _frame(y, layout, depth, dev, access):
    """The luma plane in the given access form, its whole buffer and row mask; the chroma planes are there to be checked, never read."""
    import fldr_video as V
    H, W = y.shape
    chroma = [torch.zeros(s, dtype=torch.uint16 if depth == 10 else torch.uint8, device=dev) for s in V.plane_shapes(layout, H, W)[1:]]
    view, buf, _ = _plane_to_dev(y, dev, access)
    return (view,) + tuple(chroma), buf


def _contents(H, W, seed):
    """[(name, y8 of cur, prev, next, params)] for one size: every content the measure is held to."""
    g = np.random.default_rng(seed)
    noise = lambda: g.integers(0, 256, (H, W))
    rows = np.zeros((H, W), np.int64)
    rows[1::2] = 255
    flat = np.full((H, W), 100)
    near = noise()
    return [("noise", noise(), noise(), noise(), {}),
            ("noise, low thresholds", noise(), noise(), noise(), {"comb_thresh": 1, "comb_tile_min": 1, "tile_sad_min": 1, "frame_tile_sad_min": 1}),
            ("noise, high thresholds", noise(), noise(), noise(), {"comb_thresh": 255, "comb_tile_min": 512, "tile_sad_min": 130560,
                                                                    "frame_tile_sad_min": 261120}),
            ("near", near, np.clip(near + g.integers(-3, 4, (H, W)), 0, 255), np.clip(near + g.integers(-9, 10, (H, W)), 0, 255),
             {"comb_thresh": 40, "tile_sad_min": 700, "frame_tile_sad_min": 1500}),
            ("alternating rows", rows, 255 - rows, rows.copy(), {}),
            ("one code apart", flat, flat + 1, flat - 1, {"tile_sad_min": 512, "frame_tile_sad_min": 1024}),
            ("black and white", np.zeros((H, W), np.int64), np.full((H, W), 255), np.full((H, W), 255), {})]


def _check_words(name, got, H, W):
    """What the contents are made for, worked out by hand: the largest per-tile words and the order sums."""
    if name == "alternating rows":
        # cur combs against itself everywhere; prev, its inverse, lies on the lines around every row: the largest words of a tile
        inner = lambda par: [len([y for y in range(32 * t, min(32 * t + 32, H)) if y % 2 == par and 1 <= y <= H - 2]) for t in range(-(-H // 32))]
        for q in (0, 1):
            assert got["max_tile_comb"][q] == [max(inner(1 - q)) * min(W, 32), 0, max(inner(1 - q)) * min(W, 32)]
            assert got["field_max_tile_sad"][q] == min(16, H // 2) * min(W, 32) * 255
        assert got["lap"][0] == [sum(inner(0)) * W * 510, sum(inner(1)) * W * 510] and got["lap"][1] == [0, 0]
        if H >= 64 and W >= 32:
            assert got["max_tile_comb"][0][0] == 512 and got["field_max_tile_sad"] == [130560, 130560]
    elif name == "one code apart":
        assert got["comb"] == [[0] * 3, [0] * 3] and got["field_sad"] == [H // 2 * W, H // 2 * W] and got["lap"][0] == [0, 0]
        assert got["lap"][1] == got["lap"][2] == [2 * (H // 2 - 1) * W] * 2 and got["tff_sum"] == got["bff_sum"]
        full = (H // 32) * (W // 32)                                       # whole tiles: 512 per field, 1024 together
        assert got["field_moving_tiles"] == [full, full] and got["frame_moving_tiles"] == full
    elif name == "black and white":
        assert got["lap"][1] == got["lap"][2] == [(H // 2 - 1) * W * 510] * 2 and sum(got["field_sad"]) == H * W * 255
        if H % 32 == 0 and W % 32 == 0:                                     # whole tiles only: a 4 x 1 corner tile sums to 1020
            assert got["frame_moving_tiles"] == (-(-H // 32)) * (-(-W // 32)) and got["field_max_tile_sad"] == [130560, 130560]


@pytest.mark.parametrize("access", ["aligned", "offset"])
@pytest.mark.parametrize("layout,depth", FORMS)
@pytest.mark.parametrize("H,W", SIZES)
def test_measure_equals_the_oracle_and_writes_no_frame(dev, H, W, layout, depth, access):
    import fldr_probe as K
    fmt = _fmt(layout, depth)
    g = np.random.default_rng(H * 1000 + W)
    st = K.measure_state(dev)
    for name, cur, prev, nxt, params in _contents(H, W, seed=H * W + depth):
        planes = [(_words(y, layout, depth, g),) for y in (cur, prev, nxt)]
        made = [_frame(p[0], layout, depth, dev, access) for p in planes]
        frames, before = [m[0] for m in made], [m[1].cpu().numpy().copy() for m in made]
        want = O.measure(planes[0], planes[1], planes[2], (layout, depth), **params)
        eight = O.measure(*[(y.astype(np.uint8),) for y in (cur, prev, nxt)], ("nv12", 8), **params)
        assert want == eight, name                                           # the ignored bits are ignored
        st.fill_(0xEE)                                                      # the state needs no preparation
        got = K.measure(frames[0], frames[1], frames[2], fmt, K.Params(**params), state=st)
        assert got == dict(want, reserved=ZERO_RESERVED), (name, got, want)
        if name == "noise":
            for pr, nx in ((None, None), (None, 2), (1, None)):              # a frame that is NULL is not measured: its words are 0
                want = O.measure(planes[0], None if pr is None else planes[1], None if nx is None else planes[2], (layout, depth))
                st.fill_(0x11)
                got = K.measure(frames[0], None if pr is None else frames[1], None if nx is None else frames[2], fmt, state=st)
                assert got == dict(want, reserved=ZERO_RESERVED), (pr, nx, got, want)
                assert got["tff_sum"] == got["bff_sum"] == 0 and (pr is not None or got["repeat"] == got["field_sad"][0] == got["lap"][1][0] == 0)
        else:
            _check_words(name, got, H, W)
        for m, b in zip(made, before):
            assert np.array_equal(m[1].cpu().numpy(), b), name                 # the frames and their padding are never written


@pytest.fixture(scope="module")
def stream_frames(dev):
    """Three consecutive 256 x 448 frames of a stream in every format on the device, with the oracle's result: shared, never written."""
    cache = {}

    def get(name, layout, depth, n=2):
        key = (name, layout, depth, n)
        if key not in cache:
            frames, _ = F.stream(name, layout, depth)
            host = frames[n - 1:n + 2]
            devs = [tuple(torch.from_numpy(np.ascontiguousarray(p).view(np.int16) if depth == 10 else np.ascontiguousarray(p)).to(dev) for p in f) for f in host]
            devs = [tuple(p.view(torch.uint16) if depth == 10 else p for p in f) for f in devs]
            cache[key] = (host, devs, O.measure(host[1], host[0], host[2], (layout, depth)))
        return cache[key]
    return get


@pytest.mark.parametrize("layout,depth", F.FORMATS)
@pytest.mark.parametrize("name", ["3:2 tff", "video bff", "repeats 3:2"])
def test_measure_of_stream_frames_equals_the_oracle_and_the_pulldown_measure_at_both_anchors(dev, stream_frames, name, layout, depth):
    import fldr_probe as K
    import fldr_pulldown as PD
    fmt = _fmt(layout, depth)
    host, devs, want = stream_frames(name, layout, depth)
    assert host[0][0].shape == (F.H, F.W) == (256, 448)
    st = K.measure_state(dev).fill_(0x5A)
    got = K.measure(devs[1], devs[0], devs[2], fmt, state=st)
    assert got == dict(want, reserved=ZERO_RESERVED)
    first = st.cpu().numpy().copy()
    st.fill_(0xC3)
    assert K.measure(devs[1], devs[0], devs[2], fmt, state=st) == got and np.array_equal(st.cpu().numpy(), first)     # two runs, identical states
    for q in (0, 1):
        p = PD.measure(devs[1], devs[0], devs[2], fmt, q)
        assert (got["comb"][q], got["max_tile_comb"][q], got["max_tile"][q]) == (p["comb"], p["max_tile_comb"], p["max_tile"]), q
        assert (got["field_sad"][q], got["field_max_tile_sad"][q], got["field_max_tile"][q], got["field_moving_tiles"][q]) == \
               (p["dup_sad"], p["dup_max_tile_sad"], p["dup_max_tile"], p["dup_moving_tiles"]), q


def test_measure_captured_once_follows_rewritten_frames(dev):
    import fldr_probe as K
    H, W, layout, depth = 68, 97, "nv12", 10
    fmt = _fmt(layout, depth)
    g = np.random.default_rng(11)
    sets = [[(_words(g.integers(0, 256, (H, W)), layout, depth, g),) for _ in range(3)] for _ in range(3)]
    made = [_frame(p[0], layout, depth, dev, "aligned") for p in sets[0]]
    devs = [m[0] for m in made]
    st = K.measure_state(dev).fill_(0x33)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        K.measure(devs[0], devs[1], devs[2], fmt, state=st, read=False)     # warm
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        K.measure(devs[0], devs[1], devs[2], fmt, state=st, read=False)
    states = []
    for planes in sets + sets[:1]:
        for d, p in zip(devs, planes):
            d[0].view(torch.uint8).copy_(torch.from_numpy(np.ascontiguousarray(p[0]).view(np.uint8).reshape(H, -1)).to(dev))
        st.fill_(0x77)
        graph.replay()
        torch.cuda.synchronize()
        assert K.read_result(st) == dict(O.measure(planes[0], planes[1], planes[2], (layout, depth)), reserved=ZERO_RESERVED)
        states.append(st.cpu().numpy().copy())
    assert np.array_equal(states[0], states[-1])                            # all FLDR_PROBE_STATE_BYTES, not only the result


# ---- the stream ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,depth", F.FORMATS)
@pytest.mark.parametrize("name", F.STREAMS)
def test_stream_holds_the_oracles_results_and_gives_the_expected_verdict(dev, name, layout, depth):
    import fldr_probe as K
    frames, want = F.stream(name, layout, depth)
    results = O.measure_stream(frames, (layout, depth))
    p = K.Probe(F.H, F.W, _fmt(layout, depth), window=16, device=dev.index or 0)
    for f in frames:
        p.push(f)
    v = p.verdict()
    assert v == O.classify(results) and {k: v[k] for k in want} == want, v
    assert p.results() == [(n + 1, r) for n, r in enumerate(results)]
    p.close()


def test_stream_before_enough_frames_after_reset_and_with_a_small_window(dev):
    import fldr_probe as K
    layout, depth = "nv12", 8
    frames, want = F.stream("repeats 4+1", layout, depth)
    results = O.measure_stream(frames, (layout, depth))
    p = K.Probe(F.H, F.W, _fmt(layout, depth), window=9, device=dev.index or 0)
    assert p.verdict() == O.classify([]) and p.results() == []
    for n, f in enumerate(frames[:4]):                                      # nothing is measured before the third frame
        p.push(f)
        assert p.verdict() == O.classify(results[:max(n - 1, 0)]) and p.verdict()["kind"] == K.UNKNOWN
    assert [r[0] for r in p.results()] == [1, 2]
    for f in frames[4:]:
        p.push(f)
    # a window smaller than the stream: the last nine results, oldest first, and the verdict on those alone (both repeats: one confirmed)
    assert len(results) == 12 and p.results() == [(n + 1, r) for n, r in enumerate(results)][-9:]
    v = p.verdict()
    assert v == O.classify(results[-9:]) and (v["kind"], v["cycle"], v["drop"], v["confirmed"], v["n_frames"]) == (K.PROGRESSIVE, 5, 1, 1, 9)
    p.reset()
    assert p.verdict() == O.classify([]) and p.results() == []
    video, _ = F.stream("video bff", layout, depth)                           # the next push is frame 0 of a new stream
    for f in video:
        p.push(f)
    assert p.results() == [(n + 1, r) for n, r in enumerate(O.measure_stream(video, (layout, depth)))]
    assert (p.verdict()["kind"], p.verdict()["tff"]) == (K.INTERLACED, 0)
    p.close()
