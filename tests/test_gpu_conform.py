"""The conform API (libfldr_conform.so through fldr_conform) on the GPU.  Every comparison is exact, byte for byte, against
tests/conform_oracle.py: fldr_conform_frame over all 256 format pairs, at the sizes around the kernel's lane run and workgroup, with planes
on and off a 16-byte boundary, over every code value, with the picture placed on a canvas and cropped by a view, captured into a graph;
and the stream against the fldr_rate binding's outputs put through the oracle.  Canary bytes around every plane and in every pitch gap
stay what they were."""
import itertools

import numpy as np
import pytest
import torch

import conform_oracle as O
import rate_frames as RF

pytestmark = pytest.mark.gpu

FILL = 0x5A
# four format pairs that between them cover a matrix change, both depth changes, a range change and both layouts on both sides
PAIRS = [(("nv12", "bt601", "limited", 8), ("nv12", "bt709", "limited", 10)),
         (("i420", "bt709", "full", 10), ("nv12", "bt709", "limited", 8)),
         (("nv12", "bt709", "limited", 8), ("i420", "bt601", "limited", 8)),
         (("i420", "bt601", "limited", 10), ("i420", "bt601", "full", 10))]
PAIR_IDS = ["nv12_601_8-p010_709", "i420_10_full-nv12_8", "nv12_709-i420_601", "i420_10-i420_10_full"]


def _fmt(f):
    import fldr_video
    return fldr_video.Format(*f)


def _noise_frame(fmt, H, W, g):
    """Noise over the whole container range: P010 with noise in the low six bits, yuv420p10le with noise in the high six."""
    import fldr_video as V
    layout, depth = fmt[0], fmt[3]
    if depth == 8:
        return tuple(g.integers(0, 256, s).astype(np.uint8) for s in V.plane_shapes(layout, H, W))
    return tuple(g.integers(0, 65536, s).astype(np.uint16) for s in V.plane_shapes(layout, H, W))


def _blank(fmt, size):
    import fldr_video as V
    dt = np.uint16 if fmt[3] == 10 else np.uint8
    return tuple(np.full(s, FILL | (FILL << 8) if fmt[3] == 10 else FILL, dt) for s in V.plane_shapes(fmt[0], size[0], size[1]))


def _plane_to_dev(p, dev, offset=0, pad=16):
    """A device view of a host plane `offset` bytes into a buffer filled with FILL, with a pitch of the row bytes rounded up to 16, plus
    `pad`.  -> (view, buffer, mask of the plane's own bytes)."""
    r, c = p.shape
    b = p.dtype.itemsize
    pitch = (c * b + 15) // 16 * 16 + pad
    buf = torch.full((r * pitch + offset + 256,), FILL, dtype=torch.uint8, device=dev)
    view = buf[offset:offset + r * pitch].view(r, pitch)[:, :c * b]
    view.copy_(torch.from_numpy(np.ascontiguousarray(p).view(np.uint8).reshape(r, c * b)).to(dev))
    mask = np.zeros(buf.numel(), bool)
    mask[offset:offset + r * pitch].reshape(r, pitch)[:, :c * b] = True
    return (view.view(torch.uint16) if b == 2 else view), buf, mask


def _np(view):
    a = (view.view(torch.int16) if view.dtype == torch.uint16 else view).cpu().numpy()
    return a.view(np.uint16) if view.dtype == torch.uint16 else a


def _check(dev, host, src, dst, out_size=None, at=(0, 0), dither=False, moved=(), want=None):
    """fldr_conform_frame of one host frame on the device against the oracle.  moved: the planes, numbered through the source's and then the
    output's, that sit 2 bytes off a 16-byte boundary with a pitch that is no multiple of 16.  The outputs start filled with FILL, which the
    gaps and the bytes around every plane keep.  -> the oracle's output."""
    import fldr_conform as K
    out_size = out_size or host[0].shape
    if want is None:
        want = O.conform(host, src, dst, out_size, at, int(dither))
    kw = lambda q: dict(offset=2, pad=16 + 6) if q in moved else dict(offset=0, pad=16)
    ins = [_plane_to_dev(p, dev, **kw(q)) for q, p in enumerate(host)]
    outs = [_plane_to_dev(p, dev, **kw(len(host) + q)) for q, p in enumerate(_blank(dst, out_size))]
    for q, (view, _, _) in enumerate(ins + outs):
        b = view.element_size()
        assert (view.data_ptr() % 16 == 0 and (view.stride(0) * b) % 16 == 0) == (q not in moved)
    K.frame(tuple(v for v, _, _ in ins), _fmt(src), tuple(v for v, _, _ in outs), _fmt(dst), at, dither)
    torch.cuda.synchronize()
    for p, (view, buf, mask) in enumerate(outs):
        got = _np(view)
        assert np.array_equal(got, want[p]), (src, dst, out_size, at, dither, moved, p, np.argwhere(got != want[p])[:4])
        assert (buf.cpu().numpy()[~mask] == FILL).all(), (src, dst, out_size, p)
    for view, buf, mask in ins:
        assert (buf.cpu().numpy()[~mask] == FILL).all()
    return want


def _runs(dst):
    """(samples of a luma run, chroma columns of a chroma run) of an output format, from the kernel's own constants."""
    import fldr_conform as K
    ns = K.RUN_BYTES // (2 if dst[3] == 10 else 1)
    return ns, (ns // 2 if dst[0] == "nv12" else ns)


# ---- every format pair ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(5, 7), (6, 10)], ids=["5x7", "6x10"])
def test_all_256_format_pairs(dev, size):
    g = np.random.default_rng(size[1])
    hosts = {f: _noise_frame(f, size[0], size[1], g) for f in O.FORMATS}
    pairs = list(itertools.product(O.FORMATS, O.FORMATS))
    assert len(pairs) == 256
    for src, dst in pairs:
        want = _check(dev, hosts[src], src, dst)
        if src[1:] == dst[1:]:                                                # equal matrix, range and depth: the samples, in canonical form
            vals = O.split(hosts[src], src[0], src[3])
            assert all(np.array_equal(a, b) for a, b in zip(want, O.join(*vals, dst[0], dst[3])))


@pytest.mark.parametrize("size", [(5, 7), (6, 10)], ids=["5x7", "6x10"])
def test_dither_on_every_pair_that_changes_depth_or_range(dev, size):
    """The 48 (matrix, range, depth) pairs whose depth or range differ — the 32 that change the depth among them —, the layouts alternating
    so that all four occur on both sides; and equal formats stay the identity under dither."""
    g = np.random.default_rng(size[0])
    changing = [(s, d) for s, d in itertools.product(O.COLOURS, O.COLOURS) if s[1:] != d[1:]]
    assert len(changing) == 48 and sum(s[2] != d[2] for s, d in changing) == 32
    for n, (s, d) in enumerate(changing):
        src, dst = (O.LAYOUTS[n & 1],) + s, (O.LAYOUTS[(n >> 1) & 1],) + d
        host = _noise_frame(src, size[0], size[1], g)
        want = _check(dev, host, src, dst, dither=True)
        assert any(not np.array_equal(a, b) for a, b in zip(want, O.conform(host, src, dst))) or s[2] <= d[2]
    for f in O.FORMATS[::3]:
        host = _noise_frame(f, size[0], size[1], g)
        want = _check(dev, host, f, f, dither=True)
        assert all(np.array_equal(a, b) for a, b in zip(want, O.join(*O.split(host, f[0], f[3]), f[0], f[3])))


# ---- shapes -------------------------------------------------------------------------------------------------------------------------------
def _edge_sizes(dst):
    """One sample either side of a lane's run and of a workgroup's row of runs, for the luma plane and for the chroma planes."""
    import fldr_conform as K
    ns, cols = _runs(dst)
    widths = {ns, 2 * cols, K.THREADS * ns, K.THREADS * 2 * cols}           # luma samples of: a luma run, a chroma run, a workgroup of each
    sizes = [(3, w + d) for w in sorted(widths) for d in (-1, 0, 1)]
    # ... and runs that wrap from one row to the next inside a workgroup, and a workgroup that ends inside the plane
    return sizes + [(K.THREADS // 4 + 1, 4 * ns + 1), (2 * K.THREADS // 4 + 3, 8 * cols - 1)]


@pytest.mark.parametrize("src,dst", PAIRS, ids=PAIR_IDS)
def test_small_and_edge_shapes(dev, src, dst):
    g = np.random.default_rng(11)
    for H, W in [(1, 1), (1, 2), (2, 1), (3, 5), (17, 33)] + _edge_sizes(dst):
        _check(dev, _noise_frame(src, H, W, g), src, dst, dither=src[3] > dst[3])


@pytest.mark.parametrize("src,dst", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("size", [(4, 16383), (3001, 4)], ids=["long row", "many rows"])
def test_a_long_row_and_many_rows(dev, src, dst, size):
    g = np.random.default_rng(size[0])
    _check(dev, _noise_frame(src, size[0], size[1], g), src, dst)


@pytest.mark.parametrize("src,dst", PAIRS, ids=PAIR_IDS)
def test_planes_off_a_16_byte_boundary_take_the_per_sample_path(dev, src, dst):
    """Each plane of the source and of the output once 2 bytes off a 16-byte boundary with a pitch that is no multiple of 16 while the
    others stay aligned, then all of them: the same bytes.  The picture is placed at (4, 2) and at (16, 2), so that the source runs lie
    off and on the output's runs."""
    import fldr_video as V
    g = np.random.default_rng(5)
    host = _noise_frame(src, 12, 37, g)
    n = len(V.plane_shapes(src[0], 2, 2)) + len(V.plane_shapes(dst[0], 2, 2))
    for at in ((4, 2), (16, 2)):
        want = O.conform(host, src, dst, (19, 70), at)
        for moved in [()] + [(q,) for q in range(n)] + [tuple(range(n))]:
            _check(dev, host, src, dst, (19, 70), at, moved=moved, want=want)


# ---- every code value -----------------------------------------------------------------------------------------------------------------------
def test_every_code_at_depth_8(dev):
    """1024 x 1024: the chroma planes hold every (U, V) pair (four times), the luma every Y code; 601 <-> 709, limited <-> full, 8 -> 10."""
    g = np.random.default_rng(8)
    Y = g.integers(0, 256, (1024, 1024)).astype(np.int64)
    idx = np.arange(512 * 512, dtype=np.int64).reshape(512, 512)
    U, V = idx % 256, (idx // 256) % 256
    assert len(np.unique(Y)) == 256 and len(np.unique(U * 256 + V)) == 65536
    for src, dst in ((("nv12", "bt601", "limited", 8), ("nv12", "bt709", "limited", 8)), (("i420", "bt709", "limited", 8), ("nv12", "bt601", "limited", 8)),
                     (("nv12", "bt709", "limited", 8), ("i420", "bt709", "full", 8)), (("i420", "bt601", "full", 8), ("i420", "bt601", "limited", 8)),
                     (("nv12", "bt601", "full", 8), ("nv12", "bt709", "limited", 10))):
        _check(dev, O.join(Y, U, V, src[0], 8), src, dst)


@pytest.mark.parametrize("layout", ["nv12", "i420"])
def test_every_code_at_depth_10(dev, layout):
    """Every code of each plane with the other two swept by a stride coprime to 1024; P010 with noise in its ignored low bits,
    yuv420p10le in its ignored high bits."""
    g = np.random.default_rng(10)
    il, ic = np.arange(64 * 64, dtype=np.int64).reshape(64, 64), np.arange(32 * 32, dtype=np.int64).reshape(32, 32)
    Y, U, V = (il * 77 + 5) % 1024, ic % 1024, (ic * 389 + 1) % 1024
    assert all(len(np.unique(p)) == 1024 for p in (Y, U, V))
    clean = O.join(Y, U, V, layout, 10)
    dirt = [g.integers(0, 64, p.shape).astype(np.uint16) for p in clean]
    host = tuple(p | (d if layout == "nv12" else d << 10) for p, d in zip(clean, dirt))
    assert all(np.array_equal(a, b) for a, b in zip(O.split(host, layout, 10), (Y, U, V))) and not np.array_equal(host[0], clean[0])
    for dst, dither in ((("nv12", "bt601", "limited", 8), True), (("i420", "bt709", "full", 8), False), (("i420", "bt709", "full", 10), False),
                        (("nv12", "bt601", "limited", 10), False), (("nv12", "bt709", "limited", 10), False)):
        src = (layout, "bt709", "limited", 10)
        want = _check(dev, host, src, dst, dither=dither)
        if dst[1:] == src[1:]:
            assert all(np.array_equal(a, b) for a, b in zip(want, O.join(Y, U, V, dst[0], 10)))      # the dirty bits were dropped, nothing else


# ---- placement ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", PAIRS, ids=PAIR_IDS)
def test_placement_on_a_canvas(dev, src, dst):
    g = np.random.default_rng(2)
    yo_d, _, cc_d, _, _ = O.side(dst[2], dst[3])
    for (H, W), (oH, oW), at in (((10, 14), (20, 40), (0, 0)), ((10, 14), (20, 40), (2, 4)), ((10, 14), (20, 40), (26, 10)),      # flush bottom-right
                                 ((9, 13), (20, 40), (6, 2)), ((9, 13), (21, 39), (26, 12)), ((9, 13), (21, 39), (8, 6)),          # odd in even, odd in odd
                                 ((9, 13), (9, 13), (0, 0)), ((1, 1), (3, 3), (2, 2)), ((7, 70), (11, 200), (64, 2))):             # the canvas is the picture
        host = _noise_frame(src, H, W, g)
        want = _check(dev, host, src, dst, (oH, oW), at, dither=src[3] > dst[3])
        Yo, Uo, Vo = O.split(want, dst[0], dst[3])
        border = np.ones((oH, oW), bool)
        border[at[1]:at[1] + H, at[0]:at[0] + W] = False
        cb = np.ones(Uo.shape, bool)
        cb[at[1] // 2:at[1] // 2 + (H + 1) // 2, at[0] // 2:at[0] // 2 + (W + 1) // 2] = False
        assert (Yo[border] == yo_d).all() and (Uo[cb] == cc_d).all() and (Vo[cb] == cc_d).all()       # black of the destination range and depth


@pytest.mark.parametrize("src,dst", PAIRS, ids=PAIR_IDS)
def test_a_view_crops_a_larger_device_frame(dev, src, dst):
    import fldr_conform as K
    g = np.random.default_rng(4)
    big = _noise_frame(src, 40, 60, g)
    for (x, y), size in (((6, 4), (21, 33)), ((0, 0), (40, 60)), ((32, 18), (22, 28)), ((58, 38), (1, 1))):
        crop = tuple(np.ascontiguousarray(p) for p in O.view(big, src[0], x, y, size))
        want = O.conform(crop, src, dst, (size[0] + 4, size[1] + 6), (2, 2))
        ins = [_plane_to_dev(p, dev) for p in big]
        outs = [_plane_to_dev(p, dev) for p in _blank(dst, (size[0] + 4, size[1] + 6))]
        window = K.view(tuple(v for v, _, _ in ins), _fmt(src), x, y, size)
        assert [tuple(w.shape) for w in window] == [c.shape for c in crop]
        K.frame(window, _fmt(src), tuple(v for v, _, _ in outs), _fmt(dst), (2, 2))
        torch.cuda.synchronize()
        for p, (view, buf, mask) in enumerate(outs):
            assert np.array_equal(_np(view), want[p]), ((x, y), size, p)
            assert (buf.cpu().numpy()[~mask] == FILL).all()


# ---- graphs and bad calls -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", PAIRS[:2], ids=PAIR_IDS[:2])
def test_a_conform_captured_once_follows_rewritten_sources(dev, src, dst):
    import fldr_conform as K
    in_size, out_size, at = (36, 130), (40, 160), (14, 2)
    g = np.random.default_rng(6)
    hosts = [_noise_frame(src, in_size[0], in_size[1], g) for _ in range(3)]
    ins = tuple(v for v, _, _ in [_plane_to_dev(p, dev) for p in hosts[0]])
    out = tuple(v for v, _, _ in [_plane_to_dev(p, dev) for p in _blank(dst, out_size)])
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        K.frame(ins, _fmt(src), out, _fmt(dst), at)                         # warm
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        K.frame(ins, _fmt(src), out, _fmt(dst), at)
    for h in hosts[1:] + hosts[:1]:
        for d, p in zip(ins, h):
            (d.view(torch.uint8) if p.dtype == np.uint16 else d).copy_(torch.from_numpy(np.ascontiguousarray(p).view(np.uint8).reshape(p.shape[0], -1)).to(dev))
        graph.replay()
        torch.cuda.synchronize()
        for o, w in zip(out, O.conform(h, src, dst, out_size, at)):
            assert np.array_equal(_np(o), w)
    del graph


def test_bad_frame_calls_leave_the_output_untouched(dev):
    import fldr_conform as K
    import fldr_video as V
    src, dst = PAIRS[0]
    in_size, out_size = (16, 64), (24, 96)
    g = np.random.default_rng(0)
    ins = tuple(torch.from_numpy(p).to(dev) for p in _noise_frame(src, in_size[0], in_size[1], g))
    out = tuple(torch.full(s, 0x4444, dtype=torch.int16, device=dev).view(torch.uint16) for s in V.plane_shapes("nv12", out_size[0], out_size[1]))
    fs, fo = V.frame_struct(ins), V.frame_struct(out)
    sp = V._stream_ptr(dev, None)
    cfg = lambda **kw: K.config(kw.get("in_size", in_size), _fmt(src), kw.get("out_size", out_size), _fmt(dst), kw.get("at", (2, 2)), kw.get("dither", 0))
    assert K.frame_raw(None, fs, fo, sp) == K.E_ARG and K.frame_raw(cfg(), None, fo, sp) == K.E_ARG and K.frame_raw(cfg(), fs, None, sp) == K.E_ARG
    assert K.frame_raw(cfg(at=(1, 2)), fs, fo, sp) == K.E_ARG and K.frame_raw(cfg(at=(34, 2)), fs, fo, sp) == K.E_ARG
    assert K.frame_raw(cfg(out_size=(24, 16385)), fs, fo, sp) == K.E_ARG and K.frame_raw(cfg(dither=2), fs, fo, sp) == K.E_ARG
    bad = cfg()
    bad.out_format.depth = 12
    assert K.frame_raw(bad, fs, fo, sp) == V.E_FORMAT
    gone = V.frame_struct(out)
    gone.plane[1] = None
    assert K.frame_raw(cfg(), fs, gone, sp) == V.E_PLANE
    short = V.frame_struct(out)
    short.pitch[0] = 2 * out_size[1] - 2
    assert K.frame_raw(cfg(), fs, short, sp) == V.E_PITCH
    both = V.frame_struct(out)
    both.plane[1] = ins[0].data_ptr() + 8                                   # out's chroma inside the source's luma
    assert K.frame_raw(cfg(), fs, both, sp) == K.E_ARG
    torch.cuda.synchronize()
    assert all(bool((p.view(torch.int16) == 0x4444).all()) for p in out)
    assert K.frame_raw(cfg(), fs, fo, sp) == 0                              # and a good call does write
    torch.cuda.synchronize()
    assert not bool((out[0].view(torch.int16) == 0x4444).any()) and not bool((out[1].view(torch.int16) == 0x4444).any())


# ---- the stream ----------------------------------------------------------------------------------------------------------------------------
H, W = 256, 448


@pytest.fixture(scope="module")
def nm(dev):
    import fldr_harness as Hn
    import fldr_model
    m = fldr_model.NativeModel.from_npz(Hn.DEFAULT_WEIGHTS, device=dev.index or 0)
    yield m
    m.close()


def _stream_frames(src):
    """Four frames of tests/rate_frames.py: a moving, grainy texture, then the unrelated second frame of its "cut" case and that frame
    moved two samples to the right: a cut between frames 1 and 2 and nowhere else."""
    layout, mat, rng, depth = src
    a = RF.content("grain", H, W, 0, layout, depth, mat, rng)
    b = RF.content("cut", H, W, 0, layout, depth, mat, rng)[1]
    return [a[0], a[1], b, tuple(np.roll(p, 2, axis=1) for p in b)]


def _same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for n, (a, b) in enumerate(zip(got, want)):
        for p, (x, y) in enumerate(zip(a, b)):
            assert x.dtype == y.dtype and np.array_equal(x, y), (what, n, p)


@pytest.mark.parametrize("src,dst,rates,out_size,at,dither",
                         [(("nv12", "bt601", "limited", 8), ("nv12", "bt709", "limited", 10), (24, 60), (H, 512), (32, 0), False),
                          (("i420", "bt709", "limited", 10), ("nv12", "bt709", "limited", 8), (25, 50), (H + 16, W), (0, 8), True)],
                         ids=["24-60 nv12 601 -> p010 709 pillarboxed", "25-50 i420 10 -> nv12 8 dithered letterboxed"])
def test_stream_equals_the_converter_put_through_the_oracle(nm, dev, src, dst, rates, out_size, at, dither):
    """Output j is the conform of output j of a fldr_rate.Converter of the same rates and scene settings at the in size and format, pushed
    the same frames: the outputs that are an input frame's own bytes and the ones the cut replaced included; then the flush, a second flush,
    and a reset in front of it all."""
    import fldr_conform as K
    import fldr_rate as R
    frames = _stream_frames(src)
    conv = lambda f: O.conform(f, src, dst, out_size, at, int(dither))
    ref = R.Converter(nm, H, W, _fmt(src), rates[0], rates[1], scene=True)
    want, scenes = [], []
    for f in frames:
        want.append([conv(o) for o in ref.push(f)])
        scenes.append(ref.last_scene)
    want.append([conv(o) for o in ref.flush()])
    ref.close()
    assert [len(w) for w in want] == [len(p) for p in R.schedule(len(frames), rates[0], rates[1])] and sum(len(w) for w in want) >= 6
    assert [s["cut"] for s in scenes] == [0, 0, 1, 0]
    c = K.Conformer(nm, (H, W), _fmt(src), out_size, _fmt(dst), rates[0], rates[1], at, dither, True)
    assert c.max_out == R.max_out(rates[0], rates[1])
    for f in frames[2:4]:                                                   # two frames of some other stream, forgotten by the reset
        c.push(f)
    c.reset()
    for n, f in enumerate(frames):
        _same(c.push(f), want[n], "push %d" % n)
        assert c.last_scene == scenes[n], (n, c.last_scene, scenes[n])
    _same(c.flush(), want[-1], "flush")
    assert c.flush() == []                                                  # a second flush returns none
    c.close()


def test_stream_with_equal_rates_needs_no_model(dev):
    """B == 1: every output is an input frame conformed.  No model, no workspace, no forward: a pure converter."""
    import fldr_conform as K
    src, dst = ("i420", "bt601", "full", 8), ("nv12", "bt709", "limited", 10)
    out_size, at = (H + 3, W + 7), (4, 2)
    frames = _stream_frames(src)
    want = [O.conform(f, src, dst, out_size, at) for f in frames]
    c = K.Conformer(None, (H, W), _fmt(src), out_size, _fmt(dst), (30000, 1001), (30000, 1001), at, device=dev.index or 0)
    assert c.max_out == 1
    for n, f in enumerate(frames):
        _same(c.push(f), want[n - 1:n] if n else [], "push %d" % n)
        assert c.last_scene["cut"] == (1 if n == 2 else 0)
    _same(c.flush(), want[-1:], "flush")
    assert c.flush() == []
    c.reset()                                                               # after a flush and a reset the object is a fresh stream
    assert c.push(frames[1]) == []
    _same(c.push(frames[0]), want[1:2], "after the reset")
    c.close()
