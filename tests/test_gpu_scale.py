"""The scale API (libfldr_scale.so through fldr_scale) on the GPU.  Every comparison is exact.  fldr_scale_frame gives the bytes of
tests/scale_oracle.py on the library's own tables at every size, format, filter and access form, and leaves all pitch padding alone.
fldr_scale_forward leaves in its temporaries what the oracle (BEFORE) or fldr_rate.NativeRate / fldr_video.NativeVideo (AFTER) give, and
its outputs are the composition.  A stream returns, push by push, what a fldr_rate.Converter at the out size returns for the scaled frames
(BEFORE), or the scale of what one at the in size returns (AFTER).  The stream's frames are those of tests/cadence_frames.py: a moving
texture of 256 x 448 with one cut, and their bicubic enlargement to 384 x 672."""
import functools

import numpy as np
import pytest
import torch

import cadence_frames as CF
import scale_oracle as O

pytestmark = pytest.mark.gpu

FORMATS = [("nv12", 8), ("i420", 8), ("nv12", 10), ("i420", 10)]
FILTERS = (O.BILINEAR, O.BICUBIC, O.LANCZOS3)
FILL = 0x5A
# (in H, in W) -> (out H, out W)
SHAPES = [((1, 1), (1, 1)), ((1, 1), (3, 5)), ((3, 5), (1, 1)), ((2, 2), (5, 7)), ((5, 7), (2, 2)), ((16, 16), (17, 15)), ((33, 65), (130, 257)),
          ((130, 257), (33, 65)), ((64, 48), (16, 12)),
          ((8, 200), (8, 19)),                    # Lanczos3: exactly 64 taps horizontally
          ((31, 20), (3, 20)),                    # Lanczos3: 62 taps vertically
          ((8, 1100), (8, 100)),                  # Lanczos3 would need 66 taps: refused; the other two run
          ((36, 130), (36, 130))]                 # identity
BIG = (384, 672)


def _fmt(layout, depth=8):
    import fldr_video
    return fldr_video.Format(layout, "bt709", "limited", depth)


def _noise_frame(layout, depth, H, W, g):
    """Noise over the whole container range; P010 with noise in the low six bits, yuv420p10le with noise in the high six."""
    import fldr_video as V
    if depth == 8:
        return tuple(g.integers(0, 256, s).astype(np.uint8) for s in V.plane_shapes(layout, H, W))
    return tuple(g.integers(0, 65536, s).astype(np.uint16) for s in V.plane_shapes(layout, H, W))


def _plane_to_dev(p, dev, offset=0, pad=16, fill=FILL):
    """A device view of a host plane `offset` bytes into a buffer, with a pitch of the row bytes rounded up to 16, plus `pad`.
    offset 0 and pad a multiple of 16: the 16-byte stores; anything else: the per-sample form.  -> (view, buffer, mask of row bytes)."""
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


def _blank(layout, depth, size):
    import fldr_video as V
    dt = np.uint16 if depth == 10 else np.uint8
    return tuple(np.full(s, FILL | (FILL << 8) if depth == 10 else FILL, dt) for s in V.plane_shapes(layout, size[0], size[1]))


def _check_frame(dev, host, layout, depth, out_size, access="aligned", filters=FILTERS, want_of=None):
    """fldr_scale_frame of one host frame on the device against the oracle on the library's tables; the outputs start filled with FILL,
    which the gaps and the bytes around every plane keep.  -> {filter: the oracle's output} of the filters that ran."""
    import fldr_scale as K
    in_size = host[0].shape
    fmt = _fmt(layout, depth)
    src = tuple(v for v, _, _ in _frame_to_dev(host, dev, access))
    done = {}
    for filt in filters:
        if max(O.taps_count(in_size[1], out_size[1], filt), O.taps_count(in_size[0], out_size[0], filt)) > O.MAX_TAPS:
            with pytest.raises(K.ScaleError) as e:                          # the tap limit: refused at the create, nothing to launch
                K.Map(in_size, out_size, fmt, filt)
            assert e.value.code == K.E_ARG
            continue
        want = want_of(filt) if want_of else O.scale(host, layout, depth, out_size, K.tables(in_size, out_size, filt))
        for read in (K.READ_DIRECT, K.READ_STAGED):                         # both reads of the horizontal pass: the same bytes
            m = K.Map(in_size, out_size, fmt, filt, device=dev.index or 0, read=read)
            assert m.read == read and (m.struct.stage_span[0] > 0) == (read == K.READ_STAGED)
            assert m.taps == (O.taps_count(in_size[1], out_size[1], filt), O.taps_count(in_size[0], out_size[0], filt)) and m.lds_bytes <= 65536
            outs = _frame_to_dev(_blank(layout, depth, out_size), dev, access)
            m.frame(src, tuple(v for v, _, _ in outs))
            torch.cuda.synchronize()
            for p, (view, buf, mask) in enumerate(outs):
                got = _np(view)
                assert np.array_equal(got, want[p]), (filt, read, p, np.argwhere(got != want[p])[:4])
                assert (buf.cpu().numpy()[~mask] == FILL).all(), (filt, read, p)
            m.close()
        done[filt] = want
    return done


# ---- fldr_scale_frame -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("access", ["aligned", "offset"])
@pytest.mark.parametrize("layout,depth", FORMATS)
@pytest.mark.parametrize("in_size,out_size", SHAPES, ids=["%dx%d-%dx%d" % (a + b) for a, b in SHAPES])
def test_frame_equals_the_oracle_and_leaves_the_rest_alone(dev, in_size, out_size, layout, depth, access):
    g = np.random.default_rng(in_size[0] * 1000 + in_size[1] + depth)
    host = _noise_frame(layout, depth, in_size[0], in_size[1], g)
    done = _check_frame(dev, host, layout, depth, out_size, access)
    if in_size == (8, 1100):
        assert sorted(done) == [O.BILINEAR, O.BICUBIC]                       # Lanczos3 was refused
    else:
        assert sorted(done) == list(FILTERS)
    if in_size == out_size:                                                 # identity sizes: the canonicalised input, under every filter
        want = O.canonicalised(host, layout, depth)
        assert all(np.array_equal(a, b) for w in done.values() for a, b in zip(w, want))


@pytest.mark.parametrize("layout,depth", FORMATS)
@pytest.mark.parametrize("in_size,out_size", [((4, 16383), (4, 5735)), ((3001, 4), (1001, 4))], ids=["long row", "many rows"])
def test_frame_of_a_long_row_and_of_many_rows(dev, in_size, out_size, layout, depth):
    """(4, 16383) -> (4, 5735): the longest odd row the size limit allows at the ratio of 20001 -> 7001, tens of tiles across, the last one
    partial; (3001, 4) -> (1001, 4): a column of tiles, each of whose source rows begin where the vertical table says."""
    g = np.random.default_rng(in_size[0] + in_size[1] + depth)
    host = _noise_frame(layout, depth, in_size[0], in_size[1], g)
    assert len(_check_frame(dev, host, layout, depth, out_size, "aligned")) == 3
    _check_frame(dev, host, layout, depth, out_size, "offset", filters=(O.BICUBIC,))


def test_a_row_beyond_the_size_limit_is_refused(dev):
    """4 x 20001 -> 4 x 7001 is beyond FLDR_SCALE_MAX_SIZE = 16384 on the in side: no map is made for it under any filter, so nothing can be
    launched on a frame of that size; 16384 itself is taken."""
    import fldr_scale as K
    fmt = _fmt("nv12", 8)
    for filt in FILTERS:
        for in_size, out_size in (((4, 20001), (4, 7001)), ((4, 7001), (4, 20001)), ((16385, 4), (4, 4))):
            m = K.MapStruct()
            assert K.map_create_raw(K.map_config(in_size, out_size, fmt, filt), m) == K.E_ARG and m.live == 0 and not m.tables
        m = K.Map((2, 16384), (2, 8192), fmt, filt)
        assert m.taps[0] == 4 * (filt + 1)
        m.close()


@pytest.mark.parametrize("layout,depth", FORMATS)
def test_code_range_ends_clamp_on_both_sides(dev, layout, depth):
    """Planes of all 0 and all mx stay what they are.  Checkerboards of 0 and mx — of single samples and of 2 x 2 blocks —, up and down,
    under the two filters with negative lobes: the oracle's unclamped values are asserted to leave the range on both sides in every case
    but the single-sample board going down, which averages out, and the device clamps the same."""
    import fldr_scale as K
    import fldr_video as V
    mx = 1023 if depth == 10 else 255
    word = (mx << 6) if (layout, depth) == ("nv12", 10) else mx
    dt = np.uint16 if depth == 10 else np.uint8
    H, W = 20, 44
    shapes = V.plane_shapes(layout, H, W)
    for v in (0, word):
        flat = tuple(np.full(s, v, dt) for s in shapes)
        for out_size in ((31, 70), (9, 21)):
            done = _check_frame(dev, flat, layout, depth, out_size)
            assert all((p == v).all() for w in done.values() for p in w)
    yy, xx = np.mgrid[0:H, 0:W]
    board = tuple((((yy[:r, :c] + xx[:r, :c]) & 1) * word).astype(dt) for r, c in shapes)
    blocks = tuple(((((yy[:r, :c] >> 1) + (xx[:r, :c] >> 1)) & 1) * word).astype(dt) for r, c in shapes)
    for name, host in (("board", board), ("blocks", blocks)):
        for out_size in ((31, 70), (13, 30)):
            _check_frame(dev, host, layout, depth, out_size)
            for filt in (O.BICUBIC, O.LANCZOS3):
                t = K.tables((H, W), out_size, filt)
                lo, hi = O.unclamped_range(O.value(host[0], layout, depth), t["luma_x"], t["luma_y"], depth)
                if name == "board" and out_size[0] < H:
                    # a one-sample checkerboard under a low-pass of 1.5 samples or more averages out: it cannot leave the range going down
                    assert 0 < lo and hi < mx, (filt, out_size, lo, hi)
                else:
                    assert lo < 0 and hi > mx, (name, filt, out_size, lo, hi)   # the oracle itself was clamped on both sides, up AND down
                    vals = O.value(O.scale(host, layout, depth, out_size, t)[0], layout, depth)
                    assert (vals == 0).any() and (vals == mx).any()          # ... and produced both clamped values


@pytest.mark.parametrize("layout,depth", [("nv12", 8), ("i420", 10)])
def test_one_plane_off_a_16_byte_boundary_takes_the_per_sample_path(dev, layout, depth):
    """Every other plane stays aligned: the access form is decided per output plane.  Offsets of 1 .. 15 bytes (even ones at depth 10) of an
    output plane, a pitch that is no multiple of 16, and a source plane moved the same way (which decides nothing): the same bytes."""
    import fldr_scale as K
    in_size, out_size = (12, 37), (19, 53)
    b = 2 if depth == 10 else 1
    fmt = _fmt(layout, depth)
    g = np.random.default_rng(depth)
    host = _noise_frame(layout, depth, in_size[0], in_size[1], g)
    blank = _blank(layout, depth, out_size)
    for filt in (O.BILINEAR, O.LANCZOS3):
        m = K.Map(in_size, out_size, fmt, filt)
        want = O.scale(host, layout, depth, out_size, K.tables(in_size, out_size, filt))
        for off in range(b, 16, b):
            for where in ("source", "out", "pitch"):
                which = off % len(host)                                     # the plane that is moved
                src = [_plane_to_dev(p, dev, offset=off if (where, q) == ("source", which) else 0) for q, p in enumerate(host)]
                outs = [_plane_to_dev(p, dev, offset=off if (where, q) == ("out", which) else 0, pad=16 + (off if (where, q) == ("pitch", which) else 0))
                        for q, p in enumerate(blank)]
                m.frame(tuple(v for v, _, _ in src), tuple(v for v, _, _ in outs))
                torch.cuda.synchronize()
                for p, (view, buf, mask) in enumerate(outs):
                    assert np.array_equal(_np(view), want[p]), (off, where, filt, p)
                    assert (buf.cpu().numpy()[~mask] == FILL).all(), (off, where, filt, p)
        m.close()


@pytest.mark.parametrize("layout,depth", [("nv12", 8), ("i420", 10), ("nv12", 10)])
def test_tile_boundaries(dev, layout, depth):
    """Output heights and widths one below, at and one above the tile the host picked (read from the filled map, not hard-coded), and the
    same around twice the tile, where the chroma planes of the half-size layouts meet theirs."""
    import fldr_scale as K
    in_size = (24, 200)
    fmt = _fmt(layout, depth)
    g = np.random.default_rng(7 + depth)
    host = _noise_frame(layout, depth, in_size[0], in_size[1], g)
    probe = K.Map(in_size, (32, 600), fmt, K.BICUBIC)
    (th, tw), (cth, ctw) = probe.tile
    probe.close()
    assert th >= 1 and tw >= 16 and cth >= 1 and ctw >= 16
    sizes = [(th + d, 77) for d in (-1, 0, 1)] + [(2 * cth + d, 77) for d in (-2, -1, 0, 1)] + [(9, tw + d) for d in (-1, 0, 1)] + \
            [(9, 2 * ctw + d) for d in (-1, 0, 1)]
    for out_size in sizes:
        m = K.Map(in_size, out_size, fmt, K.BICUBIC)
        assert m.tile == [(th, tw), (cth, ctw)]                             # the same pick for these ratios: the sizes do sit at its edges
        m.close()
        _check_frame(dev, host, layout, depth, out_size, filters=(O.BICUBIC,))


def test_a_strong_shrink_gets_a_lower_tile_and_stays_inside_the_lds_limit(dev):
    import fldr_scale as K
    fmt = _fmt("nv12", 8)
    easy = K.Map((64, 64), (128, 128), fmt, K.LANCZOS3)
    hard = K.Map((2000, 64), (190, 64), fmt, K.LANCZOS3)                    # 64 taps vertically: 16 output rows would need 230 source rows
    assert hard.taps[1] == 64 and hard.tile[0][0] < easy.tile[0][0] and 0 < hard.lds_bytes <= 65536 and easy.lds_bytes <= 65536
    easy.close()
    hard.close()
    g = np.random.default_rng(3)
    _check_frame(dev, _noise_frame("nv12", 8, 2000, 64, g), "nv12", 8, (190, 64), filters=(O.LANCZOS3,))


@pytest.mark.parametrize("layout,depth", FORMATS)
def test_a_reduction_too_strong_to_stage_reads_directly(dev, layout, depth):
    """Bicubic 8192 -> 512 columns (64 taps): a tile's source span (16 x the tile + 64) is beyond what a staged chunk may take.  STAGED is refused at the create,
    AUTO resolves to DIRECT, and the bytes are the oracle's.  AUTO stages a bicubic reduction by 8, and no enlargement and nothing bilinear."""
    import fldr_scale as K
    fmt = _fmt(layout, depth)
    in_size, out_size = (6, 8192), (9, 512)
    m = K.MapStruct()
    assert K.map_create_raw(K.map_config(in_size, out_size, fmt, K.BICUBIC, read=K.READ_STAGED), m) == K.E_ARG and m.live == 0
    auto = K.Map(in_size, out_size, fmt, K.BICUBIC)
    assert auto.taps[0] == 64 and auto.read == K.READ_DIRECT and list(auto.struct.stage_span) == [0, 0] and auto.struct.stage_at == 0
    g = np.random.default_rng(11 + depth)
    host = _noise_frame(layout, depth, in_size[0], in_size[1], g)
    src = tuple(v for v, _, _ in _frame_to_dev(host, dev))
    outs = _frame_to_dev(_blank(layout, depth, out_size), dev)
    auto.frame(src, tuple(v for v, _, _ in outs))
    torch.cuda.synchronize()
    want = O.scale(host, layout, depth, out_size, K.tables(in_size, out_size, K.BICUBIC))
    for p, (view, buf, mask) in enumerate(outs):
        assert np.array_equal(_np(view), want[p]) and (buf.cpu().numpy()[~mask] == FILL).all(), p
    auto.close()
    for size_in, size_out, filt, read in (((6, 2048), (9, 256), K.BICUBIC, K.READ_STAGED), ((6, 2048), (9, 256), K.LANCZOS3, K.READ_STAGED),
                                          ((6, 2048), (9, 256), K.BILINEAR, K.READ_DIRECT), ((6, 256), (9, 2048), K.LANCZOS3, K.READ_DIRECT),
                                          ((60, 256), (9, 256), K.LANCZOS3, K.READ_DIRECT)):       # the WIDTH decides: it is the horizontal pass
        mild = K.Map(size_in, size_out, fmt, filt)
        assert mild.read == read, (size_in, size_out, filt)
        if read == K.READ_STAGED:
            assert mild.struct.stage_span[0] > 0 and 0 < mild.struct.stage_at < mild.lds_bytes <= 65536
        mild.close()


@pytest.mark.parametrize("layout,depth", [("nv12", 8), ("nv12", 10), ("i420", 10)])
def test_a_scale_captured_once_follows_rewritten_sources(dev, layout, depth):
    import fldr_scale as K
    in_size, out_size = (36, 130), (50, 97)
    fmt = _fmt(layout, depth)
    g = np.random.default_rng(depth + 1)
    hosts = [_noise_frame(layout, depth, in_size[0], in_size[1], g) for _ in range(3)]
    m = K.Map(in_size, out_size, fmt, K.LANCZOS3)
    t = K.tables(in_size, out_size, K.LANCZOS3)
    src = tuple(v for v, _, _ in _frame_to_dev(hosts[0], dev))
    out = tuple(v for v, _, _ in _frame_to_dev(_blank(layout, depth, out_size), dev))
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m.frame(src, out)                                                   # warm
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        m.frame(src, out)
    for h in hosts[1:] + hosts[:1]:
        for d, p in zip(src, h):
            (d.view(torch.uint8) if depth == 10 else d).copy_(torch.from_numpy(np.ascontiguousarray(p).view(np.uint8).reshape(p.shape[0], -1)).to(dev))
        graph.replay()
        torch.cuda.synchronize()
        for o, w in zip(out, O.scale(h, layout, depth, out_size, t)):
            assert np.array_equal(_np(o), w)
    del graph
    m.close()


def test_bad_frame_calls_leave_the_output_untouched(dev):
    import fldr_scale as K
    import fldr_video as V
    in_size, out_size = (16, 64), (24, 48)
    fmt = _fmt("nv12", 8)
    g = np.random.default_rng(0)
    src = tuple(torch.from_numpy(p).to(dev) for p in _noise_frame("nv12", 8, in_size[0], in_size[1], g))
    out = tuple(torch.full(s, 0x44, dtype=torch.uint8, device=dev) for s in V.plane_shapes("nv12", out_size[0], out_size[1]))
    m = K.Map(in_size, out_size, fmt, K.BICUBIC)
    fs, fo = V.frame_struct(src), V.frame_struct(out)
    sp = V._stream_ptr(dev, None)
    assert K.frame_raw(None, fs, fo, sp) == K.E_STATE and K.frame_raw(K.MapStruct(), fs, fo, sp) == K.E_STATE
    assert K.frame_raw(m.struct, None, fo, sp) == K.E_ARG and K.frame_raw(m.struct, fs, None, sp) == K.E_ARG
    bad = V.frame_struct(out)
    bad.plane[1] = None
    assert K.frame_raw(m.struct, fs, bad, sp) == V.E_PLANE
    short = V.frame_struct(out)
    short.pitch[1] = out_size[1] - 1
    assert K.frame_raw(m.struct, fs, short, sp) == V.E_PITCH
    both = V.frame_struct(out)
    both.plane[1] = src[0].data_ptr() + 8                                   # out's chroma inside the source's luma
    assert K.frame_raw(m.struct, fs, both, sp) == K.E_ARG
    assert K.frame_raw(m.struct, fs, fs, sp) == K.E_ARG                     # the source as its own output (its pitches do hold an out row)
    dead = K.MapStruct.from_buffer_copy(bytes(m.struct))
    dead.live = 0
    assert K.frame_raw(dead, fs, fo, sp) == K.E_STATE
    torch.cuda.synchronize()
    assert all(bool((p == 0x44).all()) for p in out)
    assert K.frame_raw(m.struct, fs, fo, sp) == 0                           # and a good call does write
    torch.cuda.synchronize()
    assert not bool((out[0] == 0x44).all()) and not bool((out[1] == 0x44).all())
    m.close()


def test_auto_resolves_each_way(dev):
    import fldr_scale as K
    fmt = _fmt("nv12", 8)
    for in_size, out_size, want in (((64, 64), (96, 96), K.AFTER), ((96, 96), (64, 64), K.BEFORE), ((64, 96), (96, 64), K.AFTER)):
        m = K.Map(in_size, out_size, fmt, K.BILINEAR, K.AUTO)
        assert m.where == want == O.where(O.AUTO, in_size, out_size)
        m.close()
        for forced in (K.BEFORE, K.AFTER):
            m = K.Map(in_size, out_size, fmt, K.BILINEAR, forced)
            assert m.where == forced
            m.close()
        c = K.Scaler(None, in_size, out_size, fmt, 25, 25, K.BILINEAR, K.AUTO, device=dev.index or 0)       # B == 1: no model needed to ask
        assert c.where == want and c.cfg.where == want
        c.close()


# ---- fldr_scale_forward -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nm(dev):
    import fldr_harness as Hn
    import fldr_model
    m = fldr_model.NativeModel.from_npz(Hn.DEFAULT_WEIGHTS, device=dev.index or 0)
    yield m
    m.close()


@functools.lru_cache(maxsize=None)
def _small_frames(layout, depth):
    return CF.real_frames(layout, depth)[:6]


@functools.lru_cache(maxsize=None)
def _big_frames(layout, depth):
    """The frames of cadence_frames enlarged to BIG by the oracle (bicubic): the 384 x 672 material of the BEFORE tests, cut included."""
    import fldr_scale as K
    t = K.tables((CF.H, CF.W), BIG, K.BICUBIC)
    return [O.scale(f, layout, depth, BIG, t) for f in _small_frames(layout, depth)]


def _dev_frame(planes, dev):
    out = []
    for p in planes:
        t = torch.from_numpy(p.view(np.int16) if p.dtype == np.uint16 else p).to(dev)
        out.append(t.view(torch.uint16) if p.dtype == np.uint16 else t)
    return tuple(out)


def _host(frame):
    return tuple(_np(p) for p in frame)


def _same_frame(a, b, what):
    for p, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and np.array_equal(x, y), (what, p)


def _reference_forward(nm, frames, t, fmt, scene):
    import fldr_rate as R
    import fldr_video as V
    if scene:
        ref, res = R.NativeRate(nm).forward(frames, t, fmt)
    else:
        ref, res = V.NativeVideo(nm).forward(frames, t, fmt, fmt), None
    torch.cuda.synchronize()
    return [_host(f) for f in ref], res


@pytest.mark.parametrize("layout,depth", [("nv12", 8), ("i420", 10)])
@pytest.mark.parametrize("scene", [True, False])
@pytest.mark.parametrize("where", [O.BEFORE, O.AFTER], ids=["before", "after"])
def test_forward_temporaries_and_outputs_are_the_composition(nm, dev, layout, depth, scene, where):
    import fldr_scale as K
    small, big = (CF.H, CF.W), BIG
    in_size, out_size = (big, small) if where == O.BEFORE else (small, big)
    fmt = _fmt(layout, depth)
    src = _big_frames(layout, depth) if where == O.BEFORE else _small_frames(layout, depth)
    filt = K.BICUBIC if where == O.BEFORE else K.LANCZOS3
    m = K.Map(in_size, out_size, fmt, filt, where)
    tabs = K.tables(in_size, out_size, filt)
    ns = K.NativeScale(nm)
    t = [0.2, 0.6]
    for pair, is_cut in (((0, 1), 0), ((CF.CUT_AT - 1, CF.CUT_AT), 1)):
        frames = [_dev_frame(src[i], dev) for i in pair]
        outs = [_dev_frame(_blank(layout, depth, out_size), dev) for _ in t]
        outs, temps, got = ns.forward(m, frames, t, outs, scene)
        torch.cuda.synchronize()
        assert (got["cut"] == is_cut) if scene else got is None
        if where == O.BEFORE:
            scaled = [O.scale(src[i], layout, depth, out_size, tabs) for i in pair]
            assert len(temps) == 2
            for k in range(2):
                _same_frame(_host(temps[k]), scaled[k], ("temp", pair, k))
            ref, res = _reference_forward(nm, [_dev_frame(f, dev) for f in scaled], t, fmt, scene)
            want = ref
        else:
            ref, res = _reference_forward(nm, frames, t, fmt, scene)
            assert len(temps) == len(t)
            for k in range(len(t)):
                _same_frame(_host(temps[k]), ref[k], ("temp", pair, k))
            want = [O.scale(f, layout, depth, out_size, tabs) for f in ref]
        assert (res == got) if scene else res is None
        for k in range(len(t)):
            _same_frame(_host(outs[k]), want[k], ("out", pair, k))
    m.close()


def test_bad_forward_calls_leave_the_outputs_untouched(nm, dev):
    import fldr_scale as K
    import fldr_video as V
    layout, depth = "nv12", 8
    in_size, out_size = (CF.H, CF.W), BIG
    fmt = _fmt(layout, depth)
    real = _small_frames(layout, depth)
    frames = [_dev_frame(real[i], dev) for i in (0, 1)]
    ns = K.NativeScale(nm)
    m = K.Map(in_size, out_size, fmt, K.BILINEAR, K.AFTER)
    out = tuple(torch.full(s, 0x44, dtype=torch.uint8, device=dev) for s in V.plane_shapes(layout, out_size[0], out_size[1]))
    ws = ns.workspace(m, 2)
    tt = ns._t([0.25, 0.75])
    make = lambda: ns.make_scale_io(m, frames, tt, [out, out], True, None)
    assert ns.forward_raw(m, make(), ws, ws_bytes=ws.numel() - 1) == K.E_ARG                   # a short workspace
    assert ns.forward_raw(m, make(), ws[256:]) == K.E_ARG
    assert ns.forward_raw(m, make(), None) == K.E_ARG
    assert ns.forward_raw(m, make(), ws, model=False) == K.E_ARG
    assert ns.forward_raw(None, make(), ws) == K.E_STATE
    io = make()
    io.reserved[2] = 1
    assert ns.forward_raw(m, io, ws) == K.E_ARG
    io = make()
    io.v.H = in_size[0] - 2                                                 # not the map's in size
    assert ns.forward_raw(m, io, ws) == K.E_ARG
    io = make()
    io.v.out_format = _fmt("i420", 8)
    assert ns.forward_raw(m, io, ws) == K.E_FORMAT
    io = make()
    io._keep_out[1].pitch[1] = out_size[1] - 2
    assert ns.forward_raw(m, io, ws) == V.E_PITCH
    oh, ow = out_size
    inside = (ws[4096:4096 + oh * ow].view(oh, ow), ws[1 << 20:(1 << 20) + oh * ow // 2].view(oh // 2, ow))       # an output inside the workspace
    io = ns.make_scale_io(m, frames, tt, [out, inside], True, None)
    assert ns.forward_raw(m, io, ws) == K.E_ARG
    torch.cuda.synchronize()
    assert all(bool((p == 0x44).all()) for p in out)
    m.close()


# ---- the stream ----------------------------------------------------------------------------------------------------------------------------
def _same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for n, (a, b) in enumerate(zip(got, want)):
        _same_frame(a, b, "%s, frame %d" % (what, n))


@pytest.mark.parametrize("layout,depth,scene", [("nv12", 8, True), ("i420", 10, True), ("nv12", 8, False)])
@pytest.mark.parametrize("where", [O.BEFORE, O.AFTER], ids=["before", "after"])
def test_stream_equals_the_converter_and_the_oracle(nm, dev, layout, depth, scene, where):
    """24 -> 60 over five frames with the cut inside; the flush returns the output that lands on the last one.  BEFORE (384 x 672 -> 256 x 448): the outputs of a fldr_rate.Converter at the OUT size
    pushed the oracle's scaled frames.  AFTER (256 x 448 -> 384 x 672): the oracle's scale of the outputs of a Converter at the IN size —
    the outputs that are an input frame's own bytes and the ones the cut replaced included."""
    import fldr_rate as R
    import fldr_scale as K
    small, big = (CF.H, CF.W), BIG
    in_size, out_size = (big, small) if where == O.BEFORE else (small, big)
    fmt = _fmt(layout, depth)
    frames = (_big_frames(layout, depth) if where == O.BEFORE else _small_frames(layout, depth))[:5]
    assert 0 < CF.CUT_AT < len(frames) - 1
    filt = K.BICUBIC
    tabs = K.tables(in_size, out_size, filt)
    scale = lambda f: O.scale(f, layout, depth, out_size, tabs)
    ref = R.Converter(nm, small[0], small[1], fmt, 24, 60, scene=scene)
    want, scenes = [], []
    for f in frames:
        outs = ref.push(scale(f) if where == O.BEFORE else f)
        want.append(outs if where == O.BEFORE else [scale(o) for o in outs])
        scenes.append(ref.last_scene)
    outs = ref.flush()
    want.append(outs if where == O.BEFORE else [scale(o) for o in outs])
    ref.close()
    assert [len(w) for w in want] == [0, 3, 2, 3, 2, 1] and sum(s["cut"] for s in scenes) == (1 if scene else 0)
    c = K.Scaler(nm, in_size, out_size, fmt, 24, 60, filt, where, scene)
    assert c.where == where and c.max_out == R.max_out(24, 60) == 3
    for f in frames[2:4]:                                                   # two frames of some other stream, forgotten by the reset
        c.push(f)
    c.reset()
    for n, f in enumerate(frames):
        _same(c.push(f), want[n], "push %d" % n)
        assert c.last_scene == scenes[n], (n, c.last_scene, scenes[n])
    _same(c.flush(), want[-1], "flush")
    assert c.flush() == []                                                  # a second flush returns none
    c.close()


@pytest.mark.parametrize("layout,depth,in_size,out_size,filt", [("i420", 10, (CF.H, CF.W), (144, 255), O.LANCZOS3),
                                                                ("nv12", 8, (CF.H, CF.W), (301, 500), O.BICUBIC)])
def test_stream_with_equal_rates_needs_no_model(dev, layout, depth, in_size, out_size, filt):
    """B == 1: every output is an input frame scaled.  No model, no workspace, no forward: a pure scaling stream, both placements the same."""
    import fldr_scale as K
    fmt = _fmt(layout, depth)
    frames = _small_frames(layout, depth)[:4]
    tabs = K.tables(in_size, out_size, filt)
    want = [O.scale(f, layout, depth, out_size, tabs) for f in frames]
    for where in (K.AUTO, K.BEFORE, K.AFTER):
        c = K.Scaler(None, in_size, out_size, fmt, (30000, 1001), (30000, 1001), filt, where, device=dev.index or 0)
        assert c.max_out == 1 and c.where == O.where(where, in_size, out_size)
        for n, f in enumerate(frames):
            _same(c.push(f), want[n - 1:n] if n else [], "push %d" % n)
        _same(c.flush(), want[-1:], "flush")
        assert c.flush() == []
        c.reset()                                                           # after a flush and a reset the object is a fresh stream
        assert c.push(frames[1]) == []
        _same(c.push(frames[0]), want[1:2], "after the reset")
        c.close()
