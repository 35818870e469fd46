"""The RGB API (libfldr_rgb.so through fldr_rgb.NativeRgb / Session) on the GPU.  Every comparison is exact: the input kernel leaves
the oracle's planar BGR frames (tests/rgb_oracle.py) in the workspace, the forward gives the model's bytes on those frames, the output
kernel gives the oracle's frame of the model's planar output, the colour bytes of BGRA / RGBA equal the model's own interleaved 8-bit
forward on the same pixels, and alpha is the oracle's rule on the inputs' alpha — for every layout and depth, mixed formats, several
outputs, pitched planes, two streams, under a graph capture, through a session and through the C example.  The forwards run at 64 x 64
and 66 x 70 on a model of three pyramid scales (the shipped six-level configuration pads to multiples of 256 and takes no frame below
129 x 129); the C example creates the shipped configuration, so its frames are 130 x 134."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import rgb_oracle as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fldr-vfi_amd")
SIZES = [(64, 64), (66, 70)]
IDS = ["%s-%d" % f for f in R.FORMATS]
MARK = 0x5A


@pytest.fixture(scope="module")
def nm(dev):
    import fldr_harness as Hn
    import fldr_model
    m = fldr_model.NativeModel.from_npz(Hn.DEFAULT_WEIGHTS, device=dev.index or 0, test_scales=3)
    yield m
    m.close()


@pytest.fixture(scope="module")
def nr(nm):
    import fldr_rgb
    return fldr_rgb.NativeRgb(nm)


def _fmt(layout, depth, alpha="opaque"):
    import fldr_rgb as V
    return V.Format(layout, depth, alpha)


@functools.lru_cache(maxsize=None)
def _bgr_pair(H, W, depth, seed=0):
    """fldr_harness.synthetic_pair as planar BGR code values [2,3,H,W]: uint8, or at depth 10 uint16 (the 8-bit value with its top two
    bits repeated below).  Shared: never written."""
    import fldr_harness as Hn
    u8 = np.array(Hn.synthetic_pair(H, W, seed=seed).numpy()).reshape(2, 3, H, W)
    out = u8 if depth == 8 else (u8.astype(np.uint16) << 2) | (u8 >> 6)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _alpha_pair(H, W, bits, seed=0, extreme=False):
    """The alpha planes of the two inputs: seeded noise over the whole range, or a0 = the largest code everywhere and a1 = 0."""
    top = (1 << bits) - 1
    if extreme:
        out = np.stack([np.full((H, W), top), np.zeros((H, W), np.int64)])
    else:
        out = np.random.default_rng(1000 + seed).integers(0, top + 1, (2, H, W))
    out.setflags(write=False)
    return out


def _to_dev(frame, dev, pad=0, fill=0, offset=0):
    """A device copy of a host frame; pad / offset (bytes): every plane a view into a byte buffer `pad` bytes wider per row (gap bytes =
    fill), starting `offset` bytes into it.  -> (frame, buffers)."""
    planes, bufs = [], []
    for plane in frame:
        r, c = plane.shape
        rb = c * plane.itemsize
        pitch = rb + pad
        buf = torch.full((offset + r * pitch + 32,), fill, dtype=torch.uint8, device=dev)
        v = buf[offset:offset + r * pitch].view(r, pitch)[:, :rb]
        v.copy_(torch.from_numpy(np.ascontiguousarray(plane).view(np.uint8).reshape(r, rb)).to(dev))
        planes.append(v.view({1: torch.uint8, 2: torch.uint16, 4: torch.uint32}[plane.itemsize]))
        bufs.append(buf)
    return tuple(planes), bufs


def _host(frame):
    """The planes of a device frame as numpy arrays (through their bytes: pitched views too)."""
    out = []
    for p in frame:
        r, n = p.shape
        b = np.ascontiguousarray(p.view(torch.uint8).cpu().numpy())
        out.append(b.view({torch.uint8: np.uint8, torch.uint16: np.uint16, torch.uint32: np.uint32}[p.dtype]).reshape(r, n))
    return tuple(out)


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _inputs(H, W, fin, seed=0, extreme=False):
    """The two host frames in fin = (layout, depth) of the synthetic pair, their alpha the seeded planes where the layout has alpha."""
    layout, depth = fin
    bgr = _bgr_pair(H, W, depth, seed)
    bits = R.alpha_bits(layout, depth)
    alpha = _alpha_pair(H, W, bits, seed, extreme) if bits else (None, None)
    return [R.pack(layout, depth, *bgr[i], alpha[i]) for i in range(2)], alpha


def _model(nr, dev, pair, t, depth_out):
    """fldr_model_forward in its planar forms on a host pair [2,3,H,W] (uint8 -> U8_PLANAR, uint16 -> U10_PLANAR) -> [n_t,3,H,W]."""
    out = nr.model.interpolate_u10(torch.from_numpy(np.ascontiguousarray(pair))[None].to(dev), t, out="u10" if depth_out == 10 else "u8")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check_forward(nr, dev, H, W, fin, fout, t, policy="opaque", seed=0, extreme=False):
    """The properties of one forward; fin / fout: (layout, depth).  -> (the output frames on the host, the planar outputs)."""
    host_in, alpha = _inputs(H, W, fin, seed, extreme)
    ws = nr.workspace(H, W, len(t))
    outs = nr.forward([_to_dev(f, dev)[0] for f in host_in], t, _fmt(*fin), _fmt(*fout, policy), ws=ws)
    torch.cuda.synchronize()
    pair, planar = nr.planar(ws, H, W, len(t), fin[1], fout[1])
    want_pair = np.stack([R.planar_bgr(*fin, f) for f in host_in])
    assert np.array_equal(pair.cpu().numpy(), want_pair), (fin, "pair")       # the input kernel: the oracle's planar frames
    got = np.stack([p.cpu().numpy() for p in planar])
    assert np.array_equal(got, _model(nr, dev, want_pair, t, fout[1])), (fin, fout, "model")     # the forward: the model's bytes on them
    frames = []
    for k in range(len(t)):                                                    # the output kernel + alpha: the oracle's frame of them
        a = R.alpha_of(policy, alpha[0], alpha[1], t[k]) if R.alpha_bits(*fout) else None
        want = R.pack(*fout, *got[k], a)
        frames.append(_host(outs[k]))
        assert _same(frames[k], want), (fin, fout, policy, k)
    return frames, got


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("layout,depth", R.FORMATS, ids=IDS)
def test_forward_equals_model_on_oracle_planar(nr, dev, H, W, layout, depth):
    _check_forward(nr, dev, H, W, (layout, depth), (layout, depth), [0.5])


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("layout,order", [("bgra", "bgr"), ("rgba", "rgb")])
def test_bgra_colour_bytes_equal_the_interleaved_model_forward(nr, dev, H, W, layout, order):
    """The three colour bytes of every pixel are those of fldr_model_forward with IN_U8_INTERLEAVED / OUT_U8_INTERLEAVED on the same
    pixels as 3-byte frames: a path that shares no converter with this library."""
    host_in, _ = _inputs(H, W, (layout, 8))
    outs = nr.forward([_to_dev(f, dev)[0] for f in host_in], [0.5], _fmt(layout, 8))
    torch.cuda.synchronize()
    px = [f[0].reshape(H, W, 4) for f in host_in]
    assert all((p[:, :, 3] != 255).any() for p in px)                          # the inputs' alpha is noise; the output's is opaque
    pair = [torch.from_numpy(np.ascontiguousarray(p[:, :, :3])).to(dev) for p in px]
    ref = nr.model.interpolate_u8(pair=pair, t=[0.5], order=order, out_layout="hwc")
    torch.cuda.synchronize()
    got = _host(outs[0])[0].reshape(H, W, 4)
    assert np.array_equal(got[:, :, :3], ref.cpu().numpy()[0]), layout
    assert (got[:, :, 3] == 255).all()


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("fin,fout", [(("bgra", 8), ("x2rgb10", 10)), (("x2bgr10", 10), ("gbrap", 10)), (("gbrp", 10), ("argb", 8)),
                                      (("abgr", 8), ("gbrp", 8))])
def test_mixed_formats(nr, dev, H, W, fin, fout):
    """In and out formats are independent: layouts, depths (the model's any-in-any-out planar forward) and the presence of alpha."""
    _check_forward(nr, dev, H, W, fin, fout, [0.5], seed=1)


T3 = [0.25, 0.5, 0.75]
ALPHA_CASES = [(("bgra", 8), ("bgra", 8)), (("x2rgb10", 10), ("x2rgb10", 10)), (("gbrap", 10), ("gbrap", 10)), (("gbrap", 8), ("gbrap", 8)),
               (("argb", 8), ("gbrap", 8)), (("gbrap", 8), ("rgba", 8)), (("abgr", 8), ("bgra", 8)), (("x2bgr10", 10), ("x2rgb10", 10))]


@pytest.mark.parametrize("policy", ["nearer", "blend"])
@pytest.mark.parametrize("fin,fout", ALPHA_CASES, ids=["%s%d-%s%d" % (a + b) for a, b in ALPHA_CASES])
def test_alpha_is_the_oracles_and_colour_is_that_of_the_opaque_run(nr, dev, fin, fout, policy):
    """n_t = 3 at t = (0.25, 0.5, 0.75) on inputs whose alpha is seeded noise, at a size the wide form takes and one it does not; the
    colour values of every output are those of the OPAQUE run, whose alpha is the largest code."""
    for H, W in SIZES:
        frames, got = _check_forward(nr, dev, H, W, fin, fout, T3, policy, seed=2)
        opaque, got_o = _check_forward(nr, dev, H, W, fin, fout, T3, "opaque", seed=2)
        assert np.array_equal(got, got_o)
        differs = False
        for k in range(3):
            fb, fo = R.unpack(*fout, frames[k]), R.unpack(*fout, opaque[k])
            assert all(np.array_equal(x, y) for x, y in zip(fb[:3], fo[:3])), k
            assert (fo[3] == R.alpha_max(*fout)).all()
            differs = differs or not np.array_equal(fb[3], fo[3])
        assert differs


@pytest.mark.parametrize("fin,fout", [(("bgra", 8), ("bgra", 8)), (("argb", 8), ("gbrap", 8)), (("gbrap", 10), ("gbrap", 10)),
                                      (("x2rgb10", 10), ("x2bgr10", 10))])
def test_alpha_from_the_largest_code_to_zero(nr, dev, fin, fout):
    """a0 = the largest code, a1 = 0: BLEND gives the header's worked numbers at 8 bits (191, 128, 64), NEARER a0, a1, a1."""
    H, W = 66, 70
    top = R.alpha_max(*fout)
    frames, _ = _check_forward(nr, dev, H, W, fin, fout, T3, "blend", seed=3, extreme=True)
    values = [np.unique(R.unpack(*fout, f)[3]).tolist() for f in frames]
    assert values == [[(top * 49152 + 32768) >> 16], [(top * 32768 + 32768) >> 16], [(top * 16384 + 32768) >> 16]]
    if top == 255:
        assert values == [[191], [128], [64]]
    frames, _ = _check_forward(nr, dev, H, W, fin, fout, T3, "nearer", seed=3, extreme=True)
    assert [np.unique(R.unpack(*fout, f)[3]).tolist() for f in frames] == [[top], [0], [0]]


def test_unequal_alpha_widths_are_refused_by_the_forward(nr, dev):
    import fldr_rgb as V
    H, W = 64, 64
    host_in, _ = _inputs(H, W, ("bgra", 8))
    frames = [_to_dev(f, dev)[0] for f in host_in]
    for fout in (("x2rgb10", 10), ("gbrap", 10)):
        with pytest.raises(V.RgbError) as e:
            nr.forward(frames, [0.5], _fmt("bgra", 8), _fmt(*fout, "blend"))
        assert e.value.code == V.E_FORMAT
    nr.forward(frames, [0.5], _fmt("bgra", 8), _fmt("gbrp", 10, "blend"))      # nowhere to put alpha: the policy is ignored
    torch.cuda.synchronize()


@pytest.mark.parametrize("H,W,pad,offset", [(64, 64, 64, 0), (66, 70, 12, 4)])
@pytest.mark.parametrize("layout,depth,policy", [("bgra", 8, "blend"), ("x2rgb10", 10, "nearer"), ("gbrap", 10, "blend"), ("gbrp", 8, "opaque"),
                                                 ("argb", 8, "opaque")])
def test_pitched_and_offset_planes_give_the_tight_bytes_and_keep_the_gaps(nr, dev, H, W, pad, offset, layout, depth, policy):
    fin, fout = _fmt(layout, depth), _fmt(layout, depth, policy)
    host_in, _ = _inputs(H, W, (layout, depth), seed=3)
    tight = _host(nr.forward([_to_dev(f, dev)[0] for f in host_in], [0.5], fin, fout)[0])
    results = []
    for fill in (0xA5, 0x00):
        frames = [_to_dev(f, dev, pad=pad, fill=fill, offset=offset)[0] for f in host_in]
        zero = tuple(np.zeros_like(p) for p in host_in[0])
        opad = pad + (4 if offset else 0)
        out, bufs = _to_dev(zero, dev, pad=opad, fill=MARK, offset=offset)
        nr.forward(frames, [0.5], fin, fout, outs=[out])
        torch.cuda.synchronize()
        planes = []
        for buf, z in zip(bufs, zero):
            rb = z.shape[1] * z.itemsize
            pitch = rb + opad
            b = buf.cpu().numpy()
            keep = np.ones(b.shape, bool)
            rows = np.empty((H, rb), np.uint8)
            for y in range(H):
                rows[y] = b[offset + y * pitch:offset + y * pitch + rb]
                keep[offset + y * pitch:offset + y * pitch + rb] = False
            assert (b[keep] == MARK).all(), "a byte outside the rows of an output plane was written"
            planes.append(rows.view(z.dtype))
        results.append(tuple(planes))
    assert _same(results[0], results[1]) and _same(results[0], tight)          # gaps have no effect; pitches give the tight bytes


def test_two_streams_with_two_workspaces_give_the_bytes_of_one(nr, dev):
    H, W = 64, 64
    fin, fout = _fmt("bgra", 8), _fmt("bgra", 8, "blend")
    pairs = [[_to_dev(f, dev)[0] for f in _inputs(H, W, ("bgra", 8), seed=10 + p)[0]] for p in range(2)]
    t = torch.tensor([0.5], device=dev)
    refs = []
    for p in range(2):
        refs.append(_host(nr.forward(pairs[p], t, fin, fout)[0]))
        torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    wss = [nr.workspace(H, W) for _ in range(2)]
    got = []
    torch.cuda.synchronize()
    for i in range(6):
        with torch.cuda.stream(streams[i % 2]):
            got.append((i % 2, nr.forward(pairs[i % 2], t, fin, fout, ws=wss[i % 2])))
    torch.cuda.synchronize()
    for k, o in got:
        assert _same(_host(o[0]), refs[k]), k
    assert not _same(refs[0], refs[1])


def test_graph_capture_replays_the_eager_bytes_and_reads_t_at_replay(nr, dev):
    """The colour and, under BLEND, the alpha follow a rewritten t."""
    import fldr_rgb as V
    H, W = 64, 64
    fin, fout = _fmt("argb", 8), _fmt("gbrap", 8, "blend")
    frames = [_to_dev(f, dev)[0] for f in _inputs(H, W, ("argb", 8), seed=4)[0]]
    t = torch.tensor([0.5], device=dev)
    ws = nr.workspace(H, W)
    outs = [V.empty_frame(fout, H, W, dev)]
    st = torch.cuda.Stream(device=dev)
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        nr.forward(frames, t, fin, fout, outs=outs, ws=ws)                    # warm
    st.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        nr.forward(frames, t, fin, fout, outs=outs, ws=ws)
    seen = []
    for tv in (0.3, 0.8):
        t.fill_(tv)
        g.replay()
        torch.cuda.synchronize()
        eager = nr.forward(frames, [tv], fin, fout)
        torch.cuda.synchronize()
        assert _same(_host(outs[0]), _host(eager[0])), tv
        seen.append(_host(outs[0]))
    assert not np.array_equal(seen[0][0], seen[1][0])                          # the colour (G plane) moved
    assert not np.array_equal(seen[0][3], seen[1][3])                          # and so did the alpha


def _clip(H, W, n, depth, seed=5):
    """n frames of a texture moving 4 px down and 6 px right per frame (planar BGR code values)."""
    base = _bgr_pair(H + 4 * n, W + 6 * n, depth, seed)[0]
    return [np.ascontiguousarray(base[:, 4 * k:4 * k + H, 6 * k:6 * k + W]) for k in range(n)]


@pytest.mark.parametrize("fin,fout,policy", [(("bgra", 8), ("bgra", 8), "blend"), (("argb", 8), ("gbrap", 8), "nearer"),
                                             (("x2rgb10", 10), ("gbrp", 8), "opaque")])
def test_session_pushes_equal_forwards_on_consecutive_frames(nr, dev, fin, fout, policy):
    import fldr_rgb as V
    H, W, n_t = 66, 70, 2
    ffin, ffout = _fmt(*fin), _fmt(*fout, policy)
    bits = R.alpha_bits(*fin)
    alphas = np.random.default_rng(6).integers(0, 1 << bits, (4, H, W))
    frames = [R.pack(*fin, *f, alphas[i]) for i, f in enumerate(_clip(H, W, 4, fin[1]))]
    s = V.Session(nr.model, H, W, n_t, ffin, ffout)
    counts, prev = [], None
    t = [(k + 1) / (n_t + 1) for k in range(n_t)]
    for f in frames:
        outs = s.push(f)
        counts.append(len(outs))
        if prev is not None:
            ref = nr.forward([_to_dev(prev, dev)[0], _to_dev(f, dev)[0]], t, ffin, ffout)
            torch.cuda.synchronize()
            for k in range(n_t):
                assert _same(outs[k], _host(ref[k])), k
        prev = f
    assert counts == [0, 2, 2, 2]
    s.reset()
    assert s.push(frames[0]) == [] and s.last_n_out == 0
    assert len(s.push(frames[1])) == n_t
    s.close()


def test_c_example_reproduces_the_session_on_a_bgra_stream(dev, clean_launcher, tmp_path):
    """Raw bgra frames through examples/fldr_slowmo_rgb with alpha=blend: the input frames come back byte for byte, the frames between
    them are the session's."""
    import fldr_harness as Hn
    import fldr_model
    import fldr_rgb as V
    H, W, F = 130, 134, 2
    alphas = np.random.default_rng(7).integers(0, 256, (3, H, W))
    frames = [R.pack("bgra", 8, *f, alphas[i]) for i, f in enumerate(_clip(H, W, 3, 8, seed=6))]
    raw = [f[0].tobytes() for f in frames]
    (tmp_path / "in.bgra").write_bytes(b"".join(raw))
    exe = os.path.join(ROOT, "examples", "fldr_slowmo_rgb")
    if not os.path.exists(exe):
        exe = str(tmp_path / "fldr_slowmo_rgb")
        subprocess.run([shutil.which("cc") or "gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "examples", "fldr_slowmo_rgb.c"), "-L" + PKG, "-l:libfldr_rgb.so", "-l:libfldr_model.so",
                        "-Wl,-rpath," + PKG], check=True)
    cmd = '"%s" "%s" %d %d %d bgra alpha=blend < "%s" > "%s"' % (exe, Hn.DEFAULT_WEIGHTS, W, H, F, tmp_path / "in.bgra", tmp_path / "out.bgra")
    r = clean_launcher(["sh", "-c", cmd], env=dict(os.environ), timeout=300)
    assert r["rc"] == 0, r
    data = (tmp_path / "out.bgra").read_bytes()
    n = len(raw[0])
    assert n == 4 * W * H and len(data) == 5 * n
    got = [data[k * n:(k + 1) * n] for k in range(5)]
    for k in range(3):
        assert got[2 * k] == raw[k], k
    fmt = _fmt("bgra", 8, "blend")
    shipped = fldr_model.NativeModel.from_npz(Hn.DEFAULT_WEIGHTS, device=dev.index or 0)
    s = V.Session(shipped, H, W, F - 1, fmt, fmt)
    s.push(frames[0])
    for k in range(1, 3):
        outs = s.push(frames[k])
        assert got[2 * k - 1] == outs[0][0].tobytes(), k
        assert np.array_equal(R.unpack("bgra", 8, outs[0])[3], R.alpha_blend(alphas[k - 1], alphas[k], 0.5)), k
    s.close()
    shipped.close()
