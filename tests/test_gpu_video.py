"""The video API (libfldr_video.so through fldr_video.NativeVideo / Session) on the GPU.  Every comparison is exact: the input
kernel gives the oracle's BGR frames (tests/yuv_oracle.py), the forward on a YUV pair gives the model's bytes on those frames, and
the output kernel gives the oracle's YUV of the model's planar output — for NV12 and I420, both matrices and both ranges, at odd
sizes and 4K, with pitched planes, on several streams, under a graph capture, through a session and through the C example."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import yuv_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fldr-vfi_amd")
SIZES = [(256, 256), (201, 333), (1080, 1920), (2160, 3840), (2160, 4096)]
FORMATS = [(m, r) for m in O.MATRICES for r in O.RANGES]


@pytest.fixture(scope="module")
def nv(dev):
    import fldr_harness as Hn
    import fldr_model
    import fldr_video
    nm = fldr_model.NativeModel.from_npz(Hn.DEFAULT_WEIGHTS, device=dev.index or 0)
    v = fldr_video.NativeVideo(nm)
    yield v
    nm.close()


@functools.lru_cache(maxsize=2)
def _yuv_pair(H, W, mat, rng, seed=0):
    """((Y, U, V), (Y, U, V)) of a synthetic pair, and the oracle's BGR frames [2,3,H,W] of those planes."""
    import fldr_harness as Hn
    u8 = Hn.synthetic_pair(H, W, seed=seed).numpy()
    yuv = [O.bgr_to_yuv420(u8[i], mat, rng) for i in range(2)]
    bgr = np.stack([O.yuv420_to_bgr(*yuv[i], mat, rng) for i in range(2)])
    return yuv, bgr


def _planes(yuv, layout):
    Y, U, V = yuv
    return O.pack_nv12(Y, U, V) if layout == "nv12" else (Y, U, V)


def _to_dev(planes, dev, pad=0, fill=0, offset=0):
    """Device copies of host planes; pad > 0: each plane a view into a buffer `pad` bytes wider per row (gap bytes = fill), starting
    `offset` bytes into it."""
    out = []
    for p in planes:
        r, c = p.shape
        if not pad and not offset:
            out.append(torch.from_numpy(np.ascontiguousarray(p)).to(dev))
            continue
        pitch = c + pad
        buf = torch.full((r * pitch + offset + pitch,), fill, dtype=torch.uint8, device=dev)
        view = buf[offset:offset + r * pitch].view(r, pitch)[:, :c]
        view.copy_(torch.from_numpy(np.ascontiguousarray(p)).to(dev))
        out.append(view)
    return tuple(out)


def _host(frame):
    return tuple(p.cpu().numpy() for p in frame)


def _yuv_of(frame, layout):
    h = _host(frame)
    return (h[0],) + tuple(O.unpack_nv12(h[1])) if layout == "nv12" else h


def _fmt(layout, mat, rng):
    import fldr_video
    return fldr_video.Format(layout, mat, rng)


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("mat,rng", FORMATS)
def test_yuv_forward_equals_model_on_oracle_bgr(nv, dev, H, W, mat, rng):
    yuv, bgr = _yuv_pair(H, W, mat, rng)
    ref = nv.model.interpolate_u8(torch.from_numpy(bgr)[None].to(dev), [0.5])[0].cpu().numpy()
    for layout in ("nv12", "i420"):
        frames = [_to_dev(_planes(yuv[i], layout), dev) for i in range(2)]
        fmt = _fmt(layout, mat, rng)
        ws = nv.workspace(H, W, 1)
        outs = nv.forward(frames, [0.5], fmt, fmt, ws=ws)
        torch.cuda.synchronize()
        pair, planar = nv.planar(ws, H, W, 1)
        assert np.array_equal(pair.cpu().numpy(), bgr), layout            # the input kernel: the oracle's BGR frames
        got = planar[0].cpu().numpy()
        assert np.array_equal(got, ref), layout                           # the forward: the model's bytes on those frames
        want = O.bgr_to_yuv420(got, mat, rng)                             # the output kernel: the oracle's YUV of them
        for g, w in zip(_yuv_of(outs[0], layout), want):
            assert np.array_equal(g, w), layout


@pytest.mark.parametrize("H,W,n_t,fin,fout", [(256, 256, 7, ("nv12", "bt709", "limited"), ("i420", "bt601", "full")),
                                              (201, 333, 7, ("i420", "bt601", "limited"), ("nv12", "bt709", "full")),
                                              (1080, 1920, 1, ("nv12", "bt601", "full"), ("i420", "bt709", "limited")),
                                              (2160, 3840, 7, ("nv12", "bt709", "limited"), ("nv12", "bt709", "limited"))])
def test_outputs_equal_oracle_downsampling_of_model_output(nv, dev, H, W, n_t, fin, fout):
    yuv, _ = _yuv_pair(H, W, fin[1], fin[2], seed=1)
    frames = [_to_dev(_planes(yuv[i], fin[0]), dev) for i in range(2)]
    t = [(k + 1) / (n_t + 1) for k in range(n_t)]
    ws = nv.workspace(H, W, n_t)
    outs = nv.forward(frames, t, _fmt(*fin), _fmt(*fout), ws=ws)
    torch.cuda.synchronize()
    _, planar = nv.planar(ws, H, W, n_t)
    for k in range(n_t):
        want = O.bgr_to_yuv420(planar[k].cpu().numpy(), fout[1], fout[2])
        for g, w in zip(_yuv_of(outs[k], fout[0]), want):
            assert np.array_equal(g, w), k
    assert not np.array_equal(planar[0].cpu().numpy(), planar[n_t - 1].cpu().numpy()) or n_t == 1


@pytest.mark.parametrize("H,W,pad,offset", [(256, 256, 64, 0), (201, 333, 13, 5), (1080, 1920, 128, 4096)])
@pytest.mark.parametrize("layout", ["nv12", "i420"])
def test_pitched_planes_read_and_write_nothing_outside_the_rows(nv, dev, H, W, pad, offset, layout):
    import fldr_video
    mat, rng = "bt601", "limited"
    yuv, _ = _yuv_pair(H, W, mat, rng, seed=2)
    fmt = _fmt(layout, mat, rng)
    tight = nv.forward([_to_dev(_planes(yuv[i], layout), dev) for i in range(2)], [0.5], fmt, fmt)
    results = []
    odd = offset % 4 != 0                     # odd offsets and pitches: the byte path; 4-byte aligned ones: the 4-bytes-per-lane path
    for fill in (0xA5, 0x00):
        frames = [_to_dev(_planes(yuv[i], layout), dev, pad=pad, fill=fill, offset=offset + (3 if odd else 256) * i) for i in range(2)]
        outs = [_to_dev([np.zeros(s, np.uint8) for s in fldr_video.plane_shapes(layout, H, W)], dev, pad=pad + (3 if odd else 0), fill=0x5A,
                        offset=offset)]
        for p in outs[0]:
            p.fill_(0)
        nv.forward(frames, [0.5], fmt, fmt, outs=outs)
        torch.cuda.synchronize()
        for p in outs[0]:
            base = p.as_strided((p.shape[0], p.stride(0)), p.stride())   # the rows with their gaps
            assert bool((base[:, p.shape[1]:] == 0x5A).all()), "a gap byte of an output plane was written"
        results.append(_host(outs[0]))
    for a, b, c in zip(results[0], results[1], _host(tight[0])):
        assert np.array_equal(a, b) and np.array_equal(a, c)                # gap bytes have no effect; pitches give the tight bytes


def test_three_streams_give_the_bytes_of_one_pair_at_a_time(nv, dev):
    H, W, NS, NP = 2160, 3840, 3, 4
    fmt = _fmt("nv12", "bt709", "limited")
    pairs = []
    for p in range(NP):
        yuv, _ = _yuv_pair(H, W, "bt709", "limited", seed=10 + p)
        pairs.append([_to_dev(_planes(yuv[i], "nv12"), dev) for i in range(2)])
    t = torch.tensor([0.5], device=dev)
    refs = []
    for p in range(NP):
        refs.append(nv.forward(pairs[p], t, fmt, fmt))
        torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=dev) for _ in range(NS)]
    wss = [nv.workspace(H, W) for _ in range(NS)]
    got = []
    torch.cuda.synchronize()
    for i in range(3 * NP):
        with torch.cuda.stream(streams[i % NS]):
            got.append((i % NP, nv.forward(pairs[i % NP], t, fmt, fmt, ws=wss[i % NS])))
    torch.cuda.synchronize()
    for k, o in got:
        for a, b in zip(o[0], refs[k][0]):
            assert torch.equal(a, b), k


def test_graph_capture_replays_the_eager_bytes_and_reads_t_at_replay(nv, dev):
    H, W = 256, 384
    fmt = _fmt("i420", "bt709", "full")
    yuv, _ = _yuv_pair(H, W, "bt709", "full", seed=4)
    frames = [_to_dev(_planes(yuv[i], "i420"), dev) for i in range(2)]
    t = torch.tensor([0.5], device=dev)
    ws = nv.workspace(H, W)
    import fldr_video
    outs = [fldr_video.empty_frame(fmt, H, W, dev)]
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        nv.forward(frames, t, fmt, fmt, outs=outs, ws=ws)                  # warm
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        nv.forward(frames, t, fmt, fmt, outs=outs, ws=ws)
    seen = []
    for tv in (0.5, 0.2, 0.9):
        t.fill_(tv)
        g.replay()
        torch.cuda.synchronize()
        eager = nv.forward(frames, [tv], fmt, fmt)
        torch.cuda.synchronize()
        for a, b in zip(outs[0], eager[0]):
            assert torch.equal(a, b), tv
        seen.append(_host(outs[0])[0])
    assert not np.array_equal(seen[1], seen[2])


def _clip(H, W, n, seed=5):
    """n frames of a texture moving 4 px down and 6 px right per frame (BGR planar numpy)."""
    import fldr_harness as Hn
    base = Hn.synthetic_pair(H + 4 * n, W + 6 * n, seed=seed).numpy()[0]
    return [np.ascontiguousarray(base[:, 4 * k:4 * k + H, 6 * k:6 * k + W]) for k in range(n)]


def test_session_pushes_equal_forwards_on_consecutive_frames(nv, dev):
    import fldr_video
    H, W, n_t = 1080, 1920, 3
    fin, fout = _fmt("i420", "bt709", "limited"), _fmt("nv12", "bt709", "limited")
    frames = [O.bgr_to_yuv420(f, "bt709", "limited") for f in _clip(H, W, 5)]
    s = fldr_video.Session(nv.model, H, W, n_t, fin, fout)
    counts, prev = [], None
    t = [(k + 1) / (n_t + 1) for k in range(n_t)]
    for f in frames:
        outs = s.push(_planes(f, "i420"))
        counts.append(len(outs))
        if prev is not None:
            ref = nv.forward([_to_dev(_planes(prev, "i420"), dev), _to_dev(_planes(f, "i420"), dev)], t, fin, fout)
            torch.cuda.synchronize()
            for k in range(n_t):
                for a, b in zip(outs[k], _host(ref[k])):
                    assert np.array_equal(a, b), k
        prev = f
    assert counts == [0, 3, 3, 3, 3]
    s.reset()
    assert s.push(_planes(frames[0], "i420")) == [] and s.last_n_out == 0
    assert len(s.push(_planes(frames[1], "i420"))) == n_t
    s.close()


def test_c_example_writes_inputs_and_session_outputs(nv, dev, clean_launcher, tmp_path):
    import fldr_harness as Hn
    import fldr_video
    H, W, F = 256, 448, 2
    frames = [O.bgr_to_yuv420(f, "bt709", "limited") for f in _clip(H, W, 4, seed=6)]
    raw = [O.i420_bytes(*f) for f in frames]
    (tmp_path / "in.yuv").write_bytes(b"".join(raw))
    exe = os.path.join(ROOT, "examples", "fldr_slowmo")
    if not os.path.exists(exe):
        exe = str(tmp_path / "fldr_slowmo")
        subprocess.run([shutil.which("cc") or "gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "examples", "fldr_slowmo.c"), "-L" + PKG, "-l:libfldr_video.so", "-l:libfldr_model.so",
                        "-Wl,-rpath," + PKG], check=True)
    cmd = '"%s" "%s" %d %d %d < "%s" > "%s"' % (exe, Hn.DEFAULT_WEIGHTS, W, H, F, tmp_path / "in.yuv", tmp_path / "out.yuv")
    r = clean_launcher(["sh", "-c", cmd], env=dict(os.environ), timeout=300)
    assert r["rc"] == 0, r
    data = (tmp_path / "out.yuv").read_bytes()
    n = len(raw[0])
    assert len(data) == 7 * n
    got = [data[k * n:(k + 1) * n] for k in range(7)]
    for k in range(4):
        assert got[2 * k] == raw[k], k
    fmt = _fmt("i420", "bt709", "limited")
    s = fldr_video.Session(nv.model, H, W, F - 1, fmt, fmt)
    s.push(_planes(frames[0], "i420"))
    for k in range(1, 4):
        outs = s.push(_planes(frames[k], "i420"))
        assert got[2 * k - 1] == b"".join(p.tobytes() for p in outs[0]), k
    s.close()


def test_bad_calls_return_their_code_and_enqueue_nothing(nv, dev):
    import fldr_video as V
    H, W = 256, 256
    fmt = _fmt("nv12", "bt601", "limited")
    yuv, _ = _yuv_pair(H, W, "bt601", "limited", seed=7)
    frames = [_to_dev(_planes(yuv[i], "nv12"), dev) for i in range(2)]
    t = torch.tensor([0.5], device=dev)
    ws = nv.workspace(H, W)
    ws.fill_(0x33)
    outs = [tuple(p.fill_(0x77) for p in V.empty_frame(fmt, H, W, dev))]

    def call(mutate, ws_=ws):
        io = nv.make_io(frames, t, fmt, fmt, outs, H, W)
        mutate(io)
        return nv.forward_io(io, ws_)
    cases = [
        (lambda io: setattr(io.in_format, "layout", 5), V.E_FORMAT),
        (lambda io: setattr(io.out_format, "matrix", 2), V.E_FORMAT),
        (lambda io: io.in_format.reserved.__setitem__(2, 1), V.E_FORMAT),
        (lambda io: io.in_[1].pitch.__setitem__(0, W - 1), V.E_PITCH),
        (lambda io: io.out[0].pitch.__setitem__(1, W - 2), V.E_PITCH),
        (lambda io: io.in_[0].plane.__setitem__(1, None), V.E_PLANE),
        (lambda io: setattr(io, "n_t", 0), V.E_ARG),
        (lambda io: setattr(io, "H", 1), V.E_ARG),
    ]
    for mutate, code in cases:
        assert call(mutate) == code
    assert call(lambda io: None, ws_=ws[:1024]) == V.E_WORKSPACE
    assert call(lambda io: None, ws_=ws[1:]) == V.E_WORKSPACE                 # not 256-byte aligned
    torch.cuda.synchronize()
    assert bool((ws == 0x33).all()), "a refused call wrote the workspace"
    for p in outs[0]:
        assert bool((p == 0x77).all()), "a refused call wrote an output"
    assert call(lambda io: None) == 0                                         # and the same call, valid, works
    torch.cuda.synchronize()
    assert not bool((outs[0][0] == 0x77).all())
