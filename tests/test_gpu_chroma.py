"""The 4:2:2 / 4:4:4 API (libfldr_chroma.so through fldr_chroma.NativeChroma / Session) on the GPU.  Every comparison is exact: the input
kernel leaves the oracle's BGR frames (tests/yuv_chroma_oracle.py) in the workspace, the forward gives the model's bytes on those frames,
and the output kernel gives the oracle's YUV of the model's planar output — for every container, mixed formats, several outputs, pitched
planes, two streams, under a graph capture, through a session and through the C example."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import yuv_chroma_oracle as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fldr-vfi_amd")
SIZES = [(256, 256), (201, 333)]
P210 = ("422", "semiplanar", 10)
CASES = [c + ("bt709", "limited") for c in C.containers()] + [P210 + (m, r) for m in C.MATRICES for r in C.RANGES if (m, r) != ("bt709", "limited")]


@pytest.fixture(scope="module")
def nc(dev):
    import fldr_harness as Hn
    import fldr_chroma
    import fldr_model
    nm = fldr_model.NativeModel.from_npz(Hn.DEFAULT_WEIGHTS, device=dev.index or 0)
    yield fldr_chroma.NativeChroma(nm)
    nm.close()


def _fmt(s, l, d, mat="bt709", rng="limited"):
    import fldr_chroma as V
    return V.Format(s, l, mat, rng, d)


@functools.lru_cache(maxsize=None)
def _bgr_pair(H, W, d, seed=0):
    """fldr_harness.synthetic_pair as code values of depth d: [2,3,H,W] (at depth 10 the 8-bit value with its top two bits repeated below)."""
    import fldr_harness as Hn
    u8 = Hn.synthetic_pair(H, W, seed=seed).numpy()
    return u8 if d == 8 else ((u8.astype(np.uint16) << 2) | (u8 >> 6))


@functools.lru_cache(maxsize=None)
def _yuv_pair(H, W, s, d, mat, rng, seed=0):
    """((Y, U, V), (Y, U, V)) of the synthetic pair converted by the oracle, and the oracle's BGR frames [2,3,H,W] of those planes."""
    src = _bgr_pair(H, W, d, seed)
    yuv = [C.bgr_to_yuv(src[i], s, mat, rng, d) for i in range(2)]
    bgr = np.stack([C.yuv_to_bgr(*yuv[i], s, mat, rng, d) for i in range(2)])
    return yuv, bgr


def _to_dev(planes, dev, pad=0, fill=0, offset=0):
    """Device copies of host planes; pad / offset (bytes): each plane a view into a byte buffer `pad` bytes wider per row (gap bytes = fill),
    starting `offset` bytes into it."""
    out = []
    for p in planes:
        r, c = p.shape
        rb = c * p.itemsize
        pitch = rb + pad
        buf = torch.full((offset + r * pitch + 32,), fill, dtype=torch.uint8, device=dev)
        v = buf[offset:offset + r * pitch].view(r, pitch)[:, :rb]
        v.copy_(torch.from_numpy(np.ascontiguousarray(p).view(np.uint8).reshape(r, rb)).to(dev))
        out.append(v.view(torch.uint16) if p.itemsize == 2 else v)
    return tuple(out)


def _frames(yuv, s, l, d, dev, **kw):
    return [_to_dev(C.pack(*yuv[i], s, l, d), dev, **kw) for i in range(2)]


def _host(frame):
    return tuple(p.cpu().numpy() for p in frame)


def _model_ref(nc, bgr, t, in_d, out_d):
    """The model's own forward on planar BGR frames [2,3,H,W]: the 8-bit form, or the 10-bit forms when a side is 10-bit."""
    frames = torch.from_numpy(bgr)[None].to(nc.device)
    if in_d == 8 and out_d == 8:
        return nc.model.interpolate_u8(frames, t).cpu().numpy()
    return nc.model.interpolate_u10(frames, t, out="u10" if out_d == 10 else "u8").cpu().numpy()


def _check_forward(nc, dev, H, W, fin, fout, t, seed=0):
    """The three properties of one forward; fin / fout: (sampling, layout, depth, matrix, range).  -> the planar outputs."""
    yuv, bgr = _yuv_pair(H, W, fin[0], fin[2], fin[3], fin[4], seed)
    ws = nc.workspace(H, W, len(t))
    outs = nc.forward(_frames(yuv, fin[0], fin[1], fin[2], dev), t, _fmt(*fin), _fmt(*fout), ws=ws, W=W)
    torch.cuda.synchronize()
    pair, planar = nc.planar(ws, H, W, len(t), fin[2], fout[2])
    assert np.array_equal(pair.cpu().numpy(), bgr), (fin, "pair")           # the input kernel: the oracle's BGR frames
    got = np.stack([p.cpu().numpy() for p in planar])
    assert np.array_equal(got, _model_ref(nc, bgr, t, fin[2], fout[2])), (fin, fout, "model")   # the forward: the model's bytes on them
    for k in range(len(t)):                                                  # the output kernel: the oracle's YUV of them
        want = C.pack(*C.bgr_to_yuv(got[k], fout[0], fout[3], fout[4], fout[2]), fout[0], fout[1], fout[2])
        for p, (g, w) in enumerate(zip(_host(outs[k]), want)):
            assert np.array_equal(g, w), (fout, k, p)
    return got


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_forward_equals_model_on_oracle_bgr(nc, dev, H, W, case):
    _check_forward(nc, dev, H, W, case, case, [0.5])


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("fin,fout", [(("422", "planar", 10, "bt709", "limited"), ("444", "planar", 8, "bt601", "full")),
                                      (("422", "uyvy", 8, "bt601", "limited"), ("422", "semiplanar", 10, "bt709", "limited"))])
def test_mixed_formats(nc, dev, H, W, fin, fout):
    _check_forward(nc, dev, H, W, fin, fout, [0.5], seed=1)


def test_three_outputs_differ_and_each_is_the_oracles(nc, dev):
    got = _check_forward(nc, dev, 201, 333, P210 + ("bt709", "limited"), ("422", "yuyv", 8, "bt709", "limited"), [0.25, 0.5, 0.75], seed=2)
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])


@pytest.mark.parametrize("H,W,pad,offset", [(256, 256, 64, 0), (201, 333, 14, 6)])
@pytest.mark.parametrize("s,l,d", [("422", "planar", 10), ("422", "uyvy", 8), ("444", "semiplanar", 8)])
def test_pitched_and_offset_planes_give_the_tight_bytes_and_keep_the_gaps(nc, dev, H, W, pad, offset, s, l, d):
    import fldr_chroma as V
    fmt = _fmt(s, l, d)
    yuv, _ = _yuv_pair(H, W, s, d, "bt709", "limited", seed=3)
    tight = nc.forward(_frames(yuv, s, l, d, dev), [0.5], fmt, fmt, W=W)
    results = []
    for fill in (0xA5, 0x00):
        frames = _frames(yuv, s, l, d, dev, pad=pad, fill=fill, offset=offset)
        shapes = V.plane_shapes(fmt, H, W)
        outs = [_to_dev([np.zeros(sh, V.plane_dtype(fmt, numpy=True)) for sh in shapes], dev, pad=pad + (2 if offset else 0), fill=0x5A, offset=offset)]
        nc.forward(frames, [0.5], fmt, fmt, outs=outs, W=W)
        torch.cuda.synchronize()
        for p in outs[0]:
            b = p.view(torch.uint8) if p.dtype != torch.uint8 else p
            base = b.as_strided((b.shape[0], b.stride(0)), b.stride())       # the rows with their gaps
            assert bool((base[:, b.shape[1]:] == 0x5A).all()), "a gap byte of an output plane was written"
        results.append(_host(outs[0]))
    for a, b, c in zip(results[0], results[1], _host(tight[0])):
        assert np.array_equal(a, b) and np.array_equal(a, c)                # gap bytes have no effect; pitches give the tight bytes


def test_two_streams_with_two_workspaces_give_the_bytes_of_one(nc, dev):
    H, W = 256, 256
    s, l, d = P210
    fmt = _fmt(s, l, d)
    pairs = [_frames(_yuv_pair(H, W, s, d, "bt709", "limited", seed=10 + p)[0], s, l, d, dev) for p in range(2)]
    t = torch.tensor([0.5], device=dev)
    refs = []
    for p in range(2):
        refs.append(nc.forward(pairs[p], t, fmt, fmt))
        torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    wss = [nc.workspace(H, W) for _ in range(2)]
    got = []
    torch.cuda.synchronize()
    for i in range(6):
        with torch.cuda.stream(streams[i % 2]):
            got.append((i % 2, nc.forward(pairs[i % 2], t, fmt, fmt, ws=wss[i % 2])))
    torch.cuda.synchronize()
    for k, o in got:
        for a, b in zip(o[0], refs[k][0]):
            assert torch.equal(a, b), k
    assert not torch.equal(refs[0][0][0], refs[1][0][0])


def test_graph_capture_replays_the_eager_bytes_and_reads_t_at_replay(nc, dev):
    import fldr_chroma as V
    H, W = 256, 256
    s, l, d = "422", "planar", 10
    fmt = _fmt(s, l, d)
    frames = _frames(_yuv_pair(H, W, s, d, "bt709", "limited", seed=4)[0], s, l, d, dev)
    t = torch.tensor([0.5], device=dev)
    ws = nc.workspace(H, W)
    outs = [V.empty_frame(fmt, H, W, dev)]
    st = torch.cuda.Stream(device=dev)
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        nc.forward(frames, t, fmt, fmt, outs=outs, ws=ws)                  # warm
    st.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        nc.forward(frames, t, fmt, fmt, outs=outs, ws=ws)
    seen = []
    for tv in (0.3, 0.8):
        t.fill_(tv)
        g.replay()
        torch.cuda.synchronize()
        eager = nc.forward(frames, [tv], fmt, fmt)
        torch.cuda.synchronize()
        for a, b in zip(outs[0], eager[0]):
            assert torch.equal(a, b), tv
        seen.append(_host(outs[0])[0])
    assert not np.array_equal(seen[0], seen[1])


def _clip(H, W, n, d, seed=5):
    """n frames of a texture moving 4 px down and 6 px right per frame (planar BGR code values of depth d)."""
    base = _bgr_pair(H + 4 * n, W + 6 * n, d, seed)[0]
    return [np.ascontiguousarray(base[:, 4 * k:4 * k + H, 6 * k:6 * k + W]) for k in range(n)]


def test_session_pushes_equal_forwards_on_consecutive_frames(nc, dev):
    import fldr_chroma as V
    H, W, n_t = 256, 256, 2
    fi, fo = ("422", "uyvy", 8), ("422", "planar", 10)
    fin, fout = _fmt(*fi), _fmt(*fo)
    frames = [C.pack(*C.bgr_to_yuv(f, "422", "bt709", "limited", 8), *fi) for f in _clip(H, W, 4, 8)]
    s = V.Session(nc.model, H, W, n_t, fin, fout)
    counts, prev = [], None
    t = [(k + 1) / (n_t + 1) for k in range(n_t)]
    for f in frames:
        outs = s.push(f)
        counts.append(len(outs))
        if prev is not None:
            ref = nc.forward([_to_dev(prev, dev), _to_dev(f, dev)], t, fin, fout)
            torch.cuda.synchronize()
            for k in range(n_t):
                for a, b in zip(outs[k], _host(ref[k])):
                    assert np.array_equal(a, b), k
        prev = f
    assert counts == [0, 2, 2, 2]
    s.reset()
    assert s.push(frames[0]) == [] and s.last_n_out == 0
    assert len(s.push(frames[1])) == n_t
    s.close()


def test_c_example_reproduces_the_session_on_yuv422p10le(nc, dev, clean_launcher, tmp_path):
    import fldr_harness as Hn
    import fldr_chroma as V
    H, W, F = 256, 320, 2
    fi = ("422", "planar", 10)
    frames = [C.pack(*C.bgr_to_yuv(f, "422", "bt709", "limited", 10), *fi) for f in _clip(H, W, 3, 10, seed=6)]
    raw = [b"".join(p.tobytes() for p in f) for f in frames]
    (tmp_path / "in.yuv").write_bytes(b"".join(raw))
    exe = os.path.join(ROOT, "examples", "fldr_slowmo_pro")
    if not os.path.exists(exe):
        exe = str(tmp_path / "fldr_slowmo_pro")
        subprocess.run([shutil.which("cc") or "gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "examples", "fldr_slowmo_pro.c"), "-L" + PKG, "-l:libfldr_chroma.so", "-l:libfldr_model.so",
                        "-Wl,-rpath," + PKG], check=True)
    cmd = '"%s" "%s" %d %d %d yuv422p10le < "%s" > "%s"' % (exe, Hn.DEFAULT_WEIGHTS, W, H, F, tmp_path / "in.yuv", tmp_path / "out.yuv")
    r = clean_launcher(["sh", "-c", cmd], env=dict(os.environ), timeout=300)
    assert r["rc"] == 0, r
    data = (tmp_path / "out.yuv").read_bytes()
    n = len(raw[0])
    assert len(data) == 5 * n
    got = [data[k * n:(k + 1) * n] for k in range(5)]
    for k in range(3):
        assert got[2 * k] == raw[k], k
    fmt = _fmt(*fi)
    s = V.Session(nc.model, H, W, F - 1, fmt, fmt)
    s.push(frames[0])
    for k in range(1, 3):
        outs = s.push(frames[k])
        assert got[2 * k - 1] == b"".join(p.tobytes() for p in outs[0]), k
    s.close()
