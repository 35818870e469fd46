"""The packed 10-bit API (libfldr_pack10.so through fldr_pack10.NativePack10 / Session) on the GPU.  Every comparison is exact: the input
kernel leaves the oracle's BGR frames (tests/yuv_pack10_oracle.py on tests/yuv_chroma_oracle.py) in the workspace, the forward gives the
model's bytes on those frames, the output kernel gives the oracle's container of the model's planar output, and the whole forward gives
the bytes of libfldr_chroma.so's forward on the same samples as yuv422p10le / yuv444p10le — for every container, mixed formats, several
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

import yuv_chroma_oracle as C
import yuv_pack10_oracle as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fldr-vfi_amd")
SIZES = [(64, 64), (66, 70)]
CASES = [(c, "bt709", "limited") for c in P.CONTAINERS] + [("v210", m, r) for m in C.MATRICES for r in C.RANGES if (m, r) != ("bt709", "limited")]
MARK = 0x5A


@pytest.fixture(scope="module")
def nm(dev):
    import fldr_harness as Hn
    import fldr_model
    m = fldr_model.NativeModel.from_npz(Hn.DEFAULT_WEIGHTS, device=dev.index or 0, test_scales=3)
    yield m
    m.close()


@pytest.fixture(scope="module")
def npk(nm):
    import fldr_pack10
    return fldr_pack10.NativePack10(nm)


def _fmt(c, mat="bt709", rng="limited"):
    import fldr_pack10 as V
    return V.Format(c, mat, rng)


@functools.lru_cache(maxsize=None)
def _bgr_pair(H, W, seed=0):
    """fldr_harness.synthetic_pair as 10-bit code values: [2,3,H,W] (the 8-bit value with its top two bits repeated below)."""
    import fldr_harness as Hn
    u8 = Hn.synthetic_pair(H, W, seed=seed).numpy()
    return (u8.astype(np.uint16) << 2) | (u8 >> 6)


@functools.lru_cache(maxsize=None)
def _yuv_pair(H, W, s, mat, rng, seed=0):
    """((Y, U, V), (Y, U, V)) of the synthetic pair converted by the oracle, and the oracle's BGR frames [2,3,H,W] of those planes."""
    src = _bgr_pair(H, W, seed)
    yuv = [C.bgr_to_yuv(src[i], s, mat, rng, 10) for i in range(2)]
    bgr = np.stack([C.yuv_to_bgr(*yuv[i], s, mat, rng, 10) for i in range(2)])
    return yuv, bgr


def _to_dev(plane, dev, pad=0, fill=0, offset=0):
    """A device copy of a host plane; pad / offset (bytes): a view into a byte buffer `pad` bytes wider per row (gap bytes = fill), starting
    `offset` bytes into it.  -> (frame, buffer)."""
    r, c = plane.shape
    rb = c * plane.itemsize
    pitch = rb + pad
    buf = torch.full((offset + r * pitch + 32,), fill, dtype=torch.uint8, device=dev)
    v = buf[offset:offset + r * pitch].view(r, pitch)[:, :rb]
    v.copy_(torch.from_numpy(np.ascontiguousarray(plane).view(np.uint8).reshape(r, rb)).to(dev))
    return (v.view(torch.uint16 if plane.itemsize == 2 else torch.uint32),), buf


def _frames(yuv, c, dev, **kw):
    return [_to_dev(P.pack(*yuv[i], c)[0], dev, **kw)[0] for i in range(2)]


def _host(frame):
    """The plane of a device frame as a numpy array (through its bytes: a pitched view too)."""
    p = frame[0]
    r, n = p.shape
    b = np.ascontiguousarray(p.view(torch.uint8).cpu().numpy())
    return b.view(np.uint16 if p.dtype == torch.uint16 else np.uint32).reshape(r, n)


def _check_forward(npk, dev, H, W, fin, fout, t, seed=0):
    """The properties of one forward; fin / fout: (container, matrix, range).  -> the planar outputs."""
    import fldr_chroma as K
    si, so = P.SAMPLING[fin[0]], P.SAMPLING[fout[0]]
    yuv, bgr = _yuv_pair(H, W, si, fin[1], fin[2], seed)
    ws = npk.workspace(H, W, len(t))
    outs = npk.forward(_frames(yuv, fin[0], dev), t, _fmt(*fin), _fmt(*fout), ws=ws, W=W)
    torch.cuda.synchronize()
    pair, planar = npk.planar(ws, H, W, len(t))
    assert np.array_equal(pair.cpu().numpy(), bgr), (fin, "pair")           # the input kernel: the oracle's BGR frames
    got = np.stack([p.cpu().numpy() for p in planar])
    ref = npk.model.interpolate_u10(torch.from_numpy(bgr)[None].to(dev), t, out="u10").cpu().numpy()
    assert np.array_equal(got, ref), (fin, fout, "model")                   # the forward: the model's bytes on them
    for k in range(len(t)):                                                  # the output kernel: the oracle's container of them
        want = P.pack(*C.bgr_to_yuv(got[k], so, fout[1], fout[2], 10), fout[0])[0]
        assert np.array_equal(_host(outs[k]), want), (fout, k)
    # the planar library's forward on the same samples as yuv422p10le / yuv444p10le, repacked
    kc = K.NativeChroma(npk.model)
    kin = [tuple(torch.from_numpy(p).to(dev) for p in C.pack(*yuv[i], si, "planar", 10)) for i in range(2)]
    kouts = kc.forward(kin, t, K.Format(si, "planar", fin[1], fin[2], 10), K.Format(so, "planar", fout[1], fout[2], 10))
    torch.cuda.synchronize()
    for k in range(len(t)):
        samples = [p.cpu().numpy() for p in kouts[k]]
        assert np.array_equal(_host(outs[k]), P.pack(*samples, fout[0])[0]), (fin, fout, k, "planar library")
    return got


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_forward_equals_model_on_oracle_bgr_and_the_planar_library(npk, dev, H, W, case):
    _check_forward(npk, dev, H, W, case, case, [0.5])


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("fin,fout", [(("v210", "bt709", "limited"), ("y410", "bt601", "full")),
                                      (("y410", "bt601", "limited"), ("y210", "bt709", "limited")),
                                      (("y210", "bt709", "full"), ("v210", "bt601", "limited"))])
def test_mixed_containers_and_colour(npk, dev, H, W, fin, fout):
    _check_forward(npk, dev, H, W, fin, fout, [0.5], seed=1)


def test_three_outputs_differ_and_each_is_the_oracles(npk, dev):
    got = _check_forward(npk, dev, 66, 70, ("v210", "bt709", "limited"), ("y210", "bt709", "limited"), [0.25, 0.5, 0.75], seed=2)
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])


@pytest.mark.parametrize("H,W,pad,offset", [(64, 64, 64, 0), (66, 70, 12, 4)])
@pytest.mark.parametrize("c", P.CONTAINERS)
def test_pitched_and_offset_planes_give_the_tight_bytes_and_keep_the_gaps(npk, dev, H, W, pad, offset, c):
    fmt = _fmt(c)
    yuv, _ = _yuv_pair(H, W, P.SAMPLING[c], "bt709", "limited", seed=3)
    tight = npk.forward(_frames(yuv, c, dev), [0.5], fmt, fmt, W=W)
    results = []
    for fill in (0xA5, 0x00):
        frames = _frames(yuv, c, dev, pad=pad, fill=fill, offset=offset)
        zero = np.zeros((H, P.row_words(c, W)), np.uint16 if c == "y210" else np.uint32)
        out, buf = _to_dev(zero, dev, pad=pad + (4 if offset else 0), fill=MARK, offset=offset)
        npk.forward(frames, [0.5], fmt, fmt, outs=[out], W=W)
        torch.cuda.synchronize()
        rb, pitch = zero.shape[1] * zero.itemsize, zero.shape[1] * zero.itemsize + pad + (4 if offset else 0)
        b = buf.cpu().numpy()
        keep = np.ones(b.shape, bool)
        rows = np.empty((H, rb), np.uint8)
        for y in range(H):
            rows[y] = b[offset + y * pitch:offset + y * pitch + rb]
            keep[offset + y * pitch:offset + y * pitch + rb] = False
        assert (b[keep] == MARK).all(), "a byte outside the rows of an output plane was written"
        results.append(rows.view(zero.dtype))
    assert np.array_equal(results[0], results[1]) and np.array_equal(results[0], _host(tight[0]))   # gaps have no effect; pitches give the tight bytes


def test_two_streams_with_two_workspaces_give_the_bytes_of_one(npk, dev):
    H, W, c = 64, 64, "v210"
    fmt = _fmt(c)
    pairs = [_frames(_yuv_pair(H, W, "422", "bt709", "limited", seed=10 + p)[0], c, dev) for p in range(2)]
    t = torch.tensor([0.5], device=dev)
    refs = []
    for p in range(2):
        refs.append(_host(npk.forward(pairs[p], t, fmt, fmt, W=W)[0]))
        torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    wss = [npk.workspace(H, W) for _ in range(2)]
    got = []
    torch.cuda.synchronize()
    for i in range(6):
        with torch.cuda.stream(streams[i % 2]):
            got.append((i % 2, npk.forward(pairs[i % 2], t, fmt, fmt, ws=wss[i % 2], W=W)))
    torch.cuda.synchronize()
    for k, o in got:
        assert np.array_equal(_host(o[0]), refs[k]), k
    assert not np.array_equal(refs[0], refs[1])


def test_graph_capture_replays_the_eager_bytes_and_reads_t_at_replay(npk, dev):
    import fldr_pack10 as V
    H, W = 64, 64
    fin, fout = _fmt("v210"), _fmt("y410")
    frames = _frames(_yuv_pair(H, W, "422", "bt709", "limited", seed=4)[0], "v210", dev)
    t = torch.tensor([0.5], device=dev)
    ws = npk.workspace(H, W)
    outs = [V.empty_frame(fout, H, W, dev)]
    st = torch.cuda.Stream(device=dev)
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        npk.forward(frames, t, fin, fout, outs=outs, ws=ws, W=W)           # warm
    st.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        npk.forward(frames, t, fin, fout, outs=outs, ws=ws, W=W)
    seen = []
    for tv in (0.3, 0.8):
        t.fill_(tv)
        g.replay()
        torch.cuda.synchronize()
        eager = npk.forward(frames, [tv], fin, fout, W=W)
        torch.cuda.synchronize()
        assert np.array_equal(_host(outs[0]), _host(eager[0])), tv
        seen.append(_host(outs[0]))
    assert not np.array_equal(seen[0], seen[1])


def _clip(H, W, n, seed=5):
    """n frames of a texture moving 4 px down and 6 px right per frame (planar BGR 10-bit code values)."""
    base = _bgr_pair(H + 4 * n, W + 6 * n, seed)[0]
    return [np.ascontiguousarray(base[:, 4 * k:4 * k + H, 6 * k:6 * k + W]) for k in range(n)]


def test_session_pushes_equal_forwards_on_consecutive_frames(npk, dev):
    import fldr_pack10 as V
    H, W, n_t = 66, 70, 2
    fin, fout = _fmt("v210"), _fmt("y210", "bt601", "full")
    frames = [P.pack(*C.bgr_to_yuv(f, "422", "bt709", "limited", 10), "v210") for f in _clip(H, W, 4)]
    s = V.Session(npk.model, H, W, n_t, fin, fout)
    counts, prev = [], None
    t = [(k + 1) / (n_t + 1) for k in range(n_t)]
    for f in frames:
        outs = s.push(f)
        counts.append(len(outs))
        if prev is not None:
            ref = npk.forward([_to_dev(prev[0], dev)[0], _to_dev(f[0], dev)[0]], t, fin, fout, W=W)
            torch.cuda.synchronize()
            for k in range(n_t):
                assert np.array_equal(outs[k][0], _host(ref[k])), k
        prev = f
    assert counts == [0, 2, 2, 2]
    s.reset()
    assert s.push(frames[0]) == [] and s.last_n_out == 0
    assert len(s.push(frames[1])) == n_t
    s.close()


def test_c_example_reproduces_the_session_on_a_v210_stream(dev, clean_launcher, tmp_path):
    """Raw v210 frames at the customary pitch (128 bytes per 48 pixels, the gap zero) through examples/fldr_slowmo_sdi: the input frames
    come back byte for byte, the frames between them are the session's, their gaps zero."""
    import fldr_harness as Hn
    import fldr_model
    import fldr_pack10 as V
    H, W, F = 130, 134, 2
    pitch = P.v210_pitch(W)
    assert pitch == 384 and 4 * P.row_words("v210", W) == 368

    def raw_of(plane):
        buf = np.zeros((H, pitch // 4), np.uint32)
        buf[:, :plane.shape[1]] = plane
        return buf.tobytes()
    frames = [P.pack(*C.bgr_to_yuv(f, "422", "bt709", "limited", 10), "v210") for f in _clip(H, W, 3, seed=6)]
    raw = [raw_of(f[0]) for f in frames]
    (tmp_path / "in.v210").write_bytes(b"".join(raw))
    exe = os.path.join(ROOT, "examples", "fldr_slowmo_sdi")
    if not os.path.exists(exe):
        exe = str(tmp_path / "fldr_slowmo_sdi")
        subprocess.run([shutil.which("cc") or "gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "examples", "fldr_slowmo_sdi.c"), "-L" + PKG, "-l:libfldr_pack10.so", "-l:libfldr_model.so",
                        "-Wl,-rpath," + PKG], check=True)
    cmd = '"%s" "%s" %d %d %d < "%s" > "%s"' % (exe, Hn.DEFAULT_WEIGHTS, W, H, F, tmp_path / "in.v210", tmp_path / "out.v210")
    r = clean_launcher(["sh", "-c", cmd], env=dict(os.environ), timeout=300)
    assert r["rc"] == 0, r
    data = (tmp_path / "out.v210").read_bytes()
    n = len(raw[0])
    assert n == pitch * H and len(data) == 5 * n
    got = [data[k * n:(k + 1) * n] for k in range(5)]
    for k in range(3):
        assert got[2 * k] == raw[k], k
    fmt = _fmt("v210")
    shipped = fldr_model.NativeModel.from_npz(Hn.DEFAULT_WEIGHTS, device=dev.index or 0)
    s = V.Session(shipped, H, W, F - 1, fmt, fmt)
    s.push(frames[0])
    for k in range(1, 3):
        outs = s.push(frames[k])
        assert got[2 * k - 1] == raw_of(outs[0][0]), k
    s.close()
    shipped.close()
