"""The C model API (libfldr_model.so through fldr_model.NativeModel) on the GPU: every output form and input form gives the bits of
the Python path it replaces (DCTXVFInet.forward via fldr_harness), at the test sizes, at 4K, at every pyramid depth, for 8x
interpolation, with pairs in flight on several streams, under a graph capture and through the C example."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fldr-vfi_amd")


@pytest.fixture(scope="module")
def py_models(dev):
    """(DCTXVFInet, args, NativeModel) per pyramid depth, created on first use."""
    import fldr_harness as Hn
    import fldr_model
    cache = {}

    def get(S=5):
        if S not in cache:
            m, _, a = Hn.prepare_model(dev, args=Hn.args_config(test_scales=S))
            cache[S] = (m, a, fldr_model.NativeModel.from_module(m))
        return cache[S]
    yield get
    for _, _, nm in cache.values():
        nm.close()


def _pair(H, W, seed, dev):
    import fldr_harness as Hn
    u8 = Hn.synthetic_pair(H, W, seed=seed).to(dev)                     # [2,3,H,W] (BGR planes)
    return u8, Hn.frames_from_uint8(u8)


def _native_frame(nm, a, frames, t):
    import fldr_harness as Hn
    H, W = frames.shape[-2:]
    with torch.no_grad():
        pyr = Hn.build_pyramid(Hn.pad_frames(frames, a), a)
    return nm.forward_pyramid(pyr, t, H, W)[:, :, :H, :W], pyr


@pytest.mark.parametrize("H,W,t", [(256, 256, 0.5), (200, 500, 0.125), (2160, 3840, 0.5), (2160, 4096, 0.5)])
def test_fp64_frame_equals_python_forward(dev, py_models, H, W, t):
    import fldr_harness as Hn
    m, a, nm = py_models(5)
    _, frames = _pair(H, W, 3, dev)
    got, pyr = _native_frame(nm, a, frames, [t])
    ref = Hn.interpolate(m, a, frames, torch.tensor([[t]], device=dev), pyramid=pyr)
    torch.cuda.synchronize()
    assert got.dtype == torch.float64 and got.shape == ref.shape
    assert torch.equal(got, ref), float((got - ref).abs().max())


def test_fp64_frame_matches_the_oracle(dev, py_models, oracle, weights):
    """The smoke() case (256 x 256, t = 0.5) against the CPU oracle, within smoke()'s bound."""
    m, a, nm = py_models(5)
    _, frames = _pair(256, 256, 0, dev)
    got, _ = _native_frame(nm, a, frames, [0.5])
    with torch.no_grad():
        ref = oracle.forward(weights, oracle.pad_and_pyramid(frames.cpu()), torch.tensor([[0.5]]))[:, :, :256, :256]
    assert (got.cpu() - ref).abs().max().item() < 2e-5


@pytest.mark.parametrize("case", ["depth_S3_100x150", "depth_S4_128x200", "depth_S6_300x400", "depth_S7_520x530"])
def test_pyramid_depths_equal_python_forward(dev, py_models, golden, case):
    import fldr_harness as Hn
    g = golden(case)
    S = int(g["S_tst"])
    m, a, nm = py_models(S)
    frames = Hn.frames_from_uint8(torch.from_numpy(g["frames_u8"])).to(dev)
    t = float(g["t"])
    got, pyr = _native_frame(nm, a, frames, [t])
    ref = Hn.interpolate(m, a, frames, torch.tensor([[t]], device=dev), pyramid=pyr)
    assert torch.equal(got, ref), float((got - ref).abs().max())
    # the 8-bit path at this depth (7: more levels than the one-launch ingest holds) against interpolate_u8
    u8 = torch.from_numpy(g["frames_u8"]).to(dev)[None]
    ref8, _ = Hn.interpolate_u8(m, a, u8, torch.tensor([[t]], device=dev))
    assert torch.equal(nm.interpolate_u8(u8, [t]), ref8)
    hwc = [u8[0, k].permute(1, 2, 0).contiguous() for k in range(2)]
    assert torch.equal(nm.interpolate_u8(pair=hwc, t=[t]), ref8)


@pytest.mark.parametrize("H,W", [(256, 384), (200, 301), (2160, 3840)])
def test_planar_u8_equals_interpolate_u8(dev, py_models, H, W):
    import fldr_harness as Hn
    m, a, nm = py_models(5)
    u8, _ = _pair(H, W, 5, dev)
    ref, _ = Hn.interpolate_u8(m, a, u8[None], torch.tensor([[0.375]], device=dev))
    got = nm.interpolate_u8(u8[None], [0.375])
    assert got.shape == (1, 3, H, W) and got.dtype == torch.uint8
    assert torch.equal(got, ref)


def _pitched(hwc, extra):
    """[H,W,3] -> the same pixels in a separately allocated buffer whose rows are 3W + extra bytes apart."""
    H, W, _ = hwc.shape
    buf = torch.full((H, 3 * W + extra), 77, dtype=torch.uint8, device=hwc.device)
    buf[:, :3 * W] = hwc.reshape(H, 3 * W)
    return buf.as_strided((H, W, 3), (3 * W + extra, 3, 1)), buf


@pytest.mark.parametrize("H,W", [(256, 384), (200, 500), (2160, 4096)])
def test_interleaved_input_ingests_the_planar_pyramid(dev, py_models, H, W):
    import fldr_hip
    import fldr_model
    m, a, nm = py_models(5)
    u8, _ = _pair(H, W, 6, dev)
    bgr = [u8[k].permute(1, 2, 0).contiguous() for k in range(2)]
    f0, keep0 = _pitched(bgr[0], 40)
    f1, keep1 = _pitched(bgr[1], 8)
    want = fldr_hip.ingest_pyramid(u8[None], 6)
    Hp, Wp = fldr_model.padded_size(H, W)
    got = [torch.full((1, 3, 2, Hp >> i, Wp >> i), float("nan"), device=dev) for i in range(6)]
    out = nm.interpolate_u8(pair=(f0, f1), t=[0.5], order="bgr", pyramid_out=got)
    torch.cuda.synchronize()
    for i in range(6):
        assert torch.equal(got[i], want[i]), i
    ref = nm.interpolate_u8(u8[None], [0.5])
    assert torch.equal(out, ref)
    # RGB frames: the channel-swapped BGR frames give the same frame
    rgb = [_pitched(b[..., [2, 1, 0]].contiguous(), 24)[0] for b in bgr]
    assert torch.equal(nm.interpolate_u8(pair=rgb, t=[0.5], order="rgb"), ref)


def test_interleaved_output_is_the_permuted_planar_frame(dev, py_models):
    m, a, nm = py_models(5)
    u8, _ = _pair(200, 500, 8, dev)
    planar = nm.interpolate_u8(u8[None], [0.25, 0.75])
    bgr = nm.interpolate_u8(u8[None], [0.25, 0.75], out_layout="hwc", order="bgr")
    rgb = nm.interpolate_u8(u8[None], [0.25, 0.75], out_layout="hwc", out_order="rgb")
    assert torch.equal(bgr, planar.permute(0, 2, 3, 1))
    assert torch.equal(rgb, planar.permute(0, 2, 3, 1)[..., [2, 1, 0]])
    # a pitched interleaved output through the raw call: the row padding is left alone
    import fldr_model
    H, W = 200, 500
    pitch = 3 * W + 36
    buf = torch.full((H, pitch), 5, dtype=torch.uint8, device=dev)
    t = torch.tensor([0.25], device=dev)
    io = fldr_model.IO()
    keep = u8[None].contiguous()
    io.batch, io.H, io.W, io.input, io.frames_u8 = 1, H, W, fldr_model.IN_U8_PLANAR, keep.data_ptr()
    io.n_t, io.t, io.output, io.out_pitch = 1, t.data_ptr(), fldr_model.OUT_U8_INTERLEAVED, pitch
    ptrs = (ctypes.c_void_p * 1)(buf.data_ptr())
    io.out = ctypes.cast(ptrs, ctypes.POINTER(ctypes.c_void_p))
    assert nm.forward(io, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(buf[:, :3 * W].reshape(H, W, 3), bgr[0])
    assert bool((buf[:, 3 * W:] == 5).all())


@pytest.mark.parametrize("H,W", [(256, 384), (2160, 4096)])
def test_eight_x_outputs_equal_interpolate_multi(dev, py_models, H, W):
    import fldr_harness as Hn
    m, a, nm = py_models(5)
    _, frames = _pair(H, W, 9, dev)
    ts = [k / 8 for k in range(1, 8)]
    refs = Hn.interpolate_multi(m, a, frames, ts)
    got = nm.interpolate_multi(frames, ts)
    assert len(got) == 7
    for k in range(7):
        assert torch.equal(got[k], refs[k]), (k, float((got[k] - refs[k]).abs().max()))
    with torch.no_grad():
        pyr = Hn.build_pyramid(Hn.pad_frames(frames, a), a)
    for k in range(7):
        one = nm.forward_pyramid(pyr, [ts[k]], H, W)[:, :, :H, :W]
        assert torch.equal(one, got[k]), k


def test_pairs_in_flight_on_three_streams_equal_one_at_a_time(dev, py_models):
    """Four distinct 4K pairs on three streams with three workspaces, as the Python test of the same name does for the eager path."""
    import fldr_harness as Hn
    m, a, nm = py_models(5)
    NS, NP, H, W = 3, 4, 2160, 3840
    pyrs = []
    with torch.no_grad():
        for p in range(NP):
            _, f = _pair(H, W, 40 + p, dev)
            pyrs.append(Hn.build_pyramid(Hn.pad_frames(f, a), a))
    t = torch.tensor([0.5], device=dev)
    refs = [nm.forward_pyramid(pyrs[k], t, H, W).clone() for k in range(NP)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=dev) for _ in range(NS)]
    wss = [nm.workspace(H, W) for _ in range(NS)]
    for rep in range(2):
        for s in streams:
            s.wait_stream(torch.cuda.current_stream())
        outs = []
        for i in range(12):
            s = streams[i % NS]
            with torch.cuda.stream(s):
                o = torch.empty_like(refs[0])
                nm.forward_pyramid(pyrs[i % NP], t, H, W, ws=wss[i % NS], out=o)
                outs.append((i % NP, o))
        torch.cuda.synchronize()
        bad = [(i, k) for i, (k, o) in enumerate(outs) if not torch.equal(o, refs[k])]
        assert not bad, (rep, bad)


def test_graph_capture_replays_the_eager_frame_and_reads_t_at_replay(dev, py_models):
    import fldr_harness as Hn
    m, a, nm = py_models(5)
    H, W = 256, 384
    _, frames = _pair(H, W, 12, dev)
    with torch.no_grad():
        pyr = Hn.build_pyramid(Hn.pad_frames(frames, a), a)
    t = torch.tensor([0.5], device=dev)
    ws = nm.workspace(H, W)
    out = torch.empty(1, 3, *pyr[0].shape[3:], dtype=torch.float64, device=dev)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        nm.forward_pyramid(pyr, t, H, W, ws=ws, out=out)                 # warm: nothing lazy is left for the capture
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        nm.forward_pyramid(pyr, t, H, W, ws=ws, out=out)
    for tv in (0.5, 0.2, 0.9):
        t.fill_(tv)
        g.replay()
        torch.cuda.synchronize()
        eager = nm.forward_pyramid(pyr, [tv], H, W)
        torch.cuda.synchronize()
        assert torch.equal(out, eager), tv
    assert not torch.equal(nm.forward_pyramid(pyr, [0.2], H, W), nm.forward_pyramid(pyr, [0.9], H, W))


def test_bad_calls_return_their_code_and_enqueue_nothing(dev, py_models):
    import fldr_model
    m, a, nm = py_models(5)
    H, W = 256, 256
    u8, _ = _pair(H, W, 13, dev)
    keep = u8[None].contiguous()
    t = torch.tensor([0.5], device=dev)
    out = torch.full((1, 3, H, W), 123, dtype=torch.uint8, device=dev)
    ptrs = (ctypes.c_void_p * 1)(out.data_ptr())

    def io(**kw):
        x = fldr_model.IO()
        x.batch, x.H, x.W, x.input, x.frames_u8 = 1, H, W, fldr_model.IN_U8_PLANAR, keep.data_ptr()
        x.n_t, x.t, x.output = 1, t.data_ptr(), fldr_model.OUT_U8_PLANAR
        x.out = ctypes.cast(ptrs, ctypes.POINTER(ctypes.c_void_p))
        for k, v in kw.items():
            setattr(x, k, v)
        return x
    need = nm.workspace_bytes(H, W)
    small = torch.empty(need - 256, dtype=torch.uint8, device=dev)
    ws = nm.workspace(H, W)
    assert nm.forward(io(), small) == fldr_model.E_WORKSPACE
    assert nm.forward(io(batch=2), ws) == fldr_model.E_BATCH
    assert nm.forward(io(batch=0), ws) == fldr_model.E_BATCH
    x = io(input=fldr_model.IN_U8_INTERLEAVED)
    x.frame[0] = x.frame[1] = keep.data_ptr()
    x.frame_pitch[0], x.frame_pitch[1] = 3 * W, 3 * W - 1
    assert nm.forward(x, ws) == fldr_model.E_ARG
    assert nm.forward(io(output=fldr_model.OUT_U8_INTERLEAVED, out_pitch=3 * W - 3), ws) == fldr_model.E_ARG
    assert nm.forward(io(n_t=0), ws) == fldr_model.E_ARG
    assert nm.forward(io(H=100), ws) == fldr_model.E_SHAPE                # padded to 256 rows: reflect padding needs pad < size
    torch.cuda.synchronize()
    assert bool((out == 123).all()), "a refused call wrote its output"
    assert nm.forward(io(), ws) == 0
    torch.cuda.synchronize()
    assert not bool((out == 123).all())


def test_model_on_a_second_device_gives_the_same_bits(dev, py_models):
    if torch.cuda.device_count() < 2:
        pytest.skip("one device")
    import fldr_harness as Hn
    import fldr_model
    m, a, nm0 = py_models(5)
    nm1 = fldr_model.NativeModel.from_npz(Hn.DEFAULT_WEIGHTS, device=1)
    u8, _ = _pair(256, 384, 14, dev)
    ref = nm0.interpolate_u8(u8[None], [0.5])
    with torch.cuda.device(1):
        got = nm1.interpolate_u8(u8[None].to("cuda:1"), [0.5])
        torch.cuda.synchronize()
    assert torch.cuda.current_device() == 0
    assert torch.equal(got.cpu(), ref.cpu())
    nm1.close()


def _write_ppm(path, hwc_rgb):
    H, W, _ = hwc_rgb.shape
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (W, H))
        f.write(np.ascontiguousarray(hwc_rgb).tobytes())


def test_c_example_gives_the_bytes_of_interpolate_u8(dev, py_models, clean_launcher, tmp_path):
    import fldr_harness as Hn
    m, a, nm = py_models(5)
    H, W = 256, 384
    u8, _ = _pair(H, W, 15, dev)
    ref, _ = Hn.interpolate_u8(m, a, u8[None], torch.tensor([[0.5]], device=dev))
    want = ref[0].permute(1, 2, 0)[..., [2, 1, 0]].cpu().numpy()          # BGR planes -> RGB pixels
    host = u8.cpu().numpy()
    _write_ppm(tmp_path / "a.ppm", host[0].transpose(1, 2, 0)[..., ::-1])
    _write_ppm(tmp_path / "b.ppm", host[1].transpose(1, 2, 0)[..., ::-1])
    exe = os.path.join(ROOT, "examples", "fldr_interp")
    if not os.path.exists(exe):
        exe = str(tmp_path / "fldr_interp")
        subprocess.run([shutil.which("cc") or "gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "examples", "fldr_interp.c"), "-L" + PKG, "-l:libfldr_model.so", "-Wl,-rpath," + PKG], check=True)
    r = clean_launcher([exe, Hn.DEFAULT_WEIGHTS, str(tmp_path / "a.ppm"), str(tmp_path / "b.ppm"), "0.5", str(tmp_path / "out.ppm")],
                       env=dict(os.environ), timeout=300)
    assert r["rc"] == 0, r
    data = open(tmp_path / "out.ppm", "rb").read()
    head = b"P6\n%d %d\n255\n" % (W, H)
    assert data[:len(head)] == head
    got = np.frombuffer(data[len(head):], dtype=np.uint8).reshape(H, W, 3)
    assert np.array_equal(got, want)
