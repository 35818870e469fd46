"""The pipe API (libfldr_pipe.so through fldr_pipe) on the GPU.  The reference is always fldr_rate.Converter on the same frames — the
synchronous converter underneath, which tests/test_gpu_rate.py holds to the schedule and to the forwards of its pairs — and every
comparison is exact: job k of a pipe returns the frames, the count and the scene result of call k of the converter, at every depth and
for every interleaving of submit and receive.  Every frame of a clip differs from every other, so a stale ring slot shows; 13 frames
make every ring (depth + 1 device frames, depth + 3 pinned frames, depth + 1 pinned output sets) wrap at depth 4."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import rate_frames as RF
import yuv_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fldr-vfi_amd")
N_FRAMES, CUT_AT = 13, 7
ZERO_SCENE = {"sad": 0, "hist_dist": 0, "cut": 0}
FLUSH = "flush"


@pytest.fixture(scope="module")
def nm(dev):
    import fldr_harness as Hn
    import fldr_model
    m = fldr_model.NativeModel.from_npz(Hn.DEFAULT_WEIGHTS, device=dev.index or 0)
    yield m
    m.close()


def _fmt(layout, depth=8):
    import fldr_video
    return fldr_video.Format(layout, "bt709", "limited", depth)


def _clip(H, W, n, seed):
    """n frames of a texture moving 4 px down and 6 px right per frame (BGR planar numpy)."""
    import fldr_harness as Hn
    base = Hn.synthetic_pair(H + 4 * n, W + 6 * n, seed=seed).numpy()[0]
    return [np.ascontiguousarray(base[:, 4 * k:4 * k + H, 6 * k:6 * k + W]) for k in range(n)]


@functools.lru_cache(maxsize=None)
def _bgr(H, W):
    """13 BGR frames: seven of one moving texture, then six of another, darker one — a cut at frame 7."""
    a, b = _clip(H, W, CUT_AT, seed=5), _clip(H, W, N_FRAMES - CUT_AT, seed=11)
    return a + [(f.astype(np.float64) * 0.35).round().astype(np.uint8) for f in b]


@functools.lru_cache(maxsize=None)
def _frames(H, W, layout, depth):
    frames = [RF.planes_of_bgr(f, layout, depth) for f in _bgr(H, W)]
    for f in frames:                                                 # shared by every test: never written
        for p in f:
            p.flags.writeable = False
    assert len(set(f[0].tobytes() for f in frames)) == N_FRAMES
    return frames


_REF = {}


def _reference(nm, H, W, layout, depth, in_rate, out_rate, scene, calls=None):
    """What fldr_rate.Converter returns, call by call, for the stream `calls` (frame numbers and FLUSH; default: every frame, then a
    flush): a list of (frames, scene dict).  Computed once per configuration and shared."""
    import fldr_rate as R
    calls = tuple(calls) if calls is not None else tuple(range(N_FRAMES)) + (FLUSH,)
    key = (H, W, layout, depth, in_rate, out_rate, scene, calls)
    if key not in _REF:
        frames = _frames(H, W, layout, depth)
        c = R.Converter(nm, H, W, _fmt(layout, depth), in_rate, out_rate, scene=scene)
        ref = []
        for call in calls:
            if call == FLUSH:
                ref.append((c.flush(), dict(ZERO_SCENE)))
            else:
                outs = c.push(frames[call])
                ref.append((outs, c.last_scene))
        c.close()
        _REF[key] = ref
    return _REF[key]


def _pipe(nm, H, W, layout, depth, in_rate, out_rate, scene, pipe_depth):
    import fldr_pipe as P
    return P.Pipe(nm, H, W, _fmt(layout, depth), in_rate, out_rate, depth=pipe_depth, scene=scene)


def _do(p, frames, call):
    p.flush() if call == FLUSH else p.submit(frames[call])


def _drive(p, frames, calls, driver):
    """Run `calls` (frame numbers and FLUSH) through the pipe -> the jobs in the order received: a list of (frames, scene dict)."""
    import fldr_pipe as P
    jobs = []
    if driver == "lockstep":                                        # submit, receive
        for call in calls:
            _do(p, frames, call)
            assert p.pending == 1
            jobs.append(p.receive())
    elif driver == "greedy":                                        # submit until E_FULL, receive one, repeat
        i = 0
        while i < len(calls):
            try:
                _do(p, frames, calls[i])
                i += 1
            except P.PipeFull:
                assert p.pending == p.depth
                jobs.append(p.receive())
    else:                                                           # burst: depth submits, then depth receives
        assert driver == "burst"
        for i in range(0, len(calls), p.depth):
            for call in calls[i:i + p.depth]:
                _do(p, frames, call)
            for _ in calls[i:i + p.depth]:
                jobs.append(p.receive())
    while p.pending:
        jobs.append(p.receive())
    return jobs


def _assert_equal(jobs, ref):
    assert len(jobs) == len(ref)
    for k, ((outs, scene), (want, want_scene)) in enumerate(zip(jobs, ref)):
        assert len(outs) == len(want), (k, len(outs), len(want))
        assert scene == want_scene, (k, scene, want_scene)
        for q, (a, b) in enumerate(zip(outs, want)):
            for x, y in zip(a, b):
                assert x.dtype == y.dtype and np.array_equal(x, y), "job %d, output %d" % (k, q)


ALL = list(range(N_FRAMES)) + [FLUSH]


# ---- equality with the synchronous converter ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("driver", ["lockstep", "greedy", "burst"])
@pytest.mark.parametrize("pipe_depth", [1, 2, 3, 4])
@pytest.mark.parametrize("scene", [True, False])
def test_24_to_60_equals_the_converter_at_every_depth_and_interleaving(nm, scene, pipe_depth, driver):
    H, W = 256, 448
    ref = _reference(nm, H, W, "nv12", 8, 24, 60, scene)
    frames = _frames(H, W, "nv12", 8)
    # what the reference itself is: t changes from pair to pair, pass-through frames mix with interpolated ones, the last frame lands
    # on an output (the flush returns it), and with the detector on the splice is a cut on job 7 that repeats frames 6 and 7
    assert [len(o) for o, _ in ref] == [0, 3, 2, 3, 2, 3, 2, 3, 2, 3, 2, 3, 2, 1]
    assert [s["cut"] for _, s in ref] == ([0] * CUT_AT + [1] + [0] * 6 if scene else [0] * 14)
    same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(a, b))
    cut_outs = ref[CUT_AT][0]                                        # outputs 15, 16, 17 at 6, 6.4, 6.8
    assert same(cut_outs[0], frames[6]) and same(cut_outs[1], frames[6]) == scene and same(cut_outs[2], frames[7]) == scene
    p = _pipe(nm, H, W, "nv12", 8, 24, 60, scene, pipe_depth)
    assert p.max_out == 3 and p.pending == 0
    _assert_equal(_drive(p, frames, ALL, driver), ref)
    assert p.pending == 0
    p.close()


@pytest.mark.parametrize("in_rate,out_rate,scene", [(1, 2, True), (60, 24, True), (30, 30, True), (30, 30, False), (60, 24, False)])
def test_other_job_kinds_equal_the_converter(nm, in_rate, out_rate, scene):
    """1 -> 2: one interpolated and one pass-through frame per job; 60 -> 24: pairs without a forward (the measure alone, or with the
    detector off nothing but the upload) between pairs with one; 30 -> 30: no device work for any output."""
    H, W = 256, 448
    ref = _reference(nm, H, W, "nv12", 8, in_rate, out_rate, scene)
    if scene:
        assert [s["cut"] for _, s in ref] == [0] * CUT_AT + [1] + [0] * 6     # every pair is measured, whatever it returns
    p = _pipe(nm, H, W, "nv12", 8, in_rate, out_rate, scene, 3)
    _assert_equal(_drive(p, _frames(H, W, "nv12", 8), ALL, "greedy"), ref)
    p.close()


@pytest.mark.parametrize("H,W,layout", [(255, 447, "i420"), (256, 448, "nv12")])
def test_odd_size_and_10_bits_equal_the_converter(nm, H, W, layout):
    """yuv420p10le at an odd size (the packed frame is no multiple of 256 bytes: ring offsets) and P010."""
    ref = _reference(nm, H, W, layout, 10, 24, 60, True)
    assert sum(s["cut"] for _, s in ref) == 1
    p = _pipe(nm, H, W, layout, 10, 24, 60, True, 3)
    _assert_equal(_drive(p, _frames(H, W, layout, 10), ALL, "greedy"), ref)
    p.close()


# ---- the copy-free path ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipe_depth", [1, 3, 4])
def test_in_place_input_and_views_that_outlive_depth_more_submits(nm, pipe_depth):
    """Frames are written into input_planes() and submitted without a copy; outputs are taken as views.  Each view is left alone
    while the pipe is filled again — the `depth` jobs behind the viewed one have then all been submitted — and while the frame after
    those is already written into input_planes(); only then is it compared."""
    H, W = 256, 448
    ref = _reference(nm, H, W, "nv12", 8, 24, 60, True)
    frames = _frames(H, W, "nv12", 8)
    p = _pipe(nm, H, W, "nv12", 8, 24, 60, True, pipe_depth)
    filled = [None]

    def fill(i):
        if filled[0] != i:
            planes = p.input_planes()
            for dst, src in zip(planes, frames[i]):
                assert dst.shape == src.shape and dst.dtype == src.dtype
                dst[...] = src
            filled[0] = i
    i, jobs = 0, 0
    fill(0)
    p.submit()
    i = 1
    while p.pending:
        views, scene = p.receive_view()
        while i <= N_FRAMES and p.pending < pipe_depth:
            if i < N_FRAMES:
                fill(i)
                p.submit()
            else:
                p.flush()
            i += 1
        if i < N_FRAMES:
            fill(i)                                                  # the next frame, written before the view is looked at
        assert p.pending == min(pipe_depth, len(ref) - 1 - jobs)
        _assert_equal([(views, scene)], [ref[jobs]])
        jobs += 1
    assert jobs == len(ref)
    p.close()


def test_the_callers_frame_may_be_overwritten_when_submit_returns(nm):
    import fldr_pipe as P
    H, W = 256, 448
    ref = _reference(nm, H, W, "nv12", 8, 24, 60, True)
    frames = _frames(H, W, "nv12", 8)
    p = _pipe(nm, H, W, "nv12", 8, 24, 60, True, 3)
    jobs, i = [], 0
    while i < N_FRAMES:
        mine = tuple(a.copy() for a in frames[i])
        try:
            p.submit(mine)
            i += 1
        except P.PipeFull:
            jobs.append(p.receive())
        for a in mine:
            a.fill(0xFF)
    if p.pending == p.depth:                                         # the flush is a job too
        jobs.append(p.receive())
    p.flush()
    while p.pending:
        jobs.append(p.receive())
    _assert_equal(jobs, ref)
    p.close()


# ---- the state machine --------------------------------------------------------------------------------------------------------------------------
def test_full_empty_and_refused_calls_change_nothing(nm):
    import ctypes
    import fldr_pipe as P
    H, W = 256, 448
    ref = _reference(nm, H, W, "nv12", 8, 24, 60, True)
    frames = _frames(H, W, "nv12", 8)
    p = _pipe(nm, H, W, "nv12", 8, 24, 60, True, 2)
    for call in (p.receive, p.receive_view):                        # an idle pipe
        with pytest.raises(P.PipeEmpty) as e:
            call()
        assert e.value.code == P.E_EMPTY
    p.submit(frames[0])
    p.submit(frames[1])
    for _ in range(2):
        with pytest.raises(P.PipeFull) as e:
            p.submit(frames[12])                                     # refused: this frame never enters the stream
        assert e.value.code == P.E_FULL and p.pending == 2
        with pytest.raises(P.PipeFull):
            p.flush()
        assert p.pending == 2
    jobs = [p.receive()]
    # job 1 has three outputs: a receive without frames to write them to is refused and leaves the job where it is
    n = ctypes.c_int(-1)
    assert P.lib().fldr_pipe_receive(p._h, None, ctypes.byref(n), None) == P.E_ARG and n.value == 0 and p.pending == 1
    jobs += _drive(p, frames, ALL[2:], "greedy")
    _assert_equal(jobs, ref)
    with pytest.raises(P.PipeEmpty):
        p.receive()
    p.close()


def test_reset_drops_outstanding_jobs_and_starts_a_new_stream(nm):
    import fldr_pipe as P
    H, W = 256, 448
    ref = _reference(nm, H, W, "nv12", 8, 24, 60, True)
    frames = _frames(H, W, "nv12", 8)
    p = _pipe(nm, H, W, "nv12", 8, 24, 60, True, 3)
    for k in (5, 9, 2):
        p.submit(frames[k])
    assert p.pending == 3
    p.reset()
    assert p.pending == 0
    with pytest.raises(P.PipeEmpty):
        p.receive()
    _assert_equal(_drive(p, frames, ALL, "greedy"), ref)            # as a fresh converter's: frame 0 first, no output for it
    p.reset()
    _assert_equal(_drive(p, frames, ALL, "burst"), ref)
    p.close()


def test_a_second_flush_is_an_empty_job_and_the_stream_goes_on_after_it(nm):
    H, W = 256, 448
    calls = [0, 1, 2, FLUSH, FLUSH, 3, 4, FLUSH, 5, FLUSH]
    ref = _reference(nm, H, W, "nv12", 8, 24, 60, True, calls)
    # three frames end on output 5, which the first flush returns and the second does not (nor the push after it); five frames end on
    # output 10, six between two outputs
    assert [len(o) for o, _ in ref] == [0, 3, 2, 1, 0, 2, 2, 1, 2, 0]
    frames = _frames(H, W, "nv12", 8)
    for driver in ("lockstep", "greedy"):
        p = _pipe(nm, H, W, "nv12", 8, 24, 60, True, 3)
        _assert_equal(_drive(p, frames, calls, driver), ref)
        p.close()


# ---- the example ------------------------------------------------------------------------------------------------------------------------------
def _example(name, tmp_path, libs):
    exe = os.path.join(ROOT, "examples", name)
    if not os.path.exists(exe):
        exe = str(tmp_path / name)
        subprocess.run([shutil.which("cc") or "gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "examples", name + ".c"), "-L" + PKG] + ["-l:lib%s.so" % l for l in libs] + ["-Wl,-rpath," + PKG],
                       check=True)
    return exe


def test_example_writes_the_bytes_of_fldr_fps(dev, clean_launcher, tmp_path):
    """examples/fldr_fps_async and examples/fldr_fps, each a fresh child process with its own time limit, on the same eight raw I420
    frames with a cut in them: the same stdout byte for byte, the same lines on stderr."""
    import fldr_harness as Hn
    H, W = 256, 448
    bgr = _bgr(H, W)[CUT_AT - 4:CUT_AT + 4]                          # four frames of each scene
    (tmp_path / "in.yuv").write_bytes(b"".join(O.i420_bytes(*O.bgr_to_yuv420(f, "bt709", "limited")) for f in bgr))
    libs = ["fldr_rate", "fldr_video", "fldr_model"]
    got = {}
    for name, extra, more in (("fldr_fps", "", []), ("fldr_fps_async", " depth=3", ["fldr_pipe"])):
        exe = _example(name, tmp_path, more + libs)
        cmd = '"%s" "%s" %d %d 24 60%s < "%s" > "%s" 2> "%s"' % (exe, Hn.DEFAULT_WEIGHTS, W, H, extra, tmp_path / "in.yuv",
                                                             tmp_path / (name + ".yuv"), tmp_path / (name + ".err"))
        r = clean_launcher(["sh", "-c", cmd], env=dict(os.environ), timeout=120)
        err = (tmp_path / (name + ".err")).read_text()
        assert r["rc"] == 0, (r, err)
        got[name] = ((tmp_path / (name + ".yuv")).read_bytes(), err)
    n = H * W * 3 // 2
    assert len(got["fldr_fps"][0]) == 18 * n                         # 7 x 5 / 2 = 17.5: outputs 0 .. 17
    assert got["fldr_fps_async"][0] == got["fldr_fps"][0]
    assert got["fldr_fps_async"][1] == got["fldr_fps"][1] and "cut at frame 4\n" in got["fldr_fps"][1]
