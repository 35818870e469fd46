"""ctypes binding of libfldr_rate.so (rate API: include/fldr_rate.h) — scene-cut measure, forward with cut fallback and frame-rate
conversion on YUV 4:2:0 frames, on top of fldr_video.

    m = scene_measure((f0, f1), Format("nv12"))                  # -> {"sad", "hist_dist", "cut"} of a pair of device frames
    nr = NativeRate(fldr_model.NativeModel.from_npz(fldr_harness.DEFAULT_WEIGHTS))
    outs, scene = nr.forward((f0, f1), t=[0.25, 0.5], fmt=Format("nv12"))   # on a cut: copies of f0 / f1 by t
    c = Converter(native_model, H, W, Format("i420"), in_rate=24, out_rate=60)   # host frames (numpy planes)
    outs = c.push((y, u, v)); ...; outs = c.flush()              # c.last_scene: the measure of the pair just pushed

schedule(n_frames, in_rate, out_rate) is the pure-Python statement of which output comes from which pair at which t; the tests hold
the library to it.  Frames are fldr_video's: tuples of 2-D plane tensors (device) or numpy arrays (host).  Every forward and measure
enqueues on torch's current stream and returns without synchronising (scene_measure synchronises to read the result back unless
told not to).  No fallback: a missing library raises at load.
"""
import ctypes
import os
from fractions import Fraction

import torch

import fldr_model
import fldr_video
from fldr_video import Format, Frame, IO, _stream_ptr, empty_frame, frame_struct, plane_dtype, plane_shapes  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfldr_rate.so")
RATE_VERSION = 100                # include/fldr_rate.h: FLDR_RATE_VERSION
E_ARG, E_FORMAT, E_STATE, E_RATIO, E_DEVICE = -200, -201, -202, -203, -204
SCENE_SAD_DEFAULT, SCENE_HIST_DEFAULT = 80, 100
SCENE_STATE_BYTES = 4096
MAX_OUT = 64


class SceneParams(ctypes.Structure):
    _fields_ = [("sad_permille", ctypes.c_int32), ("hist_permille", ctypes.c_int32), ("reserved", ctypes.c_int32 * 2)]

    def __init__(self, sad_permille=0, hist_permille=0):
        super().__init__(int(sad_permille), int(hist_permille))


class SceneResult(ctypes.Structure):
    _fields_ = [("sad", ctypes.c_uint64), ("hist_dist", ctypes.c_uint32), ("cut", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 4)]

    def as_dict(self):
        return {"sad": int(self.sad), "hist_dist": int(self.hist_dist), "cut": int(self.cut)}


class RateConfig(ctypes.Structure):
    _fields_ = [("H", ctypes.c_int32), ("W", ctypes.c_int32), ("format", Format), ("in_num", ctypes.c_int32), ("in_den", ctypes.c_int32),
                ("out_num", ctypes.c_int32), ("out_den", ctypes.c_int32), ("device", ctypes.c_int32), ("scene", ctypes.c_int32),
                ("scene_params", SceneParams), ("reserved", ctypes.c_int32 * 4)]


_SIGNATURES = {
    "fldr_rate_version": (ctypes.c_int, []),
    "fldr_rate_error_string": (ctypes.c_char_p, [ctypes.c_int]),
    "fldr_rate_sizeof": (ctypes.c_int, [ctypes.c_int]),
    "fldr_scene_measure": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(Format), ctypes.POINTER(Frame), ctypes.POINTER(SceneParams),
                                          ctypes.c_void_p, ctypes.c_void_p]),
    "fldr_rate_workspace_bytes": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "fldr_rate_forward": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(IO), ctypes.POINTER(SceneParams), ctypes.c_void_p, ctypes.c_int64,
                                         ctypes.c_void_p]),
    "fldr_rate_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(RateConfig), ctypes.POINTER(ctypes.c_void_p)]),
    "fldr_rate_max_out": (ctypes.c_int, [ctypes.c_void_p]),
    "fldr_rate_push": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Frame), ctypes.POINTER(Frame), ctypes.POINTER(ctypes.c_int),
                                      ctypes.POINTER(SceneResult)]),
    "fldr_rate_flush": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Frame), ctypes.POINTER(ctypes.c_int)]),
    "fldr_rate_reset": (ctypes.c_int, [ctypes.c_void_p]),
    "fldr_rate_destroy": (None, [ctypes.c_void_p]),
}
EXPORTS = tuple(_SIGNATURES)
_lib = None


class RateError(RuntimeError):
    def __init__(self, what, code):
        super().__init__("%s failed: %s (code %d)" % (what, lib().fldr_rate_error_string(code).decode(), code))
        self.code = code


def lib():
    """The loaded libfldr_rate.so, checked against this binding (struct sizes, header version); raises when it has not been built."""
    global _lib
    if _lib is None:
        _lib = fldr_model.load_library(LIB_PATH, _SIGNATURES, (SceneParams, SceneResult, RateConfig), "fldr_rate", RATE_VERSION)
    return _lib


def _check(code, what):
    if code != 0:
        raise RateError(what, code)


# ---- the schedule -------------------------------------------------------------------------------------------------------------------
def _rate(r):
    """An int, a Fraction, a (num, den) pair or a "num/den" string -> Fraction."""
    return Fraction(*r) if isinstance(r, tuple) else Fraction(r)


def ratio(in_rate, out_rate):
    """(A, B): output frame j sits at input position j A / B (A / B = in_rate / out_rate, reduced)."""
    q = _rate(in_rate) / _rate(out_rate)
    return q.numerator, q.denominator


def max_out(in_rate, out_rate):
    """ceil(B / A): the most outputs one pushed frame can produce."""
    A, B = ratio(in_rate, out_rate)
    return -(-B // A)


def schedule(n_frames, in_rate, out_rate):
    """What a converter returns for a stream of n_frames frames: a list of n_frames + 1 lists, entry n the outputs of the push of frame
    n, the last entry those of the flush.  An output is (j, i, r, B): output frame j is input frame i when r == 0, and otherwise the
    interpolation of frames (i, i + 1) at t = r / B — on a cut, frame i when r * 2 < B, else frame i + 1.  i = floor(j A / B),
    r = j A mod B; the push of frame n >= 1 returns every j with n - 1 <= j A / B < n, the flush the j that lands on the last frame."""
    A, B = ratio(in_rate, out_rate)
    pushes, j = [[] for _ in range(n_frames + 1)], 0
    for n in range(1, n_frames):
        while j * A < n * B:
            pushes[n].append((j, (j * A) // B, (j * A) % B, B))
            j += 1
    if n_frames >= 1 and j * A == (n_frames - 1) * B:
        pushes[n_frames].append((j, n_frames - 1, 0, B))
    return pushes


def rate_config(H, W, fmt, in_rate, out_rate, scene=True, params=None, device=0, into=None):
    """A fldr_rate_config from Converter's arguments; `into`: the RateConfig to fill (the `rate` member of a larger configuration)."""
    cfg = RateConfig() if into is None else into
    cfg.H, cfg.W, cfg.device, cfg.scene = int(H), int(W), int(device), 1 if scene else 0
    cfg.format = fmt
    i, o = _rate(in_rate), _rate(out_rate)
    cfg.in_num, cfg.in_den, cfg.out_num, cfg.out_den = i.numerator, i.denominator, o.numerator, o.denominator
    if params is not None:
        cfg.scene_params = params if isinstance(params, SceneParams) else SceneParams(*params)
    return cfg


# ---- the cut measure ------------------------------------------------------------------------------------------------------------------
def scene_state(device):
    """FLDR_SCENE_STATE_BYTES of device memory (torch's allocations are 256-byte aligned)."""
    return torch.empty(SCENE_STATE_BYTES, dtype=torch.uint8, device=device)


def read_result(state):
    """The fldr_scene_result at the start of a scene state tensor (synchronising copy) -> dict."""
    return SceneResult.from_buffer_copy(state[:ctypes.sizeof(SceneResult)].cpu().numpy().tobytes()).as_dict()


def scene_measure_raw(H, W, fmt, frames, params, state_ptr, stream_ptr):
    """The raw call; returns the code without raising (tests of the error contract)."""
    arr = (Frame * 2)(*frames) if frames is not None else None
    return lib().fldr_scene_measure(int(H), int(W), ctypes.byref(fmt) if fmt is not None else None, arr,
                                    ctypes.byref(params) if params is not None else None, state_ptr, stream_ptr)


def scene_measure(frames, fmt, params=None, state=None, stream=None, read=True):
    """fldr_scene_measure of frames (I0, I1), each a tuple of device plane tensors in `fmt` (pitches from their strides); params: a
    SceneParams or (sad_permille, hist_permille), None = the defaults; state: a scene_state tensor (allocated otherwise).  Enqueues on
    torch's current stream; -> {"sad", "hist_dist", "cut"} after a synchronising read-back, or the state tensor with read=False."""
    H, W = frames[0][0].shape
    device = frames[0][0].device
    if params is not None and not isinstance(params, SceneParams):
        params = SceneParams(*params)
    if state is None:
        state = scene_state(device)
    _check(scene_measure_raw(H, W, fmt, [frame_struct(f) for f in frames], params, ctypes.c_void_p(state.data_ptr()), _stream_ptr(device, stream)),
           "fldr_scene_measure")
    return read_result(state) if read else state


class NativeRate(fldr_video.NativeVideo):
    """fldr_rate_forward on a fldr_model.NativeModel: NativeVideo's forward plus the cut measure and the select."""

    def __init__(self, native_model):
        lib()
        super().__init__(native_model)

    def workspace_bytes(self, H, W, n_t=1):
        n = lib().fldr_rate_workspace_bytes(self.model._h, int(H), int(W), int(n_t))
        if n < 0:
            raise RateError("fldr_rate_workspace_bytes", int(n))
        return int(n)

    def state_of(self, ws, H, W, n_t=1):
        """The scene state inside a workspace used by a forward with n_t outputs."""
        end = self.workspace_bytes(H, W, n_t)
        return ws[end - SCENE_STATE_BYTES:end]

    def forward_io(self, io, ws, params=None, stream=None):
        """The raw call; returns the code without raising."""
        return lib().fldr_rate_forward(self.model._h, ctypes.byref(io) if io is not None else None,
                                       ctypes.byref(params) if params is not None else None,
                                       ctypes.c_void_p(ws.data_ptr()) if ws is not None else None, ws.numel() if ws is not None else 0,
                                       _stream_ptr(self.device, stream))

    def forward(self, frames, t=0.5, fmt=None, params=None, outs=None, ws=None, stream=None, read=True):
        """frames: (I0, I1) in fmt; t as NativeVideo.forward takes it.  -> (the n_t output frames, the pair's scene dict); read=False
        skips the synchronising read-back and returns the state tensor in its place."""
        fmt = fmt or Format()
        H, W = frames[0][0].shape
        tt = self._t(t)
        n_t = tt.numel()
        if params is not None and not isinstance(params, SceneParams):
            params = SceneParams(*params)
        if outs is None:
            outs = [empty_frame(fmt, H, W, self.device) for _ in range(n_t)]
        if ws is None:
            ws = self.workspace(H, W, n_t)
        io = self.make_io(frames, tt, fmt, fmt, outs, H, W)
        _check(self.forward_io(io, ws, params, stream), "fldr_rate_forward")
        state = self.state_of(ws, H, W, n_t)
        return outs, (read_result(state) if read else state)


class Converter(fldr_video.HostStream):
    """fldr_rate: host frames (tuples of numpy planes) pushed one by one at in_rate; each push returns the output frames at out_rate that
    fall before the pushed frame (schedule()), flush() the one that lands on the last frame."""

    _destroy = staticmethod(lambda h: lib().fldr_rate_destroy(h))

    def __init__(self, native_model, H, W, fmt=None, in_rate=24, out_rate=60, scene=True, params=None):
        fmt = fmt or Format()
        cfg = rate_config(H, W, fmt, in_rate, out_rate, scene, params, native_model.device.index or 0)
        self._h = ctypes.c_void_p()
        self.model = native_model                                    # the converter uses the model: keep it alive
        _check(lib().fldr_rate_create(native_model._h, ctypes.byref(cfg), ctypes.byref(self._h)), "fldr_rate_create")
        self.H, self.W, self.format = int(H), int(W), fmt
        self.max_out = lib().fldr_rate_max_out(self._h)
        self._stage(fmt, H, W, self.max_out)
        self.last_scene = None

    def push(self, frame):
        """-> the list of output frames due (tuples of numpy planes, fresh copies); self.last_scene: the pair's scene dict."""
        fr = frame_struct(frame)
        n = ctypes.c_int(-1)
        res = SceneResult()
        _check(lib().fldr_rate_push(self._h, ctypes.byref(fr), self._out_structs(), ctypes.byref(n), ctypes.byref(res)), "fldr_rate_push")
        self.last_scene = res.as_dict()
        return self._taken(n.value)

    def flush(self):
        n = ctypes.c_int(-1)
        _check(lib().fldr_rate_flush(self._h, self._out_structs(), ctypes.byref(n)), "fldr_rate_flush")
        return self._taken(n.value)

    def reset(self):
        _check(lib().fldr_rate_reset(self._h), "fldr_rate_reset")


# ---- what the bindings of the libraries above this one share (fldr_cadence, fldr_pulldown, fldr_probe) ------------------------------------
class Binding:
    """One library on the rate library: its name (the functions are fldr_<name>_*), path, header version, the signatures of its functions
    and its struct mirrors -> lib() (loads on first use, after libfldr_rate.so), its error class `Error` (named error_name) and check()."""

    def __init__(self, name, path, version, signatures, structs, error_name):
        self.name, self.path, self.version, self.signatures, self.structs = name, path, version, signatures, structs
        self._lib = None
        api = self

        def init(self, what, code):
            RuntimeError.__init__(self, "%s failed: %s (code %d)" % (what, api.fn("error_string")(code).decode(), code))
            self.code = code

        self.Error = type(error_name, (RuntimeError,), {"__init__": init})

    def lib(self):
        if self._lib is None:
            lib()
            self._lib = fldr_model.load_library(self.path, self.signatures, self.structs, "fldr_" + self.name, self.version)
        return self._lib

    def fn(self, name):
        return getattr(self.lib(), "fldr_%s_%s" % (self.name, name))

    def check(self, code, what):
        if code != 0:
            raise self.Error(what, code)


def _ref(x):
    return ctypes.byref(x) if x is not None else None


def state_tensor(n_bytes, device):
    """A measure state: n_bytes of device memory (torch's allocations are 256-byte aligned)."""
    return torch.empty(n_bytes, dtype=torch.uint8, device=device)


def read_struct(cls, state):
    """The result struct `cls` at the start of a measure state tensor (synchronising copy) -> its dict, plus "reserved": the spare words."""
    r = cls.from_buffer_copy(state[:ctypes.sizeof(cls)].cpu().numpy().tobytes())
    d = r.as_dict()
    d["reserved"] = [int(v) for v in r.reserved]
    return d


def inner_rate(in_rate, cycle, drop):
    """The input rate of the inner converter of a cycle stream: in_rate x (cycle - drop) / cycle, a Fraction."""
    return _rate(in_rate) * (int(cycle) - int(drop)) / int(cycle)


def inner_rate_raw(api, Config, in_num, in_den, cycle, drop):
    """fldr_<name>_inner_rate on a Config with only these four words set -> (code, num, den); does not raise."""
    cfg = Config()
    cfg.rate.in_num, cfg.rate.in_den, cfg.cycle, cfg.drop = int(in_num), int(in_den), int(cycle), int(drop)
    n, d = ctypes.c_int32(0), ctypes.c_int32(0)
    return api.fn("inner_rate")(ctypes.byref(cfg), ctypes.byref(n), ctypes.byref(d)), n.value, d.value


class CycleStream(fldr_video.HostStream):
    """What Cadence and Pulldown share: frames pushed one by one at in_rate, of every `cycle` of which `drop` are dropped; the push that
    completes a cycle returns the output frames at out_rate its survivors produce, flush() those of the partial last cycle and the inner
    converter's flush.  A subclass names its library (`_api`, a Binding) and its report struct (`_Report`) and makes the configuration."""

    def _destroy(self, h):
        self._api.fn("destroy")(h)

    def _create(self, native_model, cfg, H, W, fmt, cycle, drop):
        self._h = ctypes.c_void_p()
        self.model = native_model                                    # the stream uses the model: keep it alive
        self._api.check(self._api.fn("create")(native_model._h, ctypes.byref(cfg), ctypes.byref(self._h)), "fldr_%s_create" % self._api.name)
        self.H, self.W, self.format, self.cycle, self.drop = int(H), int(W), fmt, int(cycle), int(drop)
        self.max_out = self._api.fn("max_out")(self._h)
        self._stage(fmt, H, W, self.max_out)
        self.last_report = None

    def _done(self, n, rep):
        self.last_report = rep.as_dict() if rep.n_frames else None
        return self._taken(n)

    def push(self, frame):
        """-> the list of output frames due (tuples of numpy planes, fresh copies): empty unless the push completes a cycle;
        self.last_report: that cycle's report dict, else None."""
        fr = frame_struct(frame)
        n = ctypes.c_int(-1)
        rep = self._Report()
        self._api.check(self._api.fn("push")(self._h, ctypes.byref(fr), self._out_structs(), ctypes.byref(n), ctypes.byref(rep)),
                        "fldr_%s_push" % self._api.name)
        return self._done(n.value, rep)

    def flush(self):
        n = ctypes.c_int(-1)
        rep = self._Report()
        self._api.check(self._api.fn("flush")(self._h, self._out_structs(), ctypes.byref(n), ctypes.byref(rep)), "fldr_%s_flush" % self._api.name)
        return self._done(n.value, rep)

    def reset(self):
        self._api.check(self._api.fn("reset")(self._h), "fldr_%s_reset" % self._api.name)
