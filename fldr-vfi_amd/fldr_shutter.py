"""ctypes binding of libfldr_shutter.so (shutter API: include/fldr_shutter.h) — integer integration of YUV 4:2:0 frames over a shutter
interval and motion-blurred frame-rate conversion, on top of fldr_rate and fldr_video.

    acc = accumulate(frames, weights, Format("nv12"))            # device frames -> the uint32 accumulator (a uint8 tensor)
    out = resolve(acc, sum(weights), H, W, Format("nv12"))       # -> one device frame
    out = mix(frames, weights, Format("nv12"))                   # the two fused: the same bytes, no accumulator
    ns = NativeShutter(fldr_model.NativeModel.from_npz(fldr_harness.DEFAULT_WEIGHTS))
    out = ns.forward((f0, f1), t=[0.25, 0.5, 0.75], weights=(1, 0, [1, 1, 1]), fmt=Format("nv12"))
    c = Converter(native_model, H, W, Format("i420"), in_rate=120, out_rate=24, shutter=(1, 2), sub=1)   # host frames (numpy planes)
    outs = c.push((y, u, v)); ...; outs = c.flush()              # c.last_info: one dict per output, c.last_scene: the pair's measure

schedule(n_frames, in_rate, out_rate, shutter, sub, cuts) is the statement of which push returns which output averaged over which
grid points, with the window of every output taken from the library's own host-only fldr_shutter_plan; the tests hold both to the
exact-rational rule of tests/shutter_oracle.py.  Frames are fldr_video's: tuples of 2-D plane tensors (device) or numpy arrays
(host).  Every kernel call and forward enqueues on torch's current stream and returns without synchronising.  No fallback: a missing
library raises at load.
"""
import ctypes
import os
from fractions import Fraction

import torch

import fldr_model
import fldr_rate
import fldr_video
from fldr_rate import SceneParams, SceneResult, _rate
from fldr_video import Format, Frame, IO, _stream_ptr, empty_frame, frame_struct, plane_dtype, plane_shapes  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfldr_shutter.so")
SHUTTER_VERSION = 100             # include/fldr_shutter.h: FLDR_SHUTTER_VERSION
E_ARG, E_FORMAT, E_ACC, E_WEIGHT, E_RATIO, E_DEVICE = -300, -301, -302, -303, -304, -305
MAX_OUT, MAX_SUB, LAUNCH_FRAMES, MAX_TOTAL = 64, 64, 66, 65535


class ShutterConfig(ctypes.Structure):
    _fields_ = [("H", ctypes.c_int32), ("W", ctypes.c_int32), ("format", Format), ("in_num", ctypes.c_int32), ("in_den", ctypes.c_int32),
                ("out_num", ctypes.c_int32), ("out_den", ctypes.c_int32), ("shutter_num", ctypes.c_int32), ("shutter_den", ctypes.c_int32),
                ("sub", ctypes.c_int32), ("device", ctypes.c_int32), ("scene", ctypes.c_int32), ("scene_params", SceneParams),
                ("reserved", ctypes.c_int32 * 4)]


class Info(ctypes.Structure):
    _fields_ = [("j", ctypes.c_int64), ("points", ctypes.c_int32), ("interpolated", ctypes.c_int32), ("truncated", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]

    def as_dict(self):
        return {"j": int(self.j), "points": int(self.points), "interpolated": int(self.interpolated), "truncated": int(self.truncated)}


_I32P = ctypes.POINTER(ctypes.c_int32)
_KERNEL_HEAD = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(Format)]
_SIGNATURES = {
    "fldr_shutter_version": (ctypes.c_int, []),
    "fldr_shutter_error_string": (ctypes.c_char_p, [ctypes.c_int]),
    "fldr_shutter_sizeof": (ctypes.c_int, [ctypes.c_int]),
    "fldr_shutter_acc_bytes": (ctypes.c_int64, _KERNEL_HEAD),
    "fldr_shutter_accumulate": (ctypes.c_int, _KERNEL_HEAD + [ctypes.POINTER(Frame), _I32P, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "fldr_shutter_resolve": (ctypes.c_int, _KERNEL_HEAD + [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Frame), ctypes.c_void_p]),
    "fldr_shutter_mix": (ctypes.c_int, _KERNEL_HEAD + [ctypes.POINTER(Frame), _I32P, ctypes.c_int, ctypes.POINTER(Frame), ctypes.c_void_p]),
    "fldr_shutter_reciprocal": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]),
    "fldr_shutter_workspace_bytes": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "fldr_shutter_forward": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(IO), ctypes.c_int, ctypes.c_int, _I32P, ctypes.c_void_p, ctypes.c_int64,
                                            ctypes.c_void_p]),
    "fldr_shutter_plan": (ctypes.c_int, [ctypes.POINTER(ShutterConfig), ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
    "fldr_shutter_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ShutterConfig), ctypes.POINTER(ctypes.c_void_p)]),
    "fldr_shutter_max_out": (ctypes.c_int, [ctypes.c_void_p]),
    "fldr_shutter_push": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Frame), ctypes.POINTER(Frame), ctypes.POINTER(Info), ctypes.POINTER(ctypes.c_int),
                                         ctypes.POINTER(SceneResult)]),
    "fldr_shutter_flush": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Frame), ctypes.POINTER(Info), ctypes.POINTER(ctypes.c_int)]),
    "fldr_shutter_reset": (ctypes.c_int, [ctypes.c_void_p]),
    "fldr_shutter_destroy": (None, [ctypes.c_void_p]),
}
EXPORTS = tuple(_SIGNATURES)
_lib = None


class ShutterError(RuntimeError):
    def __init__(self, what, code):
        super().__init__("%s failed: %s (code %d)" % (what, lib().fldr_shutter_error_string(code).decode(), code))
        self.code = code


def lib():
    """The loaded libfldr_shutter.so, checked against this binding (struct sizes, header version); raises when it has not been built."""
    global _lib
    if _lib is None:
        _lib = fldr_model.load_library(LIB_PATH, _SIGNATURES, (ShutterConfig, Info), "fldr_shutter", SHUTTER_VERSION)
    return _lib


class _Api:
    """A library as the code this module shares with fldr_light calls it: fldr_<prefix>_<name>(*args) of lib(), a refusal raised as the
    library's own error class."""

    def __init__(self, lib, prefix, error):
        self.lib, self.prefix, self.error, self._fns = lib, prefix, error, {}

    def fn(self, name):
        f = self._fns.get(name)
        if f is None:
            f = self._fns[name] = getattr(self.lib(), "%s_%s" % (self.prefix, name))
        return f

    def call(self, name, *args):
        """A function that returns a code."""
        code = (self._fns.get(name) or self.fn(name))(*args)
        if code != 0:
            raise self.error("%s_%s" % (self.prefix, name), code)

    def size(self, name, *args):
        """A function that returns a number of bytes, or a negative code."""
        n = self.fn(name)(*args)
        if n < 0:
            raise self.error("%s_%s" % (self.prefix, name), int(n))
        return int(n)


_API = _Api(lib, "fldr_shutter", ShutterError)


# ---- the window rule and the schedule -----------------------------------------------------------------------------------------------------
def config(in_rate, out_rate, shutter=(1, 2), sub=1, H=0, W=0, fmt=None, device=0, scene=False, params=None):
    """A ShutterConfig; rates as fldr_rate takes them (an int, a Fraction, a (num, den) pair or a "num/den" string), so is the shutter."""
    cfg = ShutterConfig()
    cfg.H, cfg.W, cfg.device, cfg.scene, cfg.sub = int(H), int(W), int(device), 1 if scene else 0, int(sub)
    cfg.format = fmt or Format()
    i, o, s = _rate(in_rate), _rate(out_rate), _rate(shutter)
    cfg.in_num, cfg.in_den, cfg.out_num, cfg.out_den = i.numerator, i.denominator, o.numerator, o.denominator
    cfg.shutter_num, cfg.shutter_den = s.numerator, s.denominator
    if params is not None:
        cfg.scene_params = params if isinstance(params, SceneParams) else SceneParams(*params)
    return cfg


def plan(cfg, j):
    """fldr_shutter_plan: (first, last) grid point of output j's window.  Host only."""
    f, l = ctypes.c_int64(), ctypes.c_int64()
    _API.call("plan", ctypes.byref(cfg), int(j), ctypes.byref(f), ctypes.byref(l))
    return f.value, l.value


def max_out(in_rate, out_rate):
    """ceil(B / A) + 1: the most outputs one pushed frame can produce (the windows that begin in its interval, and one open before)."""
    return fldr_rate.max_out(in_rate, out_rate) + 1


def schedule(n_frames, in_rate, out_rate, shutter=(1, 2), sub=1, cuts=()):
    """What a converter returns for a stream of n_frames frames: a list of n_frames + 1 lists, entry n the outputs of the push of frame
    n, the last entry those of the flush.  An output is a dict: j; "points", the kept grid points as (i, k, source) with source the input
    frame whose samples the point takes on a cut pair (None: frame i itself for k == 0, else the interpolation of (i, i + 1) at
    t = k / sub); "truncated".  cuts: the frames n whose pair (n - 1, n) is a cut (what the measure reports with scene on).  The windows
    come from fldr_shutter_plan; the push rule is the header's: the push of frame n supplies the points (n - 1) sub < m <= n sub."""
    cfg = config(in_rate, out_rate, shutter, sub)
    cuts = set(cuts)
    pushes = [[] for _ in range(n_frames + 1)]
    j, open_, scene_of_window, n_cuts = 0, None, 0, 0
    for n in range(n_frames):
        hi = n * sub
        lo = hi - sub + 1 if n else hi
        cut = n in cuts
        while True:
            f, l = plan(cfg, j)
            if f > hi:
                break
            if open_ is None:
                open_ = {"j": j, "points": [], "truncated": False}
            for m in range(max(f, lo), min(l, hi) + 1):
                k = m - (hi - sub) if n else sub                    # 1 .. sub; sub: frame n itself
                sc = n_cuts + (1 if cut and 2 * k >= sub else 0)
                if not open_["points"]:
                    scene_of_window = sc
                if sc != scene_of_window:
                    open_["truncated"] = True
                    break
                if k == sub:
                    open_["points"].append((n, 0, None))
                else:
                    open_["points"].append((n - 1, k, (n - 1 if 2 * k < sub else n) if cut else None))
            if not (open_["truncated"] or l <= hi):
                break
            pushes[n].append(open_)
            open_, j = None, j + 1
        n_cuts += 1 if cut else 0
    if open_ is not None:
        open_["truncated"] = True
        pushes[n_frames].append(open_)
    return pushes


# ---- the integration kernels --------------------------------------------------------------------------------------------------------------
def acc_bytes(H, W, fmt):
    return _API.size("acc_bytes", int(H), int(W), ctypes.byref(fmt))


def reciprocal(total):
    """(mul, shift) resolve divides by 2 total with."""
    m, s = ctypes.c_uint32(), ctypes.c_uint32()
    _API.call("reciprocal", int(total), ctypes.byref(m), ctypes.byref(s))
    return m.value, s.value


def _i32(values):
    return (ctypes.c_int32 * len(values))(*[int(v) for v in values])


def _frames_weights(frames, weights):
    return (Frame * len(frames))(*[frame_struct(f) for f in frames]), (ctypes.c_int32 * len(weights))(*[int(v) for v in weights])


# accumulate / resolve / mix of this library and of fldr_light: `lead` is what the library's function takes behind fmt (light: the curve),
# `trail` what it takes before the stream (light: the pointer to scratch).  acc: a uint8 device tensor of the library's acc_bytes, or None.
def _accumulate(api, lead, trail, frames, weights, fmt, acc, acc_size, first, stream):
    H, W = frames[0][0].shape
    device = frames[0][0].device
    if acc is None:
        acc = torch.empty(acc_size(H, W), dtype=torch.uint8, device=device)
    arr, w = _frames_weights(frames, weights)
    api.call("accumulate", int(H), int(W), ctypes.byref(fmt), *lead, arr, w, len(frames), 1 if first else 0, ctypes.c_void_p(acc.data_ptr()), *trail,
             _stream_ptr(device, stream))
    return acc


def _resolve(api, lead, trail, acc, total, H, W, fmt, out, stream):
    if out is None:
        out = empty_frame(fmt, H, W, acc.device)
    fr = frame_struct(out)
    api.call("resolve", int(H), int(W), ctypes.byref(fmt), *lead, ctypes.c_void_p(acc.data_ptr()), int(total), ctypes.byref(fr), *trail,
             _stream_ptr(acc.device, stream))
    return out


def _mix(api, lead, trail, frames, weights, fmt, out, stream):
    H, W = frames[0][0].shape
    device = frames[0][0].device
    if out is None:
        out = empty_frame(fmt, H, W, device)
    arr, w = _frames_weights(frames, weights)
    fr = frame_struct(out)
    api.call("mix", int(H), int(W), ctypes.byref(fmt), *lead, arr, w, len(frames), ctypes.byref(fr), *trail,
             _stream_ptr(device, stream))
    return out


def accumulate(frames, weights, fmt, acc=None, first=True, stream=None):
    """fldr_shutter_accumulate of device frames; acc: a uint8 device tensor of acc_bytes (allocated otherwise) -> acc."""
    return _accumulate(_API, (), (), frames, weights, fmt, acc, lambda H, W: acc_bytes(H, W, fmt), first, stream)


def resolve(acc, total, H, W, fmt, out=None, stream=None):
    """fldr_shutter_resolve -> one device frame (`out` when given; allocated packed otherwise)."""
    return _resolve(_API, (), (), acc, total, H, W, fmt, out, stream)


def mix(frames, weights, fmt, out=None, stream=None):
    """fldr_shutter_mix of device frames -> one device frame."""
    return _mix(_API, (), (), frames, weights, fmt, out, stream)


class _NativeForward(fldr_video.NativeVideo):
    """What NativeShutter and fldr_light.NativeLight share: the library's forward on a fldr_model.NativeModel.  A subclass names its
    library (`_api`) and gives forward_io / forward its own signature: `lead` is what its forward takes behind io (light: the curve)."""

    def __init__(self, native_model):
        self._api.lib()
        super().__init__(native_model)

    def workspace_bytes(self, H, W, n_t=1):
        return self._api.size("workspace_bytes", self.model._h, int(H), int(W), int(n_t))

    def _forward_io(self, io, lead, w0, w1, w, ws, stream):
        return self._api.fn("forward")(self.model._h, ctypes.byref(io) if io is not None else None, *lead, int(w0), int(w1),
                                       _i32(w) if w is not None else None, ctypes.c_void_p(ws.data_ptr()) if ws is not None else None,
                                       ws.numel() if ws is not None else 0, _stream_ptr(self.device, stream))

    def _forward(self, lead, frames, t, weights, fmt, out, ws, stream):
        fmt = fmt or Format()
        H, W = frames[0][0].shape
        tt = self._t(t)
        n_t = tt.numel()
        if out is None:
            out = empty_frame(fmt, H, W, self.device)
        if ws is None:
            ws = self.workspace(H, W, n_t)
        io = self.make_io(frames, tt, fmt, fmt, [out], H, W)
        io.n_t = n_t
        w0, w1, w = weights
        code = self._forward_io(io, lead, w0, w1, w, ws, stream)
        if code != 0:
            raise self._api.error(self._api.prefix + "_forward", code)
        return out


class NativeShutter(_NativeForward):
    """fldr_shutter_forward on a fldr_model.NativeModel: NativeVideo's forward into scratch frames, then one mix."""

    _api = _API

    def forward_io(self, io, w0, w1, w, ws, stream=None):
        """The raw call; returns the code without raising."""
        return self._forward_io(io, (), w0, w1, w, ws, stream)

    def forward(self, frames, t, weights, fmt=None, out=None, ws=None, stream=None):
        """frames: (I0, I1) in fmt; t: the n_t sub-frame times as NativeVideo.forward takes them; weights: (w0, w1, [w of each
        sub-frame]).  -> the one output frame."""
        return self._forward((), frames, t, weights, fmt, out, ws, stream)


class _WindowStream(fldr_video.HostStream):
    """What Converter and fldr_light.Converter share: the handle of a converter of the library `_api` over the window rule, the staged
    outputs and their Info, push / flush / reset.  A subclass builds its config and hands it to _open."""

    _api = _API

    def _destroy(self, h):
        self._api.fn("destroy")(h)

    def _open(self, native_model, cfg, H, W, fmt):
        self._h = ctypes.c_void_p()
        self.model = native_model                                    # the converter uses the model: keep it alive
        self._api.call("create", native_model._h, ctypes.byref(cfg), ctypes.byref(self._h))
        self.H, self.W, self.format = int(H), int(W), fmt
        self.max_out = self._api.fn("max_out")(self._h)
        self._stage(fmt, H, W, self.max_out)
        self._info = (Info * self.max_out)()
        self.last_scene, self.last_info = None, []

    def _done(self, n):
        self.last_info = [self._info[k].as_dict() for k in range(n)]
        return self._taken(n)

    def push(self, frame):
        """-> the list of output frames due (tuples of numpy planes, fresh copies); self.last_info, self.last_scene."""
        fr = frame_struct(frame)
        n = ctypes.c_int(-1)
        res = SceneResult()
        self._api.call("push", self._h, ctypes.byref(fr), self._out_structs(), self._info, ctypes.byref(n), ctypes.byref(res))
        self.last_scene = res.as_dict()
        return self._done(n.value)

    def flush(self):
        n = ctypes.c_int(-1)
        self._api.call("flush", self._h, self._out_structs(), self._info, ctypes.byref(n))
        return self._done(n.value)

    def reset(self):
        self._api.call("reset", self._h)


class Converter(_WindowStream):
    """fldr_shutter: host frames (tuples of numpy planes) pushed one by one at in_rate; each push returns the output frames at out_rate
    whose exposure window it completes (schedule()), flush() the one still open."""

    def __init__(self, native_model, H, W, fmt=None, in_rate=120, out_rate=24, shutter=(1, 2), sub=1, scene=True, params=None):
        fmt = fmt or Format()
        self._open(native_model, config(in_rate, out_rate, shutter, sub, H, W, fmt, native_model.device.index or 0, scene, params), H, W, fmt)
