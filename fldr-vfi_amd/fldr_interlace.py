"""ctypes binding of libfldr_interlace.so (interlace API: include/fldr_interlace.h) — progressive video to interlaced video with true
fields: the weave of two progressive frames through a vertical anti-twitter filter, the forward that interpolates a pair at n_t times and
weaves each result into the rows of one parity, and the stream that puts every field at its own instant.

    out = weave(even, odd, out, Format("nv12"), filter=LINEAR)     # rows y % 2 == 0 from even, y % 2 == 1 from odd; either may be None
    ni = NativeInterlace(fldr_model.NativeModel.from_npz(fldr_harness.DEFAULT_WEIGHTS))
    outs, fields, scene = ni.forward((f0, f1), t=[0.4, 0.8], outs=[w, w], parity=[0, 1], fmt=Format("nv12"))
    c = Interlacer(native_model, H, W, Format("i420"), in_rate=(24000, 1001), out_rate=(30000, 1001))   # 23.976p -> 59.94i
    frames = c.push((y, u, v)); ...; frames = c.flush()            # c.last_reports: one dict per returned frame

plan(k, in_rate, out_rate, tff) is the library's schedule of output frame k (pure host arithmetic).  Frames are fldr_video's: tuples of
2-D plane tensors (device) or numpy arrays (host).  weave and forward enqueue on torch's current stream.  No fallback: a missing library
raises at load.
"""
import ctypes
import os

import torch

import fldr_rate
from fldr_rate import E_ARG, E_DEVICE, E_FORMAT, E_RATIO, E_STATE, RateConfig, SceneParams, _ref, rate_config  # noqa: F401  (this library's codes are the rate library's)
from fldr_video import IO, Format, Frame, _stream_ptr, frame_struct
import fldr_video

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfldr_interlace.so")
INTERLACE_VERSION = 100           # include/fldr_interlace.h: FLDR_INTERLACE_VERSION
NONE, LINEAR, COMPLEX = 0, 1, 2
FILTERS = {"none": NONE, "linear": LINEAR, "complex": COMPLEX}


class InterlaceIO(ctypes.Structure):
    _fields_ = [("pair", IO), ("parity", ctypes.POINTER(ctypes.c_int32)), ("filter", ctypes.c_int32), ("scene_params", SceneParams),
                ("scene", ctypes.c_int32), ("reserved", ctypes.c_int32 * 4)]


class InterlaceConfig(ctypes.Structure):
    _fields_ = [("rate", RateConfig), ("tff", ctypes.c_int32), ("filter", ctypes.c_int32), ("reserved", ctypes.c_int32 * 4)]


class Schedule(ctypes.Structure):
    _fields_ = [("frame", ctypes.c_int64), ("input", ctypes.c_int64 * 2), ("r", ctypes.c_int64 * 2), ("B", ctypes.c_int64), ("push", ctypes.c_int64),
                ("parity", ctypes.c_int32 * 2), ("reserved", ctypes.c_int32 * 2)]

    def as_dict(self):
        return {"frame": int(self.frame), "input": [int(v) for v in self.input], "r": [int(v) for v in self.r], "B": int(self.B),
                "parity": [int(v) for v in self.parity], "push": int(self.push)}


class Report(ctypes.Structure):
    _fields_ = [("frame", ctypes.c_int64), ("input", ctypes.c_int64 * 2), ("r", ctypes.c_int64 * 2), ("cut", ctypes.c_uint32 * 2),
                ("held", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 3)]

    def as_dict(self):
        return {"frame": int(self.frame), "input": [int(v) for v in self.input], "r": [int(v) for v in self.r], "cut": [int(v) for v in self.cut],
                "held": int(self.held), "reserved": [int(v) for v in self.reserved]}


_FRAME_P = ctypes.POINTER(Frame)
_SIGNATURES = {
    "fldr_interlace_version": (ctypes.c_int, []),
    "fldr_interlace_error_string": (ctypes.c_char_p, [ctypes.c_int]),
    "fldr_interlace_sizeof": (ctypes.c_int, [ctypes.c_int]),
    "fldr_interlace_weave": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(Format), _FRAME_P, _FRAME_P, ctypes.c_int, _FRAME_P,
                                            ctypes.c_void_p]),
    "fldr_interlace_workspace_bytes": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "fldr_interlace_field_frame": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(Format), ctypes.c_int, ctypes.c_int,
                                                  ctypes.c_void_p, _FRAME_P]),
    "fldr_interlace_scene_state": (ctypes.c_void_p, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "fldr_interlace_forward": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(InterlaceIO), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "fldr_interlace_plan": (ctypes.c_int, [ctypes.POINTER(InterlaceConfig), ctypes.c_int64, ctypes.POINTER(Schedule)]),
    "fldr_interlace_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(InterlaceConfig), ctypes.POINTER(ctypes.c_void_p)]),
    "fldr_interlace_max_out": (ctypes.c_int, [ctypes.c_void_p]),
    "fldr_interlace_push": (ctypes.c_int, [ctypes.c_void_p, _FRAME_P, _FRAME_P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(Report)]),
    "fldr_interlace_flush": (ctypes.c_int, [ctypes.c_void_p, _FRAME_P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(Report)]),
    "fldr_interlace_reset": (ctypes.c_int, [ctypes.c_void_p]),
    "fldr_interlace_destroy": (None, [ctypes.c_void_p]),
}
EXPORTS = tuple(_SIGNATURES)
_API = fldr_rate.Binding("interlace", LIB_PATH, INTERLACE_VERSION, _SIGNATURES, (InterlaceIO, InterlaceConfig, Schedule, Report), "InterlaceError")
InterlaceError, lib, _check = _API.Error, _API.lib, _API.check


# ---- the weave -------------------------------------------------------------------------------------------------------------------------
def weave_raw(H, W, fmt, even, odd, filter, out, stream_ptr):
    """The raw call on Frame structs (None = NULL); returns the code without raising (tests of the error contract)."""
    return lib().fldr_interlace_weave(int(H), int(W), _ref(fmt), _ref(even), _ref(odd), int(filter), _ref(out), stream_ptr)


def weave(even, odd, out, fmt, filter=NONE, stream=None):
    """fldr_interlace_weave into `out` (a tuple of device plane tensors): its rows y % 2 == 0 from `even`, its rows y % 2 == 1 from `odd`
    (either may be None: those rows are not written), each through `filter`.  Enqueues on torch's current stream."""
    H, W = out[0].shape
    fr = [frame_struct(f) if f is not None else None for f in (even, odd, out)]
    _check(weave_raw(H, W, fmt, fr[0], fr[1], filter, fr[2], _stream_ptr(out[0].device, stream)), "fldr_interlace_weave")
    return out


# ---- the forward -----------------------------------------------------------------------------------------------------------------------
class NativeInterlace(fldr_video.NativeVideo):
    """fldr_interlace_forward on a fldr_model.NativeModel: the pair interpolated at n_t times into temporaries, each woven into the rows
    of one parity of its output frame."""

    def __init__(self, native_model):
        lib()
        super().__init__(native_model)

    def workspace_bytes(self, H, W, n_t=1):
        n = lib().fldr_interlace_workspace_bytes(self.model._h, int(H), int(W), int(n_t))
        if n < 0:
            raise InterlaceError("fldr_interlace_workspace_bytes", int(n))
        return int(n)

    def field_frame(self, ws, H, W, fmt, n_t, k):
        """Temporary k of a forward with n_t outputs in the workspace tensor ws: a tuple of plane views (pitches are multiples of 16)."""
        fr = Frame()
        _check(lib().fldr_interlace_field_frame(self.model._h, int(H), int(W), ctypes.byref(fmt), int(n_t), int(k), ctypes.c_void_p(ws.data_ptr()),
                                                ctypes.byref(fr)), "fldr_interlace_field_frame")
        planes = []
        for p, (rows, cols) in enumerate(fldr_video.plane_shapes(fmt, H, W)):
            off, pitch = fr.plane[p] - ws.data_ptr(), fr.pitch[p]
            raw = ws[off:off + pitch * rows].view(rows, pitch)
            planes.append(raw.view(torch.uint16)[:, :cols] if fmt.bits == 10 else raw[:, :cols])
        return tuple(planes)

    def scene_of(self, ws, H, W, n_t):
        """The scene state inside a workspace used by a forward with n_t outputs (a view)."""
        p = lib().fldr_interlace_scene_state(self.model._h, int(H), int(W), int(n_t), ctypes.c_void_p(ws.data_ptr()))
        off = p - ws.data_ptr()
        return ws[off:off + fldr_rate.SCENE_STATE_BYTES]

    def make_interlace_io(self, frames, t, fmt, outs, parity, filter, scene, params, H, W):
        io = InterlaceIO()
        pair = self.make_io(frames, t, fmt, fmt, outs, H, W)
        io.pair, io._keep_out = pair, pair._keep                     # the struct is copied: the array of output frames must outlive it
        arr = (ctypes.c_int32 * len(parity))(*[int(p) for p in parity])
        io.parity, io._keep_parity = ctypes.cast(arr, ctypes.POINTER(ctypes.c_int32)), arr
        io.filter, io.scene = int(filter), 1 if scene else 0
        if params is not None:
            io.scene_params = params if isinstance(params, SceneParams) else SceneParams(*params)
        return io

    def forward_raw(self, io, ws, ws_bytes=None, stream=None, model=True):
        """The raw call; returns the code without raising."""
        return lib().fldr_interlace_forward(self.model._h if model else None, _ref(io), ctypes.c_void_p(ws.data_ptr()) if ws is not None else None,
                                            (ws.numel() if ws is not None else 0) if ws_bytes is None else int(ws_bytes),
                                            _stream_ptr(self.device, stream))

    def forward(self, frames, t, outs, parity, fmt=None, filter=LINEAR, scene=True, params=None, ws=None, stream=None, read=True):
        """frames: (I0, I1) in fmt; t: n_t times; outs[k]: the woven frame field k goes into, parity[k] the rows it fills.  -> (outs, the
        n_t temporary frames, the pair's scene dict — None with scene=False or read=False)."""
        fmt = fmt or Format()
        H, W = frames[0][0].shape
        tt = self._t(t)
        n_t = tt.numel()
        if ws is None:
            ws = self.workspace(H, W, n_t)
        io = self.make_interlace_io(frames, tt, fmt, outs, parity, filter, scene, params, H, W)
        _check(self.forward_raw(io, ws, stream=stream), "fldr_interlace_forward")
        fields = [self.field_frame(ws, H, W, fmt, n_t, k) for k in range(n_t)]
        return outs, fields, (fldr_rate.read_result(self.scene_of(ws, H, W, n_t)) if scene and read else None)


# ---- the stream ------------------------------------------------------------------------------------------------------------------------
def make_config(H, W, fmt, in_rate, out_rate, tff=True, filter=LINEAR, scene=True, device=0, scene_params=None):
    cfg = InterlaceConfig()
    rate_config(H, W, fmt, in_rate, out_rate, scene, scene_params, device, into=cfg.rate)
    cfg.tff, cfg.filter = 1 if tff else 0, int(filter)
    return cfg


def plan_raw(cfg, k):
    """fldr_interlace_plan -> (code, Schedule); does not raise."""
    s = Schedule()
    return lib().fldr_interlace_plan(_ref(cfg), int(k), ctypes.byref(s)), s


def plan(k, in_rate, out_rate, tff=True):
    """The library's schedule of output frame k at these rates (out_rate in interlaced frames per second) -> dict."""
    code, s = plan_raw(make_config(4, 4, Format(), in_rate, out_rate, tff), k)
    _check(code, "fldr_interlace_plan")
    return s.as_dict()


class Interlacer(fldr_video.ReportStream):
    """fldr_interlace: progressive host frames (tuples of numpy planes) pushed one by one at in_rate; each push returns the woven frames
    at out_rate (interlaced frames per second) whose second field it computed, flush() the frame the end of the stream completes.
    native_model may be None where no field is interpolated (in_rate a multiple of the field rate)."""

    _lib, _check, _Report = staticmethod(lib), staticmethod(_check), Report
    _calls = ("fldr_interlace_destroy", "fldr_interlace_push", "fldr_interlace_flush", "fldr_interlace_reset")

    def __init__(self, native_model, H, W, fmt=None, in_rate=24, out_rate=30, tff=True, filter=LINEAR, scene=True, scene_params=None, device=0):
        fmt = fmt or Format()
        if native_model is not None:
            device = native_model.device.index or 0
        self.cfg = make_config(H, W, fmt, in_rate, out_rate, tff, filter, scene, device, scene_params)
        self._h = ctypes.c_void_p()
        self.model = native_model                                    # the stream uses the model: keep it alive
        _check(lib().fldr_interlace_create(native_model._h if native_model is not None else None, ctypes.byref(self.cfg), ctypes.byref(self._h)),
               "fldr_interlace_create")
        self.H, self.W, self.format = int(H), int(W), fmt
        self.max_out = lib().fldr_interlace_max_out(self._h)
        self._stage(fmt, H, W, self.max_out)
        self.last_reports = []

    def plan(self, k):
        """The schedule of output frame k of this stream -> dict."""
        code, s = plan_raw(self.cfg, k)
        _check(code, "fldr_interlace_plan")
        return s.as_dict()
