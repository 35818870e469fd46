"""ctypes binding of libfldr_field.so (field API: include/fldr_field.h) — motion-compensated deinterlacing of interlaced 4:2:0 video:
the weave kernel alone, the forward on the two neighbouring fields, the schedule and the stream, on top of fldr_rate and fldr_video.

    out = weave(cur, prev, next, temporal, Format("nv12"), parity=0)            # device frames -> the progressive frame
    nf = NativeField(fldr_model.NativeModel.from_npz(fldr_harness.DEFAULT_WEIGHTS))
    out, scene = nf.forward(cur, prev, next, Format("i420"), parity=1)          # measure + model at t = 0.5 on the field views + weave
    s = Stream(native_model, H, W, Format("i420"), tff=True, rate=2)            # woven host frames (numpy planes)
    outs = s.push((y, u, v)); ...; outs = s.flush()                             # s.last_reports: one dict per output

plan(j, tff, rate) is the pure-Python statement of which field output j carries; the tests hold the library to it.  Frames are
fldr_video's: tuples of 2-D plane tensors (device) or numpy arrays (host).  weave and forward enqueue on torch's current stream and
return without synchronising.  No fallback: a missing library raises at load.
"""
import ctypes
import os

import torch

import fldr_model
import fldr_rate
import fldr_video
from fldr_rate import SCENE_STATE_BYTES, SceneParams, SceneResult
from fldr_video import Format, Frame, _stream_ptr, empty_frame, frame_struct, plane_dtype, plane_shapes  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfldr_field.so")
FIELD_VERSION = 100               # include/fldr_field.h: FLDR_FIELD_VERSION
E_ARG, E_SIZE, E_WORKSPACE, E_DEVICE = -1000, -1001, -1002, -1003
MOTION, INTRA = 0, 1
STILL_DEFAULT8, SLACK_DEFAULT8 = 2, 16


class Params(ctypes.Structure):
    _fields_ = [("still", ctypes.c_int32), ("slack", ctypes.c_int32), ("reserved", ctypes.c_int32 * 2)]

    def __init__(self, still=STILL_DEFAULT8, slack=SLACK_DEFAULT8):
        super().__init__(int(still), int(slack))


class IO(ctypes.Structure):
    _fields_ = [("H", ctypes.c_int32), ("W", ctypes.c_int32), ("format", Format), ("cur", Frame), ("prev", Frame), ("next", Frame),
                ("parity", ctypes.c_int32), ("scene", ctypes.c_int32), ("scene_params", SceneParams), ("params", ctypes.POINTER(Params)),
                ("out", Frame), ("reserved", ctypes.c_int32 * 4)]


class Config(ctypes.Structure):
    _fields_ = [("H", ctypes.c_int32), ("W", ctypes.c_int32), ("format", Format), ("tff", ctypes.c_int32), ("rate", ctypes.c_int32),
                ("device", ctypes.c_int32), ("scene", ctypes.c_int32), ("scene_params", SceneParams), ("params", ctypes.POINTER(Params)),
                ("reserved", ctypes.c_int32 * 4)]


class Schedule(ctypes.Structure):
    _fields_ = [("field", ctypes.c_int64), ("cur", ctypes.c_int64), ("prev", ctypes.c_int64), ("next", ctypes.c_int64),
                ("parity", ctypes.c_int32), ("reserved", ctypes.c_int32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k in ("field", "parity", "cur", "prev", "next")}


class Report(ctypes.Structure):
    _fields_ = [("field", ctypes.c_int64), ("parity", ctypes.c_uint32), ("mode_used", ctypes.c_uint32), ("cut", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32), ("scene", SceneResult)]

    def as_dict(self):
        return {"field": int(self.field), "parity": int(self.parity), "mode_used": int(self.mode_used), "cut": int(self.cut),
                "scene": self.scene.as_dict()}


_FRAME_P = ctypes.POINTER(Frame)
_SIGNATURES = {
    "fldr_field_version": (ctypes.c_int, []),
    "fldr_field_error_string": (ctypes.c_char_p, [ctypes.c_int]),
    "fldr_field_sizeof": (ctypes.c_int, [ctypes.c_int]),
    "fldr_field_weave": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(Format), _FRAME_P, _FRAME_P, _FRAME_P, _FRAME_P, ctypes.c_int,
                                        ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(Params), _FRAME_P, ctypes.c_void_p]),
    "fldr_field_workspace_bytes": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]),
    "fldr_field_temporal": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(Format), ctypes.c_void_p, _FRAME_P]),
    "fldr_field_scene_state": (ctypes.c_void_p, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "fldr_field_forward": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(IO), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "fldr_field_plan": (ctypes.c_int, [ctypes.POINTER(Config), ctypes.c_int64, ctypes.POINTER(Schedule)]),
    "fldr_field_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Config), ctypes.POINTER(ctypes.c_void_p)]),
    "fldr_field_max_out": (ctypes.c_int, [ctypes.c_void_p]),
    "fldr_field_push": (ctypes.c_int, [ctypes.c_void_p, _FRAME_P, _FRAME_P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(Report)]),
    "fldr_field_flush": (ctypes.c_int, [ctypes.c_void_p, _FRAME_P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(Report)]),
    "fldr_field_reset": (ctypes.c_int, [ctypes.c_void_p]),
    "fldr_field_destroy": (None, [ctypes.c_void_p]),
}
EXPORTS = tuple(_SIGNATURES)
_lib = None


class FieldError(RuntimeError):
    def __init__(self, what, code):
        super().__init__("%s failed: %s (code %d)" % (what, lib().fldr_field_error_string(code).decode(), code))
        self.code = code


def lib():
    """The loaded libfldr_field.so, checked against this binding (struct sizes, header version); raises when it has not been built."""
    global _lib
    if _lib is None:
        fldr_rate.lib()
        _lib = fldr_model.load_library(LIB_PATH, _SIGNATURES, (Params, IO, Config, Schedule, Report), "fldr_field", FIELD_VERSION)
    return _lib


def _check(code, what):
    if code != 0:
        raise FieldError(what, code)


def _params(params):
    """None, a Params or a (still, slack) pair -> a Params or None."""
    return params if params is None or isinstance(params, Params) else Params(*params)


def _ref(x):
    return ctypes.byref(x) if x is not None else None


# ---- the schedule -----------------------------------------------------------------------------------------------------------------------
def plan(j, tff=True, rate=2):
    """Which field output j of a stream carries: {"field": m, "parity", "cur", "prev", "next"} — m = j at rate 2, 2 j at rate 1; the
    frames holding fields m, m - 1 (-1 for m = 0) and m + 1."""
    m = j if rate == 2 else 2 * j
    return {"field": m, "parity": (m & 1) ^ (0 if tff else 1), "cur": m >> 1, "prev": (m - 1) >> 1 if m else -1, "next": (m + 1) >> 1}


def plan_raw(j, tff, rate):
    """fldr_field_plan -> (code, dict); does not raise."""
    cfg = Config()
    cfg.tff, cfg.rate = int(tff), int(rate)
    s = Schedule()
    code = lib().fldr_field_plan(ctypes.byref(cfg), int(j), ctypes.byref(s))
    return code, s.as_dict()


def pushes(n_frames, tff=True, rate=2):
    """What a stream returns for n_frames frames: a list of n_frames + 1 lists of (plan, mode), entry n the outputs of the push of
    frame n, the last entry those of the flush.  An output goes out with the push of the frame that holds field m + 1; the first field
    and, at the flush, the last one are INTRA."""
    out, j = [[] for _ in range(n_frames + 1)], 0
    for n in range(n_frames):
        while plan(j, tff, rate)["next"] <= n:
            p = plan(j, tff, rate)
            out[n].append((p, INTRA if p["prev"] < 0 else MOTION))
            j += 1
    if n_frames and plan(j, tff, rate)["cur"] <= n_frames - 1:
        out[n_frames].append((plan(j, tff, rate), INTRA))
    return out


# ---- the weave ---------------------------------------------------------------------------------------------------------------------------
def weave_raw(H, W, fmt, cur, prev, next, temporal, parity, mode, intra_if, params, out, stream_ptr):
    """The raw call on Frame structs (or None); returns the code without raising (tests of the error contract)."""
    return lib().fldr_field_weave(int(H), int(W), _ref(fmt), _ref(cur), _ref(prev), _ref(next), _ref(temporal), int(parity), int(mode),
                                  intra_if, _ref(params), _ref(out), stream_ptr)


def weave(cur, prev, next, temporal, fmt, parity, mode=MOTION, intra_if=None, params=None, out=None, stream=None):
    """fldr_field_weave on device frames (tuples of plane tensors in `fmt`, pitches from their strides): cur is H x W and holds the
    field, prev / next hold the fields before / after it, temporal is H/2 x W; all three may be None with mode=INTRA.  intra_if: a
    uint32 / int32 device tensor whose first word forces INTRA when it is non-zero at run time.  -> `out` (allocated packed otherwise)."""
    H, W = cur[0].shape
    device = cur[0].device
    if out is None:
        out = empty_frame(fmt, H, W, device)
    st = lambda f: frame_struct(f) if f is not None else None
    _check(weave_raw(H, W, fmt, st(cur), st(prev), st(next), st(temporal), parity, mode,
                     ctypes.c_void_p(intra_if.data_ptr()) if intra_if is not None else None, _params(params), st(out), _stream_ptr(device, stream)),
           "fldr_field_weave")
    return out


# ---- the forward -------------------------------------------------------------------------------------------------------------------------
def field_view(frame, parity):
    """The field of a frame: the rows y = parity (mod 2) of every plane, as views."""
    return tuple(p[parity::2] for p in frame)


class NativeField:
    """Deinterlacing forwards on a fldr_model.NativeModel (read-only: forwards on several streams, each with its own workspace, may run
    at once)."""

    def __init__(self, native_model):
        lib()
        self.model = native_model
        self.device = native_model.device

    def workspace_bytes(self, H, W):
        n = lib().fldr_field_workspace_bytes(self.model._h, int(H), int(W))
        if n < 0:
            raise FieldError("fldr_field_workspace_bytes", int(n))
        return int(n)

    def workspace(self, H, W):
        return torch.empty(self.workspace_bytes(H, W), dtype=torch.uint8, device=self.device)

    def _plane_views(self, ws, fr, fmt, H, W):
        b = 2 if fmt.bits == 10 else 1
        planes = []
        for p, (r, c) in enumerate(plane_shapes(fmt, H // 2, W)):
            off, pitch = fr.plane[p] - ws.data_ptr(), fr.pitch[p]
            raw = ws[off:off + r * pitch].view(r, pitch)[:, :c * b]
            planes.append(raw.view(torch.uint16) if b == 2 else raw)
        return tuple(planes)

    def temporal(self, ws, H, W, fmt):
        """The H/2 x W temporal frame inside a workspace, as views (fldr_field_temporal)."""
        fr = Frame()
        _check(lib().fldr_field_temporal(self.model._h, int(H), int(W), ctypes.byref(fmt), ctypes.c_void_p(ws.data_ptr()), ctypes.byref(fr)),
               "fldr_field_temporal")
        return self._plane_views(ws, fr, fmt, H, W)

    def scene_result(self, ws, H, W):
        """The fldr_scene_result of the last forward with scene=1 in this workspace (synchronising copy) -> dict."""
        ptr = lib().fldr_field_scene_state(self.model._h, int(H), int(W), ctypes.c_void_p(ws.data_ptr()))
        off = ptr - ws.data_ptr()
        return SceneResult.from_buffer_copy(ws[off:off + ctypes.sizeof(SceneResult)].cpu().numpy().tobytes()).as_dict()

    def make_io(self, cur, prev, next, fmt, parity, scene, scene_params, params, out):
        H, W = cur[0].shape
        io = IO()
        io.H, io.W, io.format = int(H), int(W), fmt
        io.cur, io.prev, io.next, io.out = frame_struct(cur), frame_struct(prev), frame_struct(next), frame_struct(out)
        io.parity, io.scene = int(parity), 1 if scene else 0
        if scene_params is not None:
            io.scene_params = scene_params if isinstance(scene_params, SceneParams) else SceneParams(*scene_params)
        p = _params(params)
        if p is not None:
            io.params = ctypes.pointer(p)
        io._keep = p
        return io

    def forward_io(self, io, ws, stream=None, model=True):
        """The raw call; returns the code without raising (tests of the error contract)."""
        return lib().fldr_field_forward(self.model._h if model else None, ctypes.byref(io), ctypes.c_void_p(ws.data_ptr()) if ws is not None else None,
                                        ws.numel() if ws is not None else 0, _stream_ptr(self.device, stream))

    def forward(self, cur, prev, next, fmt, parity, scene=False, scene_params=None, params=None, out=None, ws=None, stream=None):
        """fldr_field_forward on device frames: -> `out` (allocated packed otherwise).  With scene=True the pair's result is read with
        scene_result(ws, H, W) after a synchronisation."""
        H, W = cur[0].shape
        if out is None:
            out = empty_frame(fmt, H, W, self.device)
        if ws is None:
            ws = self.workspace(H, W)
        io = self.make_io(cur, prev, next, fmt, parity, scene, scene_params, params, out)
        _check(self.forward_io(io, ws, stream), "fldr_field_forward")
        return out


# ---- the stream ---------------------------------------------------------------------------------------------------------------------------
def make_config(H, W, fmt, tff=True, rate=2, scene=True, device=0, scene_params=None, params=None):
    cfg = Config()
    cfg.H, cfg.W, cfg.format = int(H), int(W), fmt
    cfg.tff, cfg.rate, cfg.device, cfg.scene = 1 if tff else 0, int(rate), int(device), 1 if scene else 0
    if scene_params is not None:
        cfg.scene_params = scene_params if isinstance(scene_params, SceneParams) else SceneParams(*scene_params)
    p = _params(params)
    if p is not None:
        cfg.params = ctypes.pointer(p)
    cfg._keep = p
    return cfg


class Stream(fldr_video.ReportStream):
    """fldr_field: woven frames (tuples of numpy planes) pushed one by one; each push returns the progressive frames that became
    computable, flush() the last field at rate 2.  last_reports: one dict per frame of the last call."""

    _lib, _check, _Report = staticmethod(lib), staticmethod(_check), Report
    _calls = ("fldr_field_destroy", "fldr_field_push", "fldr_field_flush", "fldr_field_reset")

    def __init__(self, native_model, H, W, fmt=None, tff=True, rate=2, scene=True, scene_params=None, params=None):
        fmt = fmt or Format()
        cfg = make_config(H, W, fmt, tff, rate, scene, native_model.device.index or 0, scene_params, params)
        self._h = ctypes.c_void_p()
        self.model = native_model                                    # the stream uses the model: keep it alive
        _check(lib().fldr_field_create(native_model._h, ctypes.byref(cfg), ctypes.byref(self._h)), "fldr_field_create")
        self.H, self.W, self.format, self.tff, self.rate = int(H), int(W), fmt, bool(tff), int(rate)
        self.max_out = lib().fldr_field_max_out(self._h)
        self._stage(fmt, H, W, self.max_out)
        self.last_reports = []
