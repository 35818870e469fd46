"""ctypes binding of libfldr_scale.so (scale API: include/fldr_scale.h) — resizing of YUV 4:2:0 video on the device, placed on the cheaper
side of the frame interpolation: the table builder, the map (the tables of one in size -> out size on the device), the kernel entry
that scales one device frame, the forward that scales before or after interpolating, and the stream that changes size and rate.

    n, left, coef = taps(1080, 2160, LANCZOS3, LUMA)               # pure host arithmetic: the table of one axis
    m = Map((1080, 1920), (2160, 3840), Format("nv12"), LANCZOS3)  # m.where, m.taps, m.tile: what the create resolved and picked
    m.frame(src, dst)                                              # device frames (tuples of plane tensors), on torch's current stream
    ns = NativeScale(fldr_model.NativeModel.from_npz(fldr_harness.DEFAULT_WEIGHTS))
    outs, temps, scene = ns.forward(m, (f0, f1), t=[0.4, 0.8], outs=[a, b])
    c = Scaler(native_model, (1080, 1920), (2160, 3840), Format("i420"), in_rate=24, out_rate=60)      # 1080p24 -> 2160p60
    frames = c.push((y, u, v)); ...; frames = c.flush()            # c.last_scene: the measure of the pair just pushed; c.where

Sizes are (H, W).  Frames are fldr_video's: tuples of 2-D plane tensors (device) or numpy arrays (host).  No fallback: a missing library
raises at load.
"""
import ctypes
import os

import numpy as np
import torch

import fldr_rate
from fldr_rate import E_ARG, E_DEVICE, E_FORMAT, E_RATIO, E_STATE, RateConfig, SceneParams, SceneResult, _ref, rate_config  # noqa: F401  (this library's codes are the rate library's)
from fldr_video import IO, Format, Frame, _stream_ptr, frame_struct
import fldr_video

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfldr_scale.so")
SCALE_VERSION = 100               # include/fldr_scale.h: FLDR_SCALE_VERSION
MAX_SIZE, MAX_TAPS = 16384, 64
MAP_LIVE = 0x5ca1e001             # fldr_scale_map.live of a created map
BILINEAR, BICUBIC, LANCZOS3 = 0, 1, 2
FILTERS = {"bilinear": BILINEAR, "bicubic": BICUBIC, "lanczos": LANCZOS3}
LUMA, CHROMA_H, CHROMA_V = 0, 1, 2
BEFORE, AFTER, AUTO = 0, 1, 2
WHERE = {"before": BEFORE, "after": AFTER, "auto": AUTO}
READ_AUTO, READ_DIRECT, READ_STAGED = 0, 1, 2     # how the kernel's horizontal pass reads its source


class MapConfig(ctypes.Structure):
    _fields_ = [("in_H", ctypes.c_int32), ("in_W", ctypes.c_int32), ("out_H", ctypes.c_int32), ("out_W", ctypes.c_int32), ("format", Format),
                ("filter", ctypes.c_int32), ("device", ctypes.c_int32), ("where", ctypes.c_int32), ("read", ctypes.c_int32), ("reserved", ctypes.c_int32 * 3)]


class MapStruct(ctypes.Structure):
    _fields_ = [("cfg", MapConfig), ("where", ctypes.c_int32), ("taps_x", ctypes.c_int32), ("taps_y", ctypes.c_int32), ("tile_w", ctypes.c_int32 * 2),
                ("tile_h", ctypes.c_int32 * 2), ("lds_bytes", ctypes.c_int32), ("live", ctypes.c_int32), ("tables", ctypes.c_void_p),
                ("offset", ctypes.c_int64 * 8), ("read", ctypes.c_int32), ("stage_span", ctypes.c_int32 * 2), ("stage_at", ctypes.c_int32)]


class ScaleIO(ctypes.Structure):
    _fields_ = [("v", IO), ("scene", ctypes.c_int32), ("scene_params", SceneParams), ("reserved", ctypes.c_int32 * 4)]


class ScaleConfig(ctypes.Structure):
    _fields_ = [("rate", RateConfig), ("out_H", ctypes.c_int32), ("out_W", ctypes.c_int32), ("filter", ctypes.c_int32), ("where", ctypes.c_int32),
                ("reserved", ctypes.c_int32 * 4)]


_FRAME_P = ctypes.POINTER(Frame)
_MAP_P = ctypes.POINTER(MapStruct)
_SIGNATURES = {
    "fldr_scale_version": (ctypes.c_int, []),
    "fldr_scale_error_string": (ctypes.c_char_p, [ctypes.c_int]),
    "fldr_scale_sizeof": (ctypes.c_int, [ctypes.c_int]),
    "fldr_scale_taps_count": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "fldr_scale_taps": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "fldr_scale_map_create": (ctypes.c_int, [ctypes.POINTER(MapConfig), _MAP_P]),
    "fldr_scale_map_destroy": (None, [_MAP_P]),
    "fldr_scale_frame": (ctypes.c_int, [_MAP_P, _FRAME_P, _FRAME_P, ctypes.c_void_p]),
    "fldr_scale_workspace_bytes": (ctypes.c_int64, [ctypes.c_void_p, _MAP_P, ctypes.c_int]),
    "fldr_scale_temp_frame": (ctypes.c_int, [ctypes.c_void_p, _MAP_P, ctypes.POINTER(Format), ctypes.c_int, ctypes.c_int, ctypes.c_void_p, _FRAME_P]),
    "fldr_scale_forward": (ctypes.c_int, [ctypes.c_void_p, _MAP_P, ctypes.POINTER(ScaleIO), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "fldr_scale_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ScaleConfig), ctypes.POINTER(ctypes.c_void_p)]),
    "fldr_scale_max_out": (ctypes.c_int, [ctypes.c_void_p]),
    "fldr_scale_push": (ctypes.c_int, [ctypes.c_void_p, _FRAME_P, _FRAME_P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(SceneResult)]),
    "fldr_scale_flush": (ctypes.c_int, [ctypes.c_void_p, _FRAME_P, ctypes.POINTER(ctypes.c_int)]),
    "fldr_scale_reset": (ctypes.c_int, [ctypes.c_void_p]),
    "fldr_scale_destroy": (None, [ctypes.c_void_p]),
}
EXPORTS = tuple(_SIGNATURES)
_API = fldr_rate.Binding("scale", LIB_PATH, SCALE_VERSION, _SIGNATURES, (MapConfig, MapStruct, ScaleIO, ScaleConfig), "ScaleError")
ScaleError, lib, _check = _API.Error, _API.lib, _API.check


# ---- the tables ------------------------------------------------------------------------------------------------------------------------
def outputs(luma_out, kind):
    """The outputs of a table: luma_out, or ceil(luma_out / 2) for the chroma kinds."""
    return int(luma_out) if kind == LUMA else (int(luma_out) + 1) // 2


def taps_count(luma_in, luma_out, filter):
    """fldr_scale_taps_count: n, or the negative code (does not raise)."""
    return lib().fldr_scale_taps_count(int(luma_in), int(luma_out), int(filter))


def taps(luma_in, luma_out, filter, kind):
    """fldr_scale_taps -> (n, left [outputs] int32, coef [outputs, n] int16)."""
    n = taps_count(luma_in, luma_out, filter)
    _check(min(n, 0), "fldr_scale_taps_count")
    left = np.zeros(outputs(luma_out, kind), np.int32)
    coef = np.zeros((left.size, n), np.int16)
    _check(lib().fldr_scale_taps(int(luma_in), int(luma_out), int(filter), int(kind), left.ctypes.data, coef.ctypes.data), "fldr_scale_taps")
    return n, left, coef


def tables(in_size, out_size, filter):
    """The library's four axis tables of (H, W) -> (H, W), as tests/scale_oracle.scale takes them:
    {"luma_x", "luma_y", "chroma_x", "chroma_y"} -> (left, coef)."""
    (iH, iW), (oH, oW) = in_size, out_size
    return {"luma_x": taps(iW, oW, filter, LUMA)[1:], "luma_y": taps(iH, oH, filter, LUMA)[1:],
            "chroma_x": taps(iW, oW, filter, CHROMA_H)[1:], "chroma_y": taps(iH, oH, filter, CHROMA_V)[1:]}


# ---- the map and the kernel entry --------------------------------------------------------------------------------------------------------
def map_config(in_size, out_size, fmt, filter=LANCZOS3, where=AUTO, device=0, read=READ_AUTO):
    cfg = MapConfig()
    (cfg.in_H, cfg.in_W), (cfg.out_H, cfg.out_W) = in_size, out_size
    cfg.format, cfg.filter, cfg.where, cfg.device, cfg.read = fmt, int(filter), int(where), int(device), int(read)
    return cfg


def map_create_raw(cfg, m):
    """The raw call (None = NULL); returns the code without raising."""
    return lib().fldr_scale_map_create(_ref(cfg), _ref(m))


def frame_raw(m, src, dst, stream_ptr):
    """fldr_scale_frame on a MapStruct and Frame structs (None = NULL); returns the code without raising."""
    return lib().fldr_scale_frame(_ref(m), _ref(src), _ref(dst), stream_ptr)


class Map:
    """fldr_scale_map: the tables of in_size -> out_size ((H, W) each) in `fmt` on `device`; read-only after the create."""

    def __init__(self, in_size, out_size, fmt=None, filter=LANCZOS3, where=AUTO, device=0, read=READ_AUTO):
        self.format = fmt or Format()
        self.cfg = map_config(in_size, out_size, self.format, filter, where, device, read)
        self.struct = MapStruct()
        _check(map_create_raw(self.cfg, self.struct), "fldr_scale_map_create")
        self.in_size, self.out_size, self.filter = tuple(in_size), tuple(out_size), int(filter)
        self.where = int(self.struct.where)
        self.taps = (int(self.struct.taps_x), int(self.struct.taps_y))
        self.tile = [(int(self.struct.tile_h[j]), int(self.struct.tile_w[j])) for j in range(2)]       # (rows, samples) of luma, chroma
        self.lds_bytes = int(self.struct.lds_bytes)
        self.read = int(self.struct.read)                            # READ_DIRECT or READ_STAGED: what the create resolved

    def frame(self, src, dst, stream=None):
        """fldr_scale_frame: src (in_size) -> dst (out_size), tuples of device plane tensors.  Enqueues on torch's current stream."""
        _check(frame_raw(self.struct, frame_struct(src), frame_struct(dst), _stream_ptr(dst[0].device, stream)), "fldr_scale_frame")
        return dst

    def close(self):
        if self.struct is not None:
            lib().fldr_scale_map_destroy(ctypes.byref(self.struct))
        self.struct = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- the forward -----------------------------------------------------------------------------------------------------------------------
class NativeScale(fldr_video.NativeVideo):
    """fldr_scale_forward on a fldr_model.NativeModel: a pair scaled and interpolated in the order the map's placement says."""

    def __init__(self, native_model):
        lib()
        super().__init__(native_model)

    def forward_size(self, m):
        return m.out_size if m.where == BEFORE else m.in_size

    def workspace_bytes(self, m, n_t=1):
        n = lib().fldr_scale_workspace_bytes(self.model._h, ctypes.byref(m.struct), int(n_t))
        if n < 0:
            raise ScaleError("fldr_scale_workspace_bytes", int(n))
        return int(n)

    def workspace(self, m, n_t=1):
        return torch.empty(self.workspace_bytes(m, n_t), dtype=torch.uint8, device=self.device)

    def temp_frame(self, m, ws, n_t, k):
        """Temporary k of a forward with n_t outputs in the workspace tensor ws: a tuple of plane views (pitches are multiples of 16)."""
        fr = Frame()
        _check(lib().fldr_scale_temp_frame(self.model._h, ctypes.byref(m.struct), ctypes.byref(m.format), int(n_t), int(k),
                                           ctypes.c_void_p(ws.data_ptr()), ctypes.byref(fr)), "fldr_scale_temp_frame")
        H, W = self.forward_size(m)
        planes = []
        for p, (rows, cols) in enumerate(fldr_video.plane_shapes(m.format, H, W)):
            off, pitch = fr.plane[p] - ws.data_ptr(), fr.pitch[p]
            raw = ws[off:off + pitch * rows].view(rows, pitch)
            planes.append(raw.view(torch.uint16)[:, :cols] if m.format.bits == 10 else raw[:, :cols])
        return tuple(planes)

    def scene_of(self, m, ws, n_t):
        """The scene state inside a workspace used by a forward with n_t outputs (a view): fldr_scale.h says where it is."""
        H, W = self.forward_size(m)
        end = fldr_rate.lib().fldr_rate_workspace_bytes(self.model._h, int(H), int(W), int(n_t))
        return ws[end - fldr_rate.SCENE_STATE_BYTES:end]

    def make_scale_io(self, m, frames, t, outs, scene, params):
        io = ScaleIO()
        v = self.make_io(frames, t, m.format, m.format, outs, m.in_size[0], m.in_size[1])
        io.v, io._keep_out = v, v._keep                             # the struct is copied: the array of output frames must outlive it
        io.scene = 1 if scene else 0
        if params is not None:
            io.scene_params = params if isinstance(params, SceneParams) else SceneParams(*params)
        return io

    def forward_raw(self, m, io, ws, ws_bytes=None, stream=None, model=True):
        """The raw call; returns the code without raising."""
        return lib().fldr_scale_forward(self.model._h if model else None, _ref(m.struct if m is not None else None), _ref(io),
                                        ctypes.c_void_p(ws.data_ptr()) if ws is not None else None,
                                        (ws.numel() if ws is not None else 0) if ws_bytes is None else int(ws_bytes), _stream_ptr(self.device, stream))

    def forward(self, m, frames, t, outs, scene=True, params=None, ws=None, stream=None, read=True):
        """frames: (I0, I1) at m.in_size; t: n_t times; outs: n_t frames at m.out_size.  -> (outs, the temporaries — 2 under BEFORE, n_t
        under AFTER —, the pair's scene dict — None with scene=False or read=False)."""
        tt = self._t(t)
        n_t = tt.numel()
        if ws is None:
            ws = self.workspace(m, n_t)
        io = self.make_scale_io(m, frames, tt, outs, scene, params)
        _check(self.forward_raw(m, io, ws, stream=stream), "fldr_scale_forward")
        temps = [self.temp_frame(m, ws, n_t, k) for k in range(2 if m.where == BEFORE else n_t)]
        return outs, temps, (fldr_rate.read_result(self.scene_of(m, ws, n_t)) if scene and read else None)


# ---- the stream ------------------------------------------------------------------------------------------------------------------------
def make_config(in_size, out_size, fmt, in_rate, out_rate, filter=LANCZOS3, where=AUTO, scene=True, device=0, scene_params=None):
    cfg = ScaleConfig()
    rate_config(in_size[0], in_size[1], fmt, in_rate, out_rate, scene, scene_params, device, into=cfg.rate)
    cfg.out_H, cfg.out_W, cfg.filter, cfg.where = int(out_size[0]), int(out_size[1]), int(filter), int(where)
    return cfg


class Scaler(fldr_video.HostStream):
    """fldr_scale: host frames (tuples of numpy planes) at in_size pushed one by one at in_rate; each push returns the frames at out_size
    and out_rate that fall before the pushed frame, flush() the one that lands on the last frame.  native_model may be None where the
    rates are equal: a pure scaling stream.  self.where: the resolved placement."""

    _destroy = staticmethod(lambda h: lib().fldr_scale_destroy(h))

    def __init__(self, native_model, in_size, out_size, fmt=None, in_rate=24, out_rate=60, filter=LANCZOS3, where=AUTO, scene=True, scene_params=None,
                 device=0):
        fmt = fmt or Format()
        if native_model is not None:
            device = native_model.device.index or 0
        self.cfg = make_config(in_size, out_size, fmt, in_rate, out_rate, filter, where, scene, device, scene_params)
        self._h = ctypes.c_void_p()
        self.model = native_model                                    # the stream uses the model: keep it alive
        _check(lib().fldr_scale_create(native_model._h if native_model is not None else None, ctypes.byref(self.cfg), ctypes.byref(self._h)),
               "fldr_scale_create")
        self.in_size, self.out_size, self.format, self.where = tuple(in_size), tuple(out_size), fmt, int(self.cfg.where)
        self.max_out = lib().fldr_scale_max_out(self._h)
        self._stage(fmt, out_size[0], out_size[1], self.max_out)
        self.last_scene = None

    def push(self, frame):
        """-> the list of output frames due (tuples of numpy planes, fresh copies); self.last_scene: the pair's scene dict."""
        fr = frame_struct(frame)
        n = ctypes.c_int(-1)
        res = SceneResult()
        _check(lib().fldr_scale_push(self._h, ctypes.byref(fr), self._out_structs(), ctypes.byref(n), ctypes.byref(res)), "fldr_scale_push")
        self.last_scene = res.as_dict()
        return self._taken(n.value)

    def flush(self):
        n = ctypes.c_int(-1)
        _check(lib().fldr_scale_flush(self._h, self._out_structs(), ctypes.byref(n)), "fldr_scale_flush")
        return self._taken(n.value)

    def reset(self):
        _check(lib().fldr_scale_reset(self._h), "fldr_scale_reset")
