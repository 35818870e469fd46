"""ctypes binding of libfldr_conform.so (conform API: include/fldr_conform.h) — direct YUV 4:2:0 -> YUV 4:2:0 conversion on the device
between any two formats (matrix, range, depth with optional ordered dither, layout), with the picture placed on a larger black canvas:
the coefficient table, the crop view, the kernel entry that conforms one device frame, and the stream that changes format, canvas and rate.

    k = coefs(Format("nv12", "bt601"), Format("nv12", "bt709", depth=10))          # pure host arithmetic: the seven 14-bit coefficients
    frame(src, Format("nv12", "bt601"), dst, Format("nv12", "bt709", depth=10))    # device frames (tuples of plane tensors), torch's stream
    frame(src, fin, dst, fout, at=(152, 0), dither=True)                           # pillarbox: the picture's top-left luma sample at x, y
    win = view(src, fin, 64, 32, (480, 640))                                       # the 480 x 640 window of src that starts at x 64, y 32
    c = Conformer(native_model, (576, 720), Format("i420", "bt601"), (576, 1024), Format("i420", "bt709", depth=10), 25, 50, at=(152, 0))
    frames = c.push((y, u, v)); ...; frames = c.flush()                            # c.last_scene: the measure of the pair just pushed

Sizes are (H, W); `at` is (x, y).  Frames are fldr_video's: tuples of 2-D plane tensors (device) or numpy arrays (host).  No fallback: a
missing library raises at load.
"""
import ctypes
import os

import numpy as np

import fldr_rate
from fldr_rate import E_ARG, E_DEVICE, E_FORMAT, E_RATIO, E_STATE, RateConfig, SceneResult, _ref, rate_config  # noqa: F401  (this library's codes are the rate library's)
from fldr_video import Format, Frame, _stream_ptr, frame_struct, plane_shapes
import fldr_video

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfldr_conform.so")
CONFORM_VERSION = 100             # include/fldr_conform.h: FLDR_CONFORM_VERSION
MAX_SIZE = 16384
DITHER_NONE, DITHER_ORDERED = 0, 1
KYY, KYU, KYV, KUU, KUV, KVU, KVV = range(7)
# the kernel's own constants (conform/conform_internal.h): a lane owns RUN_BYTES of an output row, a workgroup THREADS consecutive runs
RUN_BYTES, THREADS = 16, 256


class Config(ctypes.Structure):
    _fields_ = [("in_H", ctypes.c_int32), ("in_W", ctypes.c_int32), ("in_format", Format), ("out_H", ctypes.c_int32), ("out_W", ctypes.c_int32),
                ("out_format", Format), ("dst_x", ctypes.c_int32), ("dst_y", ctypes.c_int32), ("dither", ctypes.c_int32), ("reserved", ctypes.c_int32 * 3)]


class StreamConfig(ctypes.Structure):
    _fields_ = [("rate", RateConfig), ("out_H", ctypes.c_int32), ("out_W", ctypes.c_int32), ("out_format", Format), ("dst_x", ctypes.c_int32),
                ("dst_y", ctypes.c_int32), ("dither", ctypes.c_int32), ("reserved", ctypes.c_int32 * 4)]


_FRAME_P = ctypes.POINTER(Frame)
_FORMAT_P = ctypes.POINTER(Format)
_SIGNATURES = {
    "fldr_conform_version": (ctypes.c_int, []),
    "fldr_conform_error_string": (ctypes.c_char_p, [ctypes.c_int]),
    "fldr_conform_sizeof": (ctypes.c_int, [ctypes.c_int]),
    "fldr_conform_coefs": (ctypes.c_int, [_FORMAT_P, _FORMAT_P, ctypes.c_void_p]),
    "fldr_conform_view": (ctypes.c_int, [_FRAME_P, _FORMAT_P, ctypes.c_int, ctypes.c_int, _FRAME_P]),
    "fldr_conform_frame": (ctypes.c_int, [ctypes.POINTER(Config), _FRAME_P, _FRAME_P, ctypes.c_void_p]),
    "fldr_conform_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(StreamConfig), ctypes.POINTER(ctypes.c_void_p)]),
    "fldr_conform_max_out": (ctypes.c_int, [ctypes.c_void_p]),
    "fldr_conform_push": (ctypes.c_int, [ctypes.c_void_p, _FRAME_P, _FRAME_P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(SceneResult)]),
    "fldr_conform_flush": (ctypes.c_int, [ctypes.c_void_p, _FRAME_P, ctypes.POINTER(ctypes.c_int)]),
    "fldr_conform_reset": (ctypes.c_int, [ctypes.c_void_p]),
    "fldr_conform_destroy": (None, [ctypes.c_void_p]),
}
EXPORTS = tuple(_SIGNATURES)
_API = fldr_rate.Binding("conform", LIB_PATH, CONFORM_VERSION, _SIGNATURES, (Config, StreamConfig), "ConformError")
ConformError, lib, _check = _API.Error, _API.lib, _API.check


# ---- host only --------------------------------------------------------------------------------------------------------------------------
def coefs_raw(src, dst, out):
    """The raw call (None = NULL; out: an int32 array of 7 or None); returns the code without raising."""
    return lib().fldr_conform_coefs(_ref(src), _ref(dst), out.ctypes.data if out is not None else None)


def coefs(src, dst):
    """fldr_conform_coefs -> [KYY, KYU, KYV, KUU, KUV, KVU, KVV] of the conversion from Format src to Format dst."""
    k = np.zeros(7, np.int32)
    _check(coefs_raw(src, dst, k), "fldr_conform_coefs")
    return [int(v) for v in k]


def view_raw(fr, fmt, x, y, out):
    """fldr_conform_view on Frame structs (None = NULL); returns the code without raising."""
    return lib().fldr_conform_view(_ref(fr), _ref(fmt), int(x), int(y), _ref(out))


def view(planes, fmt, x, y, size):
    """The window of `size` = (H, W) of a frame (a tuple of plane tensors or arrays) whose top-left luma sample is (x, y): a tuple of
    plane views at the addresses fldr_conform_view gives."""
    out = Frame()
    _check(view_raw(frame_struct(planes), fmt, x, y, out), "fldr_conform_view")
    got = []
    for p, (rows, cols) in enumerate(plane_shapes(fmt, size[0], size[1])):
        r0, c0 = (y, x) if p == 0 else (y // 2, (x // 2) * (2 if fmt.layout == 0 else 1))
        win = planes[p][r0:r0 + rows, c0:c0 + cols]
        ptr = win.data_ptr() if hasattr(win, "data_ptr") else win.ctypes.data
        assert ptr == out.plane[p] and out.pitch[p] == frame_struct(planes).pitch[p], "fldr_conform_view moved plane %d elsewhere" % p
        got.append(win)
    return tuple(got)


# ---- the kernel entry ----------------------------------------------------------------------------------------------------------------------
def config(in_size, in_format, out_size, out_format, at=(0, 0), dither=False):
    cfg = Config()
    (cfg.in_H, cfg.in_W), (cfg.out_H, cfg.out_W) = in_size, out_size
    cfg.in_format, cfg.out_format = in_format, out_format
    cfg.dst_x, cfg.dst_y, cfg.dither = int(at[0]), int(at[1]), int(dither)
    return cfg


def frame_raw(cfg, src, dst, stream_ptr):
    """fldr_conform_frame on a Config and Frame structs (None = NULL); returns the code without raising."""
    return lib().fldr_conform_frame(_ref(cfg), _ref(src), _ref(dst), stream_ptr)


def frame(src, in_format, dst, out_format, at=(0, 0), dither=False, stream=None):
    """fldr_conform_frame: src (device planes in in_format) -> dst (device planes in out_format, the canvas), the picture's top-left luma
    sample at `at` = (x, y).  The sizes are those of the luma planes.  Enqueues on torch's current stream."""
    cfg = config(tuple(src[0].shape), in_format, tuple(dst[0].shape), out_format, at, dither)
    _check(frame_raw(cfg, frame_struct(src), frame_struct(dst), _stream_ptr(dst[0].device, stream)), "fldr_conform_frame")
    return dst


# ---- the stream ------------------------------------------------------------------------------------------------------------------------
def stream_config(in_size, in_format, out_size, out_format, in_rate, out_rate, at=(0, 0), dither=False, scene=True, device=0, scene_params=None):
    cfg = StreamConfig()
    rate_config(in_size[0], in_size[1], in_format, in_rate, out_rate, scene, scene_params, device, into=cfg.rate)
    cfg.out_H, cfg.out_W, cfg.out_format = int(out_size[0]), int(out_size[1]), out_format
    cfg.dst_x, cfg.dst_y, cfg.dither = int(at[0]), int(at[1]), int(dither)
    return cfg


class Conformer(fldr_video.HostStream):
    """fldr_conform: host frames (tuples of numpy planes) of in_size in in_format pushed one by one at in_rate; each push returns the
    frames of out_size in out_format at out_rate that fall before the pushed frame, flush() the one that lands on the last frame.
    native_model may be None where the rates are equal: a pure converter."""

    _destroy = staticmethod(lambda h: lib().fldr_conform_destroy(h))

    def __init__(self, native_model, in_size, in_format, out_size, out_format, in_rate=25, out_rate=25, at=(0, 0), dither=False, scene=True,
                 scene_params=None, device=0):
        if native_model is not None:
            device = native_model.device.index or 0
        self.cfg = stream_config(in_size, in_format, out_size, out_format, in_rate, out_rate, at, dither, scene, device, scene_params)
        self._h = ctypes.c_void_p()
        self.model = native_model                                    # the stream uses the model: keep it alive
        _check(lib().fldr_conform_create(native_model._h if native_model is not None else None, ctypes.byref(self.cfg), ctypes.byref(self._h)),
               "fldr_conform_create")
        self.in_size, self.out_size, self.in_format, self.out_format = tuple(in_size), tuple(out_size), in_format, out_format
        self.max_out = lib().fldr_conform_max_out(self._h)
        self._stage(out_format, out_size[0], out_size[1], self.max_out)
        self.last_scene = None

    def push(self, frame):
        """-> the list of output frames due (tuples of numpy planes, fresh copies); self.last_scene: the pair's scene dict."""
        fr = frame_struct(frame)
        n = ctypes.c_int(-1)
        res = SceneResult()
        _check(lib().fldr_conform_push(self._h, ctypes.byref(fr), self._out_structs(), ctypes.byref(n), ctypes.byref(res)), "fldr_conform_push")
        self.last_scene = res.as_dict()
        return self._taken(n.value)

    def flush(self):
        n = ctypes.c_int(-1)
        _check(lib().fldr_conform_flush(self._h, self._out_structs(), ctypes.byref(n)), "fldr_conform_flush")
        return self._taken(n.value)

    def reset(self):
        _check(lib().fldr_conform_reset(self._h), "fldr_conform_reset")
