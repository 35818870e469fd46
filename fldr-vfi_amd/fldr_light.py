"""ctypes binding of libfldr_light.so (linear-light API: include/fldr_light.h) — the shutter integration of fldr_shutter done on light
instead of on code values: every sample through a transfer curve (a table) before it is summed, and back through it afterwards.

    curve = Curve("gamma24", 8)                                  # or "pq", "hlg", or Curve(table=[...]) — the one call that allocates
    acc = accumulate(curve, frames, weights, Format("nv12"))     # device frames -> three uint32 planes (a uint8 tensor)
    out = resolve(curve, acc, sum(weights), H, W, Format("nv12"))
    out = mix(curve, frames, weights, Format("nv12"))            # the same bytes
    nl = NativeLight(fldr_model.NativeModel.from_npz(fldr_harness.DEFAULT_WEIGHTS))
    out = nl.forward(curve, (f0, f1), t=[0.25, 0.5, 0.75], weights=(1, 0, [1, 1, 1]), fmt=Format("nv12"))
    c = Converter(native_model, curve, H, W, Format("i420"), in_rate=120, out_rate=24, shutter=(1, 2), sub=1)
    outs = c.push((y, u, v)); ...; outs = c.flush()              # as fldr_shutter.Converter: c.last_info, c.last_scene

table(transfer, depth) is the host-only fldr_light_table: the words a built-in curve holds, what the tests feed their oracle.  Windows
and pushes are fldr_shutter's (fldr_shutter.schedule), and so is the code under the three kernel calls, the forward and the converter
(fldr_shutter._accumulate / _resolve / _mix, _NativeForward, _WindowStream): this module adds the curve and scratch.  Every kernel call and
forward enqueues on torch's current stream and returns without synchronising.  No fallback: a missing library raises at load.
"""
import ctypes
import os

import numpy as np
import torch

import fldr_model
import fldr_shutter
from fldr_rate import SceneResult
from fldr_shutter import Info, ShutterConfig
from fldr_video import Format, Frame, IO, _stream_ptr  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfldr_light.so")
LIGHT_VERSION = 100               # include/fldr_light.h: FLDR_LIGHT_VERSION
E_ARG, E_CURVE, E_TABLE, E_ACC, E_WEIGHT, E_RATIO, E_DEVICE, E_FORMAT = -400, -401, -402, -403, -404, -405, -406, -407
MAX_TOTAL, SCALE = 255, (1 << 24) - 1
TRANSFERS = {"gamma24": 0, "pq": 1, "hlg": 2, "table": 3}


class LightConfig(ctypes.Structure):
    _fields_ = [("shutter", ShutterConfig), ("curve", ctypes.c_void_p)]


_I32P = ctypes.POINTER(ctypes.c_int32)
_U32P = ctypes.POINTER(ctypes.c_uint32)
_KERNEL_HEAD = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(Format), ctypes.c_void_p]
_SIGNATURES = {
    "fldr_light_version": (ctypes.c_int, []),
    "fldr_light_error_string": (ctypes.c_char_p, [ctypes.c_int]),
    "fldr_light_sizeof": (ctypes.c_int, [ctypes.c_int]),
    "fldr_light_table": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _U32P]),
    "fldr_light_curve_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _U32P, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    "fldr_light_curve_destroy": (None, [ctypes.c_void_p]),
    "fldr_light_acc_bytes": (ctypes.c_int64, [ctypes.c_int, ctypes.c_int]),
    "fldr_light_scratch_bytes": (ctypes.c_int64, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(Format)]),
    "fldr_light_accumulate": (ctypes.c_int, _KERNEL_HEAD + [ctypes.POINTER(Frame), _I32P, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                            ctypes.c_void_p]),
    "fldr_light_resolve": (ctypes.c_int, _KERNEL_HEAD + [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Frame), ctypes.c_void_p, ctypes.c_void_p]),
    "fldr_light_mix": (ctypes.c_int, _KERNEL_HEAD + [ctypes.POINTER(Frame), _I32P, ctypes.c_int, ctypes.POINTER(Frame), ctypes.c_void_p, ctypes.c_void_p]),
    "fldr_light_workspace_bytes": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "fldr_light_forward": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(IO), ctypes.c_void_p, ctypes.c_int, ctypes.c_int, _I32P, ctypes.c_void_p,
                                          ctypes.c_int64, ctypes.c_void_p]),
    "fldr_light_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(LightConfig), ctypes.POINTER(ctypes.c_void_p)]),
    "fldr_light_max_out": (ctypes.c_int, [ctypes.c_void_p]),
    "fldr_light_push": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Frame), ctypes.POINTER(Frame), ctypes.POINTER(Info), ctypes.POINTER(ctypes.c_int),
                                       ctypes.POINTER(SceneResult)]),
    "fldr_light_flush": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Frame), ctypes.POINTER(Info), ctypes.POINTER(ctypes.c_int)]),
    "fldr_light_reset": (ctypes.c_int, [ctypes.c_void_p]),
    "fldr_light_destroy": (None, [ctypes.c_void_p]),
}
EXPORTS = tuple(_SIGNATURES)
_lib = None


class LightError(RuntimeError):
    def __init__(self, what, code):
        super().__init__("%s failed: %s (code %d)" % (what, lib().fldr_light_error_string(code).decode(), code))
        self.code = code


def lib():
    """The loaded libfldr_light.so, checked against this binding (struct size, header version); raises when it has not been built."""
    global _lib
    if _lib is None:
        fldr_shutter.lib()
        _lib = fldr_model.load_library(LIB_PATH, _SIGNATURES, (LightConfig,), "fldr_light", LIGHT_VERSION)
    return _lib


_API = fldr_shutter._Api(lib, "fldr_light", LightError)


# ---- the curve --------------------------------------------------------------------------------------------------------------------------
def table(transfer, depth=8):
    """fldr_light_table: the built-in table of "gamma24" / "pq" / "hlg" at depth 8 or 10 -> uint32 numpy [2^depth].  Host only."""
    lin = np.zeros(1 << (depth or 8), np.uint32)
    _API.call("table", TRANSFERS[transfer] if isinstance(transfer, str) else int(transfer), int(depth), lin.ctypes.data_as(_U32P))
    return lin


class Curve:
    """A fldr_light_curve on a device: a built-in transfer, or a caller's table (uint32, strictly increasing, last entry <= SCALE).
    self.lin: the table the curve holds (numpy uint32)."""

    def __init__(self, transfer="gamma24", depth=8, table_=None, device=0):
        if table_ is not None:
            transfer = "table"
            self.lin = np.ascontiguousarray(table_, dtype=np.uint32)
            ptr = self.lin.ctypes.data_as(_U32P)
        else:
            self.lin = table(transfer, depth)
            ptr = None
        self.depth = depth or 8
        self._h = ctypes.c_void_p()
        _API.call("curve_create", TRANSFERS[transfer], int(depth), ptr, int(device), ctypes.byref(self._h))

    def close(self):
        if self._h is not None and self._h.value:
            lib().fldr_light_curve_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- the integration kernels --------------------------------------------------------------------------------------------------------------
def acc_bytes(H, W):
    return _API.size("acc_bytes", int(H), int(W))


def scratch_bytes(H, W, fmt):
    return _API.size("scratch_bytes", int(H), int(W), ctypes.byref(fmt))


def _scratch(scratch, H, W, fmt, device):
    return scratch if scratch is not None else torch.empty(scratch_bytes(H, W, fmt), dtype=torch.uint8, device=device)


# The three calls are fldr_shutter's with the curve behind fmt and scratch before the stream.
def accumulate(curve, frames, weights, fmt, acc=None, first=True, scratch=None, stream=None):
    """fldr_light_accumulate of device frames; acc: a uint8 device tensor of acc_bytes (allocated otherwise) -> acc."""
    H, W = frames[0][0].shape
    scratch = _scratch(scratch, H, W, fmt, frames[0][0].device)
    return fldr_shutter._accumulate(_API, (curve._h,), (ctypes.c_void_p(scratch.data_ptr()),), frames, weights, fmt, acc, acc_bytes, first, stream)


def resolve(curve, acc, total, H, W, fmt, out=None, scratch=None, stream=None):
    """fldr_light_resolve -> one device frame (`out` when given; allocated packed otherwise)."""
    scratch = _scratch(scratch, H, W, fmt, acc.device)
    return fldr_shutter._resolve(_API, (curve._h,), (ctypes.c_void_p(scratch.data_ptr()),), acc, total, H, W, fmt, out, stream)


def mix(curve, frames, weights, fmt, out=None, scratch=None, stream=None):
    """fldr_light_mix of device frames -> one device frame."""
    H, W = frames[0][0].shape
    scratch = _scratch(scratch, H, W, fmt, frames[0][0].device)
    return fldr_shutter._mix(_API, (curve._h,), (ctypes.c_void_p(scratch.data_ptr()),), frames, weights, fmt, out, stream)


class NativeLight(fldr_shutter._NativeForward):
    """fldr_light_forward on a fldr_model.NativeModel: NativeVideo's forward, then one linear-light mix of its planar frames."""

    _api = _API

    def forward_io(self, io, curve, w0, w1, w, ws, stream=None):
        """The raw call; returns the code without raising."""
        return self._forward_io(io, (curve._h if curve is not None else None,), w0, w1, w, ws, stream)

    def forward(self, curve, frames, t, weights, fmt=None, out=None, ws=None, stream=None):
        """frames: (I0, I1) in fmt; t: the n_t sub-frame times; weights: (w0, w1, [w of each sub-frame]).  -> the one output frame."""
        return self._forward((curve._h if curve is not None else None,), frames, t, weights, fmt, out, ws, stream)


class Converter(fldr_shutter._WindowStream):
    """fldr_light: fldr_shutter.Converter with every output the linear-light mean of its points."""

    _api = _API

    def __init__(self, native_model, curve, H, W, fmt=None, in_rate=120, out_rate=24, shutter=(1, 2), sub=1, scene=True, params=None):
        fmt = fmt or Format()
        cfg = LightConfig()
        cfg.shutter = fldr_shutter.config(in_rate, out_rate, shutter, sub, H, W, fmt, native_model.device.index or 0, scene, params)
        cfg.curve = curve._h
        self.curve = curve                                           # the converter uses the curve as well as the model: keep it alive
        self._open(native_model, cfg, H, W, fmt)
