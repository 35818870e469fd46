"""ctypes binding of libfldr_cadence.so (cadence API: include/fldr_cadence.h) — the repeat measure per tile of 32 x 32 luma samples, and
the stream that drops the repeated frames of a container stream before rate conversion, on top of fldr_rate.

    m = repeat_measure((f0, f1), Format("nv12"))               # -> {"sad", "max_tile_sad", "max_tile", "moving_tiles", "repeat"}
    c = Cadence(native_model, H, W, Format("i420"), in_rate=60, out_rate=120, cycle=5, drop=3)   # 3:2 film in 60p -> 120
    outs = c.push((y, u, v)); ...; outs = c.flush()           # c.last_report: the cycle a call completed, or None

inner_rate(in_rate, cycle, drop) is the pure-Python statement of the rate the survivors are converted from.  Frames are fldr_video's:
tuples of 2-D plane tensors (device) or numpy arrays (host).  repeat_measure enqueues on torch's current stream (and synchronises to
read the result back unless told not to).  No fallback: a missing library raises at load.
"""
import ctypes
import functools
import os

import fldr_rate
from fldr_rate import RateConfig, inner_rate, rate_config  # noqa: F401  (inner_rate: the pure-Python statement of fldr_cadence_inner_rate)
from fldr_video import Format, Frame, _stream_ptr, frame_struct

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfldr_cadence.so")
CADENCE_VERSION = 100             # include/fldr_cadence.h: FLDR_CADENCE_VERSION
E_ARG, E_STATE, E_DEVICE = -600, -601, -602
TILE = 32
TILE_SAD_MAX = 261120
TILE_SAD_DEFAULT = 2048
REPEAT_STATE_BYTES = 4096
MAX_CYCLE = 16
RESULT_KEYS = ("sad", "max_tile_sad", "max_tile", "moving_tiles", "repeat")


class RepeatParams(ctypes.Structure):
    _fields_ = [("tile_sad_min", ctypes.c_int32), ("reserved", ctypes.c_int32 * 3)]

    def __init__(self, tile_sad_min=0):
        super().__init__(int(tile_sad_min))


class RepeatResult(ctypes.Structure):
    _fields_ = [("sad", ctypes.c_uint64), ("max_tile_sad", ctypes.c_uint32), ("max_tile", ctypes.c_uint32), ("moving_tiles", ctypes.c_uint32),
                ("repeat", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 2)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k in RESULT_KEYS}


class CadenceConfig(ctypes.Structure):
    _fields_ = [("rate", RateConfig), ("cycle", ctypes.c_int32), ("drop", ctypes.c_int32), ("repeat", RepeatParams),
                ("reserved", ctypes.c_int32 * 2)]


class Report(ctypes.Structure):
    _fields_ = [("first_frame", ctypes.c_int64), ("n_frames", ctypes.c_uint32), ("dropped_mask", ctypes.c_uint32),
                ("moving_dropped", ctypes.c_uint32), ("still_kept", ctypes.c_uint32), ("cut_mask", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32), ("measure", RepeatResult * MAX_CYCLE)]

    def as_dict(self):
        n = int(self.n_frames)
        return {"first_frame": int(self.first_frame), "n_frames": n, "dropped_mask": int(self.dropped_mask),
                "moving_dropped": int(self.moving_dropped), "still_kept": int(self.still_kept), "cut_mask": int(self.cut_mask),
                "measure": [self.measure[k].as_dict() for k in range(n)]}


_SIGNATURES = {
    "fldr_cadence_version": (ctypes.c_int, []),
    "fldr_cadence_error_string": (ctypes.c_char_p, [ctypes.c_int]),
    "fldr_cadence_sizeof": (ctypes.c_int, [ctypes.c_int]),
    "fldr_repeat_measure": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(Format), ctypes.POINTER(Frame), ctypes.POINTER(RepeatParams),
                                           ctypes.c_void_p, ctypes.c_void_p]),
    "fldr_cadence_inner_rate": (ctypes.c_int, [ctypes.POINTER(CadenceConfig), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
    "fldr_cadence_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(CadenceConfig), ctypes.POINTER(ctypes.c_void_p)]),
    "fldr_cadence_max_out": (ctypes.c_int, [ctypes.c_void_p]),
    "fldr_cadence_push": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Frame), ctypes.POINTER(Frame), ctypes.POINTER(ctypes.c_int),
                                         ctypes.POINTER(Report)]),
    "fldr_cadence_flush": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Frame), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(Report)]),
    "fldr_cadence_reset": (ctypes.c_int, [ctypes.c_void_p]),
    "fldr_cadence_destroy": (None, [ctypes.c_void_p]),
}
EXPORTS = tuple(_SIGNATURES)
_API = fldr_rate.Binding("cadence", LIB_PATH, CADENCE_VERSION, _SIGNATURES, (RepeatParams, RepeatResult, CadenceConfig, Report), "CadenceError")
CadenceError, lib, _check = _API.Error, _API.lib, _API.check
inner_rate_raw = functools.partial(fldr_rate.inner_rate_raw, _API, CadenceConfig)


# ---- the repeat measure --------------------------------------------------------------------------------------------------------------
repeat_state = functools.partial(fldr_rate.state_tensor, REPEAT_STATE_BYTES)      # (device) -> FLDR_REPEAT_STATE_BYTES of device memory
read_result = functools.partial(fldr_rate.read_struct, RepeatResult)               # (state) -> the fldr_repeat_result at its start, a dict


def repeat_measure_raw(H, W, fmt, frames, params, state_ptr, stream_ptr):
    """The raw call; returns the code without raising (tests of the error contract)."""
    arr = (Frame * 2)(*frames) if frames is not None else None
    return lib().fldr_repeat_measure(int(H), int(W), ctypes.byref(fmt) if fmt is not None else None, arr,
                                     ctypes.byref(params) if params is not None else None, state_ptr, stream_ptr)


def repeat_measure(frames, fmt, params=None, state=None, stream=None, read=True):
    """fldr_repeat_measure of frames (I0, I1), each a tuple of device plane tensors in `fmt` (pitches from their strides); params: a
    RepeatParams or tile_sad_min, None = the default; state: a repeat_state tensor (allocated otherwise).  Enqueues on torch's current
    stream; -> the result dict after a synchronising read-back, or the state tensor with read=False."""
    H, W = frames[0][0].shape
    device = frames[0][0].device
    if params is not None and not isinstance(params, RepeatParams):
        params = RepeatParams(params)
    if state is None:
        state = repeat_state(device)
    _check(repeat_measure_raw(H, W, fmt, [frame_struct(f) for f in frames], params, ctypes.c_void_p(state.data_ptr()), _stream_ptr(device, stream)),
           "fldr_repeat_measure")
    return read_result(state) if read else state


# ---- the stream ------------------------------------------------------------------------------------------------------------------------
def make_config(H, W, fmt, in_rate, out_rate, cycle, drop, scene=True, device=0, scene_params=None, tile_sad_min=0):
    cfg = CadenceConfig()
    rate_config(H, W, fmt, in_rate, out_rate, scene, scene_params, device, into=cfg.rate)
    cfg.cycle, cfg.drop = int(cycle), int(drop)
    cfg.repeat = tile_sad_min if isinstance(tile_sad_min, RepeatParams) else RepeatParams(tile_sad_min)
    return cfg


class Cadence(fldr_rate.CycleStream):
    """fldr_cadence: container frames (tuples of numpy planes) pushed one by one at in_rate, of every `cycle` of which `drop` are
    repeats; push, flush, reset and last_report are fldr_rate.CycleStream's."""
    _api, _Report = _API, Report

    def __init__(self, native_model, H, W, fmt=None, in_rate=60, out_rate=120, cycle=5, drop=3, scene=True, params=None, tile_sad_min=0):
        fmt = fmt or Format()
        cfg = make_config(H, W, fmt, in_rate, out_rate, cycle, drop, scene, native_model.device.index or 0, params, tile_sad_min)
        self._create(native_model, cfg, H, W, fmt, cycle, drop)
