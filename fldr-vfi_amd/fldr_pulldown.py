"""ctypes binding of libfldr_pulldown.so (pulldown API: include/fldr_pulldown.h) — inverse telecine of film in interlaced video: the
field-matching measure per tile of 32 x 32 luma samples, the assembly of the matched frame, and the stream that matches every frame,
drops the duplicates of every cycle and converts the survivors with fldr_rate.

    r = measure(cur, prev, next, Format("nv12"), anchor=0)       # -> {"match", "combed", "comb", "max_tile_comb", "max_tile", "dup_*"}
    out = assemble(cur, prev, next, Format("nv12"), anchor=0, match=r["match"], combed=r["combed"], post=POST_AVERAGE)
    c = Pulldown(native_model, H, W, Format("i420"), in_rate=(30000, 1001), out_rate=(60000, 1001), cycle=5, drop=1)   # 3:2 in 60i -> 60p
    outs = c.push((y, u, v)); ...; outs = c.flush()              # c.last_report: the cycle a call completed, or None

inner_rate(in_rate, cycle, drop) is the pure-Python statement of the rate the survivors are converted from.  Frames are fldr_video's:
tuples of 2-D plane tensors (device) or numpy arrays (host).  measure and assemble enqueue on torch's current stream (measure
synchronises to read the result back unless told not to).  No fallback: a missing library raises at load.
"""
import ctypes
import functools
import os

import fldr_rate
from fldr_rate import E_ARG, E_DEVICE, E_RATIO, E_STATE, RateConfig, _ref, inner_rate, rate_config  # noqa: F401  (this library's codes are the rate library's)
from fldr_video import Format, Frame, _stream_ptr, frame_struct

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfldr_pulldown.so")
PULLDOWN_VERSION = 100            # include/fldr_pulldown.h: FLDR_PULLDOWN_VERSION
C, P, N = 0, 1, 2
POST_KEEP, POST_AVERAGE = 0, 1
TILE = 32
TILE_COMB_MAX = 512
TILE_SAD_MAX = 130560
COMB_THRESH_DEFAULT, COMB_TILE_DEFAULT, TILE_SAD_DEFAULT = 6, 32, 1024
STATE_BYTES = 8192
MAX_CYCLE = 16
RESULT_KEYS = ("match", "combed", "comb", "max_tile_comb", "max_tile", "dup_sad", "dup_max_tile_sad", "dup_max_tile", "dup_moving_tiles")


class Params(ctypes.Structure):
    _fields_ = [("comb_thresh", ctypes.c_int32), ("comb_tile_min", ctypes.c_int32), ("tile_sad_min", ctypes.c_int32),
                ("allowed", ctypes.c_int32), ("reserved", ctypes.c_int32 * 4)]

    def __init__(self, comb_thresh=0, comb_tile_min=0, tile_sad_min=0, allowed=0):
        super().__init__(int(comb_thresh), int(comb_tile_min), int(tile_sad_min), int(allowed))


class Result(ctypes.Structure):
    _fields_ = [("match", ctypes.c_int32), ("combed", ctypes.c_uint32), ("comb", ctypes.c_uint64 * 3), ("max_tile_comb", ctypes.c_uint32 * 3),
                ("max_tile", ctypes.c_uint32 * 3), ("dup_sad", ctypes.c_uint64), ("dup_max_tile_sad", ctypes.c_uint32),
                ("dup_max_tile", ctypes.c_uint32), ("dup_moving_tiles", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 5)]

    def as_dict(self):
        return {k: [int(v) for v in getattr(self, k)] if k in ("comb", "max_tile_comb", "max_tile") else int(getattr(self, k)) for k in RESULT_KEYS}


class PulldownConfig(ctypes.Structure):
    _fields_ = [("rate", RateConfig), ("cycle", ctypes.c_int32), ("drop", ctypes.c_int32), ("anchor", ctypes.c_int32), ("post", ctypes.c_int32),
                ("params", Params), ("reserved", ctypes.c_int32 * 4)]


class Report(ctypes.Structure):
    _fields_ = [("first_frame", ctypes.c_int64), ("n_frames", ctypes.c_uint32), ("dropped_mask", ctypes.c_uint32), ("combed_mask", ctypes.c_uint32),
                ("moving_dropped", ctypes.c_uint32), ("still_kept", ctypes.c_uint32), ("cut_mask", ctypes.c_uint32),
                ("match", ctypes.c_int32 * MAX_CYCLE), ("reserved", ctypes.c_uint32 * 2), ("measure", Result * MAX_CYCLE)]

    def as_dict(self):
        n = int(self.n_frames)
        return {"first_frame": int(self.first_frame), "n_frames": n, "dropped_mask": int(self.dropped_mask), "combed_mask": int(self.combed_mask),
                "moving_dropped": int(self.moving_dropped), "still_kept": int(self.still_kept), "cut_mask": int(self.cut_mask),
                "match": [int(self.match[k]) for k in range(n)], "measure": [self.measure[k].as_dict() for k in range(n)]}


_FRAME_P = ctypes.POINTER(Frame)
_SIGNATURES = {
    "fldr_pulldown_version": (ctypes.c_int, []),
    "fldr_pulldown_error_string": (ctypes.c_char_p, [ctypes.c_int]),
    "fldr_pulldown_sizeof": (ctypes.c_int, [ctypes.c_int]),
    "fldr_pulldown_measure": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(Format), _FRAME_P, _FRAME_P, _FRAME_P, ctypes.c_int,
                                             ctypes.POINTER(Params), ctypes.c_void_p, ctypes.c_void_p]),
    "fldr_pulldown_assemble": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(Format), _FRAME_P, _FRAME_P, _FRAME_P, _FRAME_P,
                                              ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "fldr_pulldown_inner_rate": (ctypes.c_int, [ctypes.POINTER(PulldownConfig), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
    "fldr_pulldown_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(PulldownConfig), ctypes.POINTER(ctypes.c_void_p)]),
    "fldr_pulldown_max_out": (ctypes.c_int, [ctypes.c_void_p]),
    "fldr_pulldown_push": (ctypes.c_int, [ctypes.c_void_p, _FRAME_P, _FRAME_P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(Report)]),
    "fldr_pulldown_flush": (ctypes.c_int, [ctypes.c_void_p, _FRAME_P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(Report)]),
    "fldr_pulldown_reset": (ctypes.c_int, [ctypes.c_void_p]),
    "fldr_pulldown_destroy": (None, [ctypes.c_void_p]),
}
EXPORTS = tuple(_SIGNATURES)
_API = fldr_rate.Binding("pulldown", LIB_PATH, PULLDOWN_VERSION, _SIGNATURES, (Params, Result, PulldownConfig, Report), "PulldownError")
PulldownError, lib, _check = _API.Error, _API.lib, _API.check
inner_rate_raw = functools.partial(fldr_rate.inner_rate_raw, _API, PulldownConfig)


# ---- the measure -----------------------------------------------------------------------------------------------------------------------
measure_state = functools.partial(fldr_rate.state_tensor, STATE_BYTES)             # (device) -> FLDR_PULLDOWN_STATE_BYTES of device memory
read_result = functools.partial(fldr_rate.read_struct, Result)                     # (state) -> the fldr_pulldown_result at its start, a dict


def measure_raw(H, W, fmt, cur, prev, nxt, anchor, params, state_ptr, stream_ptr):
    """The raw call on Frame structs (None = NULL); returns the code without raising (tests of the error contract)."""
    return lib().fldr_pulldown_measure(int(H), int(W), _ref(fmt), _ref(cur), _ref(prev), _ref(nxt), int(anchor), _ref(params), state_ptr, stream_ptr)


def measure(cur, prev, nxt, fmt, anchor=0, params=None, state=None, stream=None, read=True):
    """fldr_pulldown_measure of cur against prev and nxt (each a tuple of device plane tensors in `fmt`, or None where `allowed` does not
    need it); params: a Params, None = the defaults; state: a measure_state tensor (allocated otherwise).  Enqueues on torch's current
    stream; -> the result dict after a synchronising read-back, or the state tensor with read=False."""
    H, W = cur[0].shape
    device = cur[0].device
    if state is None:
        state = measure_state(device)
    fr = [frame_struct(f) if f is not None else None for f in (cur, prev, nxt)]
    _check(measure_raw(H, W, fmt, fr[0], fr[1], fr[2], anchor, params, ctypes.c_void_p(state.data_ptr()), _stream_ptr(device, stream)),
           "fldr_pulldown_measure")
    return read_result(state) if read else state


# ---- the assembly ----------------------------------------------------------------------------------------------------------------------
def assemble_raw(H, W, fmt, cur, prev, nxt, out, anchor, match, combed, decision_ptr, post, stream_ptr):
    """The raw call on Frame structs (None = NULL); returns the code without raising."""
    return lib().fldr_pulldown_assemble(int(H), int(W), _ref(fmt), _ref(cur), _ref(prev), _ref(nxt), _ref(out), int(anchor), int(match), int(combed),
                                        decision_ptr, int(post), stream_ptr)


def assemble(cur, prev, nxt, out, fmt, anchor=0, match=-1, combed=0, decision=None, post=POST_KEEP, stream=None):
    """fldr_pulldown_assemble into `out` (a tuple of device plane tensors).  match 0 .. 2 with `combed` given, or -1 with `decision` a
    measure_state tensor (or any device tensor that begins with the two words).  Enqueues on torch's current stream."""
    H, W = cur[0].shape
    device = cur[0].device
    fr = [frame_struct(f) if f is not None else None for f in (cur, prev, nxt, out)]
    dp = ctypes.c_void_p(decision.data_ptr()) if decision is not None else None
    _check(assemble_raw(H, W, fmt, fr[0], fr[1], fr[2], fr[3], anchor, match, combed, dp, post, _stream_ptr(device, stream)), "fldr_pulldown_assemble")
    return out


# ---- the stream ------------------------------------------------------------------------------------------------------------------------
def make_config(H, W, fmt, in_rate, out_rate, cycle, drop, anchor=0, post=POST_KEEP, scene=True, device=0, scene_params=None, params=None):
    cfg = PulldownConfig()
    rate_config(H, W, fmt, in_rate, out_rate, scene, scene_params, device, into=cfg.rate)
    cfg.cycle, cfg.drop, cfg.anchor, cfg.post = int(cycle), int(drop), int(anchor), int(post)
    if params is not None:
        cfg.params = params
    return cfg


class Pulldown(fldr_rate.CycleStream):
    """fldr_pulldown: woven container frames (tuples of numpy planes) pushed one by one at in_rate, of every `cycle` of which, once
    matched, `drop` are duplicates; push, flush, reset and last_report are fldr_rate.CycleStream's."""
    _api, _Report = _API, Report

    def __init__(self, native_model, H, W, fmt=None, in_rate=(30000, 1001), out_rate=(60000, 1001), cycle=5, drop=1, anchor=0, post=POST_KEEP,
                 scene=True, scene_params=None, params=None):
        fmt = fmt or Format()
        cfg = make_config(H, W, fmt, in_rate, out_rate, cycle, drop, anchor, post, scene, native_model.device.index or 0, scene_params, params)
        self._create(native_model, cfg, H, W, fmt, cycle, drop)
