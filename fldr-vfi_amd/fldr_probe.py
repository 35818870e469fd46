"""ctypes binding of libfldr_probe.so (probe API: include/fldr_probe.h) — what a stream of 4:2:0 frames carries: progressive frames (with
or without repeats), film in interlaced video with its pulldown cadence, or true interlaced video with its field order.  One measure
kernel per frame (both anchors' comb counts, both fields' differences, the whole-frame motion and the field-order sums, per tile of
32 x 32 luma samples), a host classifier, and the stream that keeps a window of results.

    r = measure(cur, prev, next, Format("nv12"))                 # -> {"comb", "max_tile_comb", ..., "lap", "tff_sum", "bff_sum"}
    v = classify([r1, r2, ...])                                  # -> {"kind", "tff", "mixed", "cycle", "drop", ...}
    p = Probe(H, W, Format("i420"), window=32); p.push((y, u, v)); ...; p.verdict(); p.results()

Frames are fldr_video's: tuples of 2-D plane tensors (device) or numpy arrays (host).  measure enqueues on torch's current stream
(and synchronises to read the result back unless told not to).  No fallback: a missing library raises at load.
"""
import ctypes
import functools
import os

import fldr_rate
from fldr_rate import E_ARG, E_DEVICE, E_STATE, _ref  # noqa: F401  (this library's codes are the rate library's)
from fldr_video import Format, Frame, _stream_ptr, frame_struct

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfldr_probe.so")
PROBE_VERSION = 100               # include/fldr_probe.h: FLDR_PROBE_VERSION
C, P, N = 0, 1, 2
TILE = 32
TILE_COMB_MAX = 512
TILE_SAD_MAX = 130560
FRAME_TILE_SAD_MAX = 261120
COMB_THRESH_DEFAULT, COMB_TILE_DEFAULT, TILE_SAD_DEFAULT, FRAME_TILE_SAD_DEFAULT, MIN_MOVED_DEFAULT = 6, 32, 1024, 2048, 4
STATE_BYTES = 16384
MAX_CYCLE = 16
MIN_WINDOW, MAX_WINDOW = 3, 64
UNKNOWN, PROGRESSIVE, FILM, INTERLACED, MIXED = 0, 1, 2, 3, 4
FRAME_STILL, FRAME_PROG, FRAME_FILM, FRAME_VIDEO = 0, 1, 2, 3
RESULT_KEYS = ("comb", "max_tile_comb", "max_tile", "field_sad", "field_max_tile_sad", "field_max_tile", "field_moving_tiles",
               "frame_moving_tiles", "repeat", "lap", "tff_sum", "bff_sum")
VERDICT_KEYS = ("kind", "tff", "mixed", "cycle", "drop", "anchor", "irregular", "confirmed", "n_frames", "n_moved", "n_still", "n_prog",
                "n_film", "n_video", "votes_tff", "votes_bff")


class Params(ctypes.Structure):
    _fields_ = [("comb_thresh", ctypes.c_int32), ("comb_tile_min", ctypes.c_int32), ("tile_sad_min", ctypes.c_int32),
                ("frame_tile_sad_min", ctypes.c_int32), ("min_moved", ctypes.c_int32), ("max_outliers", ctypes.c_int32),
                ("anchor", ctypes.c_int32), ("reserved", ctypes.c_int32 * 5)]

    def __init__(self, comb_thresh=0, comb_tile_min=0, tile_sad_min=0, frame_tile_sad_min=0, min_moved=0, max_outliers=0, anchor=0):
        super().__init__(int(comb_thresh), int(comb_tile_min), int(tile_sad_min), int(frame_tile_sad_min), int(min_moved), int(max_outliers),
                         int(anchor))


def _plain(v):
    return [_plain(x) for x in v] if hasattr(v, "__len__") else int(v)


class Result(ctypes.Structure):
    _fields_ = [("comb", ctypes.c_uint64 * 3 * 2), ("max_tile_comb", ctypes.c_uint32 * 3 * 2), ("max_tile", ctypes.c_uint32 * 3 * 2),
                ("field_sad", ctypes.c_uint64 * 2), ("field_max_tile_sad", ctypes.c_uint32 * 2), ("field_max_tile", ctypes.c_uint32 * 2),
                ("field_moving_tiles", ctypes.c_uint32 * 2), ("frame_moving_tiles", ctypes.c_uint32), ("repeat", ctypes.c_uint32),
                ("lap", ctypes.c_uint64 * 2 * 3), ("tff_sum", ctypes.c_uint64), ("bff_sum", ctypes.c_uint64), ("reserved", ctypes.c_uint32 * 12)]

    def as_dict(self):
        return {k: _plain(getattr(self, k)) for k in RESULT_KEYS}

    @classmethod
    def from_dict(cls, d):
        r = cls()
        for k in RESULT_KEYS:
            v = d[k]
            if isinstance(v, (list, tuple)):
                for i, x in enumerate(v):
                    if isinstance(x, (list, tuple)):
                        for j, y in enumerate(x):
                            getattr(r, k)[i][j] = int(y)
                    else:
                        getattr(r, k)[i] = int(x)
            else:
                setattr(r, k, int(v))
        return r


class Verdict(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in VERDICT_KEYS] + [("reserved", ctypes.c_int32 * 8)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k in VERDICT_KEYS}


class ProbeConfig(ctypes.Structure):
    _fields_ = [("H", ctypes.c_int32), ("W", ctypes.c_int32), ("format", Format), ("device", ctypes.c_int32), ("window", ctypes.c_int32),
                ("params", Params), ("reserved", ctypes.c_int32 * 4)]


_FRAME_P = ctypes.POINTER(Frame)
_SIGNATURES = {
    "fldr_probe_version": (ctypes.c_int, []),
    "fldr_probe_error_string": (ctypes.c_char_p, [ctypes.c_int]),
    "fldr_probe_sizeof": (ctypes.c_int, [ctypes.c_int]),
    "fldr_probe_measure": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(Format), _FRAME_P, _FRAME_P, _FRAME_P,
                                          ctypes.POINTER(Params), ctypes.c_void_p, ctypes.c_void_p]),
    "fldr_probe_frame_class": (ctypes.c_int, [ctypes.POINTER(Result), ctypes.POINTER(Params)]),
    "fldr_probe_classify": (ctypes.c_int, [ctypes.POINTER(Result), ctypes.c_int, ctypes.POINTER(Params), ctypes.POINTER(Verdict)]),
    "fldr_probe_create": (ctypes.c_int, [ctypes.POINTER(ProbeConfig), ctypes.POINTER(ctypes.c_void_p)]),
    "fldr_probe_push": (ctypes.c_int, [ctypes.c_void_p, _FRAME_P]),
    "fldr_probe_verdict_get": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Verdict)]),
    "fldr_probe_result_get": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Result), ctypes.POINTER(ctypes.c_int64)]),
    "fldr_probe_reset": (ctypes.c_int, [ctypes.c_void_p]),
    "fldr_probe_destroy": (None, [ctypes.c_void_p]),
}
EXPORTS = tuple(_SIGNATURES)
_API = fldr_rate.Binding("probe", LIB_PATH, PROBE_VERSION, _SIGNATURES, (Params, Result, Verdict, ProbeConfig), "ProbeError")
ProbeError, lib, _check = _API.Error, _API.lib, _API.check


# ---- the measure -----------------------------------------------------------------------------------------------------------------------
measure_state = functools.partial(fldr_rate.state_tensor, STATE_BYTES)             # (device) -> FLDR_PROBE_STATE_BYTES of device memory
read_result = functools.partial(fldr_rate.read_struct, Result)                     # (state) -> the fldr_probe_result at its start, a dict


def measure_raw(H, W, fmt, cur, prev, nxt, params, state_ptr, stream_ptr):
    """The raw call on Frame structs (None = NULL); returns the code without raising (tests of the error contract)."""
    return lib().fldr_probe_measure(int(H), int(W), _ref(fmt), _ref(cur), _ref(prev), _ref(nxt), _ref(params), state_ptr, stream_ptr)


def measure(cur, prev, nxt, fmt, params=None, state=None, stream=None, read=True):
    """fldr_probe_measure of cur against prev and nxt (each a tuple of device plane tensors in `fmt`; prev / nxt may be None); params: a
    Params, None = the defaults; state: a measure_state tensor (allocated otherwise).  Enqueues on torch's current stream; -> the result
    dict after a synchronising read-back, or the state tensor with read=False."""
    H, W = cur[0].shape
    device = cur[0].device
    if state is None:
        state = measure_state(device)
    fr = [frame_struct(f) if f is not None else None for f in (cur, prev, nxt)]
    _check(measure_raw(H, W, fmt, fr[0], fr[1], fr[2], params, ctypes.c_void_p(state.data_ptr()), _stream_ptr(device, stream)), "fldr_probe_measure")
    return read_result(state) if read else state


# ---- the classifier (host only) ----------------------------------------------------------------------------------------------------------
def _results_array(results):
    arr = (Result * max(len(results), 1))()
    for i, r in enumerate(results):
        arr[i] = r if isinstance(r, Result) else Result.from_dict(r)
    return arr


def frame_class(result, params=None):
    """fldr_probe_frame_class of one result (a dict or a Result) -> FRAME_STILL / _PROG / _FILM / _VIDEO."""
    r = result if isinstance(result, Result) else Result.from_dict(result)
    c = lib().fldr_probe_frame_class(ctypes.byref(r), _ref(params))
    if c < 0:
        raise ProbeError("fldr_probe_frame_class", c)
    return c


def classify_raw(results, M, params, verdict):
    """The raw call (results: a ctypes array or None); returns the code without raising."""
    return lib().fldr_probe_classify(results, int(M), _ref(params), _ref(verdict))


def classify(results, params=None):
    """fldr_probe_classify of a list of results (dicts or Results) of consecutive frames -> the verdict dict."""
    v = Verdict()
    _check(classify_raw(_results_array(results) if len(results) else None, len(results), params, v), "fldr_probe_classify")
    return v.as_dict()


# ---- the stream ------------------------------------------------------------------------------------------------------------------------
def make_config(H, W, fmt, window=32, device=0, params=None):
    cfg = ProbeConfig()
    cfg.H, cfg.W, cfg.format, cfg.device, cfg.window = int(H), int(W), fmt, int(device), int(window)
    if params is not None:
        cfg.params = params
    return cfg


class Probe:
    """fldr_probe: host frames (tuples of numpy planes) pushed one by one; verdict() classifies the last `window` measured frames,
    results() returns them, oldest first, with the stream number of each."""

    def __init__(self, H, W, fmt=None, window=32, device=0, params=None):
        fmt = fmt or Format()
        cfg = make_config(H, W, fmt, window, device, params)
        self._h = ctypes.c_void_p()
        _check(lib().fldr_probe_create(ctypes.byref(cfg), ctypes.byref(self._h)), "fldr_probe_create")
        self.H, self.W, self.format, self.window = int(H), int(W), fmt, int(window)

    def push(self, frame):
        fr = frame_struct(frame)
        _check(lib().fldr_probe_push(self._h, ctypes.byref(fr)), "fldr_probe_push")

    def verdict(self):
        v = Verdict()
        _check(lib().fldr_probe_verdict_get(self._h, ctypes.byref(v)), "fldr_probe_verdict_get")
        return v.as_dict()

    def results(self):
        """-> [(stream frame number, result dict)] of the ring, oldest first."""
        out = []
        for i in range(self.verdict()["n_frames"]):
            r, n = Result(), ctypes.c_int64(-1)
            _check(lib().fldr_probe_result_get(self._h, i, ctypes.byref(r), ctypes.byref(n)), "fldr_probe_result_get")
            out.append((n.value, r.as_dict()))
        return out

    def reset(self):
        _check(lib().fldr_probe_reset(self._h), "fldr_probe_reset")

    def close(self):
        if self._h:
            lib().fldr_probe_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
