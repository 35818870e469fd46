"""ctypes binding of libfldr_pipe.so (pipe API: include/fldr_pipe.h) — fldr_rate's converter with several pushed frames in flight.

    p = Pipe(native_model, H, W, Format("nv12"), in_rate=24, out_rate=60, depth=3)
    p.submit((y, uv))                                  # copies the planes into pinned memory, enqueues, returns
    outs, scene = p.receive()                          # waits for the OLDEST job: what Converter.push returned for that frame
    for plane, src in zip(p.input_planes(), frame): plane[...] = src      # or fill the pinned frame in place ...
    p.submit()                                         # ... and submit it without a copy
    views, scene = p.receive_view()                    # numpy views of pinned memory, valid until the next receive / reset / close
    p.flush(); outs, _ = p.receive()                   # the end-of-stream job

submit raises PipeFull with `depth` jobs outstanding, receive raises PipeEmpty with none (both PipeError, code E_FULL / E_EMPTY).
The k-th job received is the k-th Converter.push / flush of the same stream, byte for byte.  No fallback: a missing library raises at
load."""
import ctypes
import os

import numpy as np

import fldr_model
import fldr_rate
from fldr_rate import RateConfig, SceneResult, rate_config
from fldr_video import Format, Frame, frame_struct, plane_dtype, plane_shapes

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfldr_pipe.so")
PIPE_VERSION = 100                # include/fldr_pipe.h: FLDR_PIPE_VERSION
E_ARG, E_FULL, E_EMPTY, E_DEVICE = -500, -501, -502, -503
MAX_DEPTH = 8


class PipeConfig(ctypes.Structure):
    _fields_ = [("rate", RateConfig), ("depth", ctypes.c_int32), ("reserved", ctypes.c_int32 * 3)]


_SIGNATURES = {
    "fldr_pipe_version": (ctypes.c_int, []),
    "fldr_pipe_error_string": (ctypes.c_char_p, [ctypes.c_int]),
    "fldr_pipe_sizeof": (ctypes.c_int, [ctypes.c_int]),
    "fldr_pipe_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(PipeConfig), ctypes.POINTER(ctypes.c_void_p)]),
    "fldr_pipe_max_out": (ctypes.c_int, [ctypes.c_void_p]),
    "fldr_pipe_pending": (ctypes.c_int, [ctypes.c_void_p]),
    "fldr_pipe_input": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Frame)]),
    "fldr_pipe_submit": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Frame)]),
    "fldr_pipe_receive": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Frame), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(SceneResult)]),
    "fldr_pipe_receive_view": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Frame), ctypes.POINTER(ctypes.c_int),
                                              ctypes.POINTER(SceneResult)]),
    "fldr_pipe_flush": (ctypes.c_int, [ctypes.c_void_p]),
    "fldr_pipe_reset": (ctypes.c_int, [ctypes.c_void_p]),
    "fldr_pipe_destroy": (None, [ctypes.c_void_p]),
}
EXPORTS = tuple(_SIGNATURES)
_lib = None


class PipeError(RuntimeError):
    def __init__(self, what, code):
        super().__init__("%s failed: %s (code %d)" % (what, lib().fldr_pipe_error_string(code).decode(), code))
        self.code = code


class PipeFull(PipeError):
    pass


class PipeEmpty(PipeError):
    pass


def lib():
    """The loaded libfldr_pipe.so, checked against this binding (struct size, header version); raises when it has not been built."""
    global _lib
    if _lib is None:
        fldr_rate.lib()
        _lib = fldr_model.load_library(LIB_PATH, _SIGNATURES, (PipeConfig,), "fldr_pipe", PIPE_VERSION)
    return _lib


def _check(code, what):
    if code != 0:
        raise {E_FULL: PipeFull, E_EMPTY: PipeEmpty}.get(code, PipeError)(what, code)


def pipe_config(H, W, fmt, in_rate, out_rate, depth, scene=True, params=None, device=0):
    """A fldr_pipe_config: fldr_rate.Converter's arguments plus the depth."""
    cfg = PipeConfig()
    rate_config(H, W, fmt, in_rate, out_rate, scene, params, device, into=cfg.rate)
    cfg.depth = int(depth)
    return cfg


class Pipe:
    """fldr_pipe: host frames (tuples of numpy planes) submitted one by one at in_rate; every submit and every flush is one job, and
    jobs are received in order, each with the frames and the scene dict Converter.push / flush returns for it."""
    _h = None

    def __init__(self, native_model, H, W, fmt=None, in_rate=24, out_rate=60, depth=3, scene=True, params=None):
        fmt = fmt or Format()
        cfg = pipe_config(H, W, fmt, in_rate, out_rate, depth, scene, params, native_model.device.index or 0)
        self._h = ctypes.c_void_p()
        self.model = native_model                                    # the pipe uses the model: keep it alive
        _check(lib().fldr_pipe_create(native_model._h, ctypes.byref(cfg), ctypes.byref(self._h)), "fldr_pipe_create")
        self.H, self.W, self.format, self.depth = int(H), int(W), fmt, int(depth)
        self.max_out = lib().fldr_pipe_max_out(self._h)
        self._shapes = plane_shapes(fmt, H, W)
        self._dtype = np.dtype(plane_dtype(fmt, numpy=True))
        self._outs = [tuple(np.empty(s, self._dtype) for s in self._shapes) for _ in range(self.max_out)]
        self._out_structs = (Frame * self.max_out)(*[frame_struct(o) for o in self._outs])
        self._views = (Frame * self.max_out)()

    @property
    def pending(self):
        return lib().fldr_pipe_pending(self._h)

    def _planes_at(self, fr):
        """numpy views of the packed planes a library-filled Frame points to (pinned memory of the pipe)."""
        out = []
        for p, (r, c) in enumerate(self._shapes):
            nbytes = r * c * self._dtype.itemsize
            assert fr.pitch[p] == c * self._dtype.itemsize
            buf = (ctypes.c_uint8 * nbytes).from_address(fr.plane[p])
            out.append(np.frombuffer(buf, dtype=self._dtype).reshape(r, c))
        return tuple(out)

    def input_planes(self):
        """The pinned frame the next submit() takes, as writable numpy planes: fill them, then submit() without a frame."""
        fr = Frame()
        _check(lib().fldr_pipe_input(self._h, ctypes.byref(fr)), "fldr_pipe_input")
        return self._planes_at(fr)

    def submit(self, frame=None):
        """Frame n of the stream: copied into pinned memory (frame given) or taken from input_planes() as filled (None).  Returns after
        the enqueue; the caller's arrays may be overwritten at once.  PipeFull with `depth` jobs outstanding."""
        fr = frame_struct(frame) if frame is not None else None
        _check(lib().fldr_pipe_submit(self._h, ctypes.byref(fr) if fr is not None else None), "fldr_pipe_submit")

    def flush(self):
        """The end-of-stream job (Converter.flush's frame, if any); received like any job."""
        _check(lib().fldr_pipe_flush(self._h), "fldr_pipe_flush")

    def receive(self):
        """Wait for the oldest job -> (its output frames as fresh numpy copies, the pair's scene dict)."""
        n = ctypes.c_int(-1)
        res = SceneResult()
        _check(lib().fldr_pipe_receive(self._h, self._out_structs, ctypes.byref(n), ctypes.byref(res)), "fldr_pipe_receive")
        return [tuple(p.copy() for p in o) for o in self._outs[:n.value]], res.as_dict()

    def receive_view(self):
        """The same without a copy: numpy views of the pipe's pinned memory, valid until the next receive / receive_view / reset /
        close, whatever is submitted in between."""
        n = ctypes.c_int(-1)
        res = SceneResult()
        _check(lib().fldr_pipe_receive_view(self._h, self._views, ctypes.byref(n), ctypes.byref(res)), "fldr_pipe_receive_view")
        return [self._planes_at(self._views[k]) for k in range(n.value)], res.as_dict()

    def reset(self):
        _check(lib().fldr_pipe_reset(self._h), "fldr_pipe_reset")

    def close(self):
        if self._h is not None and self._h.value:
            lib().fldr_pipe_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
