"""ctypes binding of libfldr_video.so (video API: include/fldr_video.h) — frame interpolation on 8-bit YUV 4:2:0 frames (NV12, I420).

    nv = NativeVideo(fldr_model.NativeModel.from_npz(fldr_harness.DEFAULT_WEIGHTS))
    outs = nv.forward((f0, f1), t=[0.5], in_format=Format("nv12"), out_format=Format("nv12"))   # -> list of n_t output frames
    s = Session(native_model, H, W, n_t=3, in_format=Format("i420"))    # host frames (numpy planes), each uploaded once
    outs = s.push((y, u, v))                                            # [] on the first push, n_t frames afterwards

A device frame is a tuple of 2-D uint8 device tensors, one per plane (NV12: Y, UV; I420: Y, U, V), each [rows, row bytes] with
stride(1) == 1; the pitch is stride(0), so views into wider buffers work.  Host frames of a Session are the same as numpy arrays.
Every forward enqueues on torch's current stream of the model's device and returns without synchronising.  No fallback: a missing
library raises at load.
"""
import ctypes
import os

import numpy as np
import torch

import fldr_model

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfldr_video.so")
VIDEO_VERSION = 101               # include/fldr_video.h: FLDR_VIDEO_VERSION

LAYOUTS = {"nv12": 0, "i420": 1}
MATRICES = {"bt601": 0, "bt709": 1}
RANGES = {"limited": 0, "full": 1}
E_ARG, E_FORMAT, E_PITCH, E_PLANE, E_WORKSPACE, E_DEVICE = -100, -101, -102, -103, -104, -105


class Format(ctypes.Structure):
    _fields_ = [("layout", ctypes.c_int32), ("matrix", ctypes.c_int32), ("range", ctypes.c_int32), ("reserved", ctypes.c_int32 * 5)]

    # `reserved` mirrors the five words behind `range` of fldr_video_format: word 0 is `depth` (0 or 8: 8-bit samples, 10: 10-bit
    # samples in 16-bit words — NV12 is then P010, I420 yuv420p10le), words 1 .. 4 are the header's reserved[4]
    def __init__(self, layout="nv12", matrix="bt709", range="limited", depth=8):
        super().__init__(LAYOUTS.get(layout, layout) if isinstance(layout, str) else layout,
                         MATRICES[matrix] if isinstance(matrix, str) else matrix, RANGES[range] if isinstance(range, str) else range)
        self.depth = depth

    def copy(self):
        return Format(self.layout, self.matrix, self.range, self.depth)

    @property
    def depth(self):
        return int(self.reserved[0])

    @depth.setter
    def depth(self, v):
        self.reserved[0] = int(v)

    @property
    def bits(self):
        """8 or 10: the depth with the 0 alias resolved."""
        return 10 if self.depth == 10 else 8

    @property
    def name(self):
        return {0: "nv12", 1: "i420"}.get(self.layout, self.layout)


class Frame(ctypes.Structure):
    _fields_ = [("plane", ctypes.c_void_p * 3), ("pitch", ctypes.c_int64 * 3)]


def yuv_structs(Format, Frame):
    """The IO and SessionConfig struct classes of a library on the model from its Format and Frame (fldr_video_io and
    fldr_video_session_config; fldr_chroma.h, fldr_pack10.h and fldr_rgb.h lay theirs out the same)."""
    class IO(ctypes.Structure):
        _fields_ = [("H", ctypes.c_int32), ("W", ctypes.c_int32), ("in_format", Format), ("in_", Frame * 2), ("out_format", Format),
                    ("n_t", ctypes.c_int32), ("t", ctypes.c_void_p), ("out", ctypes.POINTER(Frame))]

    class SessionConfig(ctypes.Structure):
        _fields_ = [("H", ctypes.c_int32), ("W", ctypes.c_int32), ("in_format", Format), ("out_format", Format), ("n_t", ctypes.c_int32),
                    ("device", ctypes.c_int32), ("t", ctypes.POINTER(ctypes.c_float)), ("reserved", ctypes.c_int32 * 4)]

    return IO, SessionConfig


IO, SessionConfig = yuv_structs(Format, Frame)


def yuv_signatures(prefix, Frame, IO, SessionConfig):
    """The functions every library on the model exports (fldr_video.h, fldr_chroma.h, fldr_pack10.h, fldr_rgb.h), as
    fldr_model.load_library takes them."""
    return {
        prefix + "version": (ctypes.c_int, []),
        prefix + "error_string": (ctypes.c_char_p, [ctypes.c_int]),
        prefix + "sizeof": (ctypes.c_int, [ctypes.c_int]),
        prefix + "workspace_bytes": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
        prefix + "forward": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(IO), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
        prefix + "session_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(SessionConfig), ctypes.POINTER(ctypes.c_void_p)]),
        prefix + "session_push": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Frame), ctypes.POINTER(Frame), ctypes.POINTER(ctypes.c_int)]),
        prefix + "session_reset": (ctypes.c_int, [ctypes.c_void_p]),
        prefix + "session_destroy": (None, [ctypes.c_void_p]),
    }


def converter_signatures(prefix, Format, Frame):
    """The two converters alone, which the chroma, pack10 and rgb libraries export beside the functions of yuv_signatures."""
    return {
        prefix + "to_planar": (ctypes.c_int, [ctypes.POINTER(Frame), ctypes.c_int, ctypes.POINTER(Format), ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_void_p]),
        prefix + "from_planar": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Format), ctypes.POINTER(Frame), ctypes.c_int, ctypes.c_int,
                                                ctypes.c_void_p]),
    }


_SIGNATURES = yuv_signatures("fldr_video_", Frame, IO, SessionConfig)
EXPORTS = tuple(_SIGNATURES)
# libfldr_video_test.so (-DFLDR_TEST_HOOKS): the same sources + the converter hooks of include/fldr_video_test_hooks.h; tests only
TEST_LIB_PATH = os.path.join(_HERE, "libfldr_video_test.so")
_HOOK_SIGNATURES = {
    "fldr_video_debug_to_planar": (ctypes.c_int, [ctypes.POINTER(Frame), ctypes.POINTER(Format), ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "fldr_video_debug_from_planar": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Frame), ctypes.POINTER(Format), ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "fldr_video_debug_last_path": (ctypes.c_int, []),
}
HOOKS = tuple(_HOOK_SIGNATURES)
_hooks_lib = None


class YuvError(RuntimeError):
    """A failed call `what` of a library on the model: its code and the library's string for it (YuvApi.failure makes one); each module
    derives its own class."""

    def __init__(self, what, code, text):
        super().__init__("%s failed: %s (code %d)" % (what, text, code))
        self.code = code


class VideoError(YuvError):
    pass


def test_hooks():
    """The loaded libfldr_video_test.so (the product's sources + the fldr_video_debug_* converter hooks); tests only.  The product
    library stays what lib() returns: the two are separate handles in one process."""
    global _hooks_lib
    if _hooks_lib is None:
        _hooks_lib = fldr_model.load_library(TEST_LIB_PATH, {**_SIGNATURES, **_HOOK_SIGNATURES}, (), "fldr_video", VIDEO_VERSION)
    return _hooks_lib


# ---- geometry ---------------------------------------------------------------------------------------------------------------------
def plane_shapes(layout, H, W):
    """[(rows, samples per row)] of each plane of an H x W frame: bytes at depth 8, 16-bit words at depth 10 (plane_dtype)."""
    ch, cw = (H + 1) // 2, (W + 1) // 2
    return [(H, W), (ch, 2 * cw)] if _layout(layout) == 0 else [(H, W), (ch, cw), (ch, cw)]


def _depth(fmt):
    return fmt.bits if isinstance(fmt, Format) else 8


def plane_dtype(fmt, numpy=False):
    """The element type of a frame's planes: uint8, or uint16 for a Format of depth 10."""
    if _depth(fmt) == 10:
        return np.uint16 if numpy else torch.uint16
    return np.uint8 if numpy else torch.uint8


def _layout(layout):
    return layout.layout if isinstance(layout, Format) else LAYOUTS[layout] if isinstance(layout, str) else int(layout)


def frame_struct(planes):
    """A Frame from a tuple of 2-D plane arrays (torch tensors or numpy arrays) with unit column stride."""
    f = Frame()
    for p, a in enumerate(planes):
        if torch.is_tensor(a):
            assert a.dtype in (torch.uint8, torch.uint16) and a.dim() == 2 and a.stride(1) == 1, "planes are 2-D uint8 / uint16 with unit column stride"
            f.plane[p], f.pitch[p] = a.data_ptr(), a.stride(0) * a.element_size()          # pitches are in bytes
        else:
            assert a.dtype in (np.uint8, np.uint16) and a.ndim == 2 and a.strides[1] == a.itemsize, "planes are 2-D uint8 / uint16 with unit column stride"
            f.plane[p], f.pitch[p] = a.ctypes.data, a.strides[0]
    return f


def empty_frame(layout, H, W, device):
    return tuple(torch.empty(r, c, dtype=plane_dtype(layout), device=device) for r, c in plane_shapes(layout, H, W))


def _stream_ptr(device, stream):
    """The hipStream_t of `stream` (a torch.cuda.Stream), or of torch's current stream of `device` when None."""
    st = stream if stream is not None else torch.cuda.current_stream(device)
    return ctypes.c_void_p(st.cuda_stream)


# ---- the converters alone (test build) ----------------------------------------------------------------------------------------------
def debug_to_planar(frames, fmt, pair=None, stream=None):
    """fldr_video_debug_to_planar: frames (I0, I1), each a tuple of device plane tensors in `fmt` (pitches from their strides) -> the
    planar BGR pair [2,3,H,W] (uint8; uint16 at depth 10; `pair` when given).  Enqueues on torch's current stream."""
    H, W = frames[0][0].shape
    if pair is None:
        pair = torch.empty(2, 3, H, W, dtype=plane_dtype(fmt), device=frames[0][0].device)
    arr = (Frame * 2)(*[frame_struct(f) for f in frames])
    _YUV.check(test_hooks().fldr_video_debug_to_planar(arr, ctypes.byref(fmt), ctypes.c_void_p(pair.data_ptr()), int(H), int(W),
                                                       _stream_ptr(pair.device, stream)), "debug_to_planar")
    return pair


def debug_from_planar(planar, fmt, out=None, stream=None):
    """fldr_video_debug_from_planar: a contiguous planar BGR device tensor [3,H,W] (uint8; uint16 at depth 10) -> one frame in `fmt`
    (`out`: a tuple of plane tensors, pitches from their strides; allocated packed otherwise).  Enqueues on torch's current stream."""
    _, H, W = planar.shape
    assert planar.is_contiguous() and planar.dtype == plane_dtype(fmt)
    if out is None:
        out = empty_frame(fmt, H, W, planar.device)
    fr = frame_struct(out)
    _YUV.check(test_hooks().fldr_video_debug_from_planar(ctypes.c_void_p(planar.data_ptr()), ctypes.byref(fr), ctypes.byref(fmt), int(H), int(W),
                                                         _stream_ptr(planar.device, stream)), "debug_from_planar")
    return out


def debug_last_path():
    """1: the most recent converter launch of the test build took the wide-access (VEC) form, 0: the per-sample form, -1: none yet."""
    return int(test_hooks().fldr_video_debug_last_path())


class YuvApi:
    """One library on the model, as YuvNative and YuvSession use it: its name (the functions are fldr_<name>_*), path and header version,
    its error class, the signatures of its functions, its struct classes and the geometry functions of its frames (planar_dtype: the
    sample type of the model's planar BGR frames for a format, where that is not the planes').  Loads the library on first use."""

    def __init__(self, name, path, version, error, signatures, Format, Frame, IO, SessionConfig, frame_struct, plane_shapes, plane_dtype,
                 planar_dtype=None):
        self.name, self.prefix, self.path, self.version, self.error, self.signatures = name, "fldr_%s_" % name, path, version, error, signatures
        self.Format, self.Frame, self.IO, self.SessionConfig = Format, Frame, IO, SessionConfig
        self.frame_struct, self.plane_shapes, self.plane_dtype = frame_struct, plane_shapes, plane_dtype
        self.planar_dtype = planar_dtype or plane_dtype
        self._lib = None

    def lib(self):
        """The loaded library, checked against this binding (struct sizes, header version); raises when it has not been built."""
        if self._lib is None:
            self._lib = fldr_model.load_library(self.path, self.signatures, (self.Format, self.Frame, self.IO, self.SessionConfig),
                                                "fldr_" + self.name, self.version)
        return self._lib

    def fn(self, name):
        return getattr(self.lib(), self.prefix + name)

    def failure(self, name, code):
        """The library's error for the code its function `name` returned."""
        return self.error(self.prefix + name, code, self.fn("error_string")(code).decode())

    def check(self, code, name):
        if code != 0:
            raise self.failure(name, code)

    def empty_frame(self, fmt, H, W, device):
        return tuple(torch.empty(r, c, dtype=self.plane_dtype(fmt), device=device) for r, c in self.plane_shapes(fmt, H, W))

    def frame_array(self, frames):
        return (self.Frame * len(frames))(*[self.frame_struct(f) for f in frames])

    # the converters alone (they need no model; libfldr_video.so exports none)
    def to_planar(self, frames, fmt, H, W, planar=None, stream=None):
        """fldr_<name>_to_planar: a list of H x W frames in `fmt` (tuples of device plane tensors, pitches from their strides) -> planar
        BGR [n,3,H,W] (`planar` when given)."""
        device = frames[0][0].device
        if planar is None:
            planar = torch.empty(len(frames), 3, H, W, dtype=self.planar_dtype(fmt), device=device)
        self.check(self.fn("to_planar")(self.frame_array(frames), len(frames), ctypes.byref(fmt), ctypes.c_void_p(planar.data_ptr()), int(H), int(W),
                                        _stream_ptr(device, stream)), "to_planar")
        return planar

    def from_planar(self, planar, fmt, out=None, stream=None):
        """fldr_<name>_from_planar: a planar BGR device tensor [3,H,W] with contiguous rows and planes -> one frame in `fmt` (`out`: a
        tuple of plane tensors, pitches from their strides; allocated packed otherwise)."""
        _, H, W = planar.shape
        assert planar.is_contiguous() and planar.dtype == self.planar_dtype(fmt)
        if out is None:
            out = self.empty_frame(fmt, H, W, planar.device)
        fr = self.frame_struct(out)
        self.check(self.fn("from_planar")(ctypes.c_void_p(planar.data_ptr()), ctypes.byref(fmt), ctypes.byref(fr), int(H), int(W),
                                          _stream_ptr(planar.device, stream)), "from_planar")
        return out


_YUV = YuvApi("video", LIB_PATH, VIDEO_VERSION, VideoError, _SIGNATURES, Format, Frame, IO, SessionConfig, frame_struct, plane_shapes, plane_dtype)
lib = _YUV.lib


class YuvNative:
    """YUV forwards of the library `_yuv` (a YuvApi) on a fldr_model.NativeModel; a subclass names the library and gives `forward` its
    signature."""

    def __init__(self, native_model):
        self._yuv.lib()
        self.model = native_model
        self.device = native_model.device

    def workspace_bytes(self, H, W, n_t=1):
        n = self._yuv.fn("workspace_bytes")(self.model._h, int(H), int(W), int(n_t))
        if n < 0:
            raise self._yuv.failure("workspace_bytes", int(n))
        return int(n)

    def workspace(self, H, W, n_t=1):
        return torch.empty(self.workspace_bytes(H, W, n_t), dtype=torch.uint8, device=self.device)

    def planar(self, ws, H, W, n_t=1, in_depth=8, out_depth=8):
        """Views into a workspace after a forward: (pair [2,3,H,W], outputs [n_t][3,H,W]) — the planar BGR frames of the model, uint8, or
        uint16 for the side whose format had depth 10."""
        mb = fldr_model.lib().fldr_model_workspace_bytes(self.model._h, int(H), int(W), int(n_t))
        al = lambda v: (v + 255) // 256 * 256
        bi, bo = (2 if in_depth == 10 else 1), (2 if out_depth == 10 else 1)
        as_ = lambda x, b, shape: (x.view(torch.uint16) if b == 2 else x).view(shape)
        pair = as_(ws[al(mb):al(mb) + 6 * H * W * bi], bi, (2, 3, H, W))
        o = al(mb) + al(6 * H * W * bi)
        st = al(3 * H * W * bo)
        outs = [as_(ws[o + k * st:o + k * st + 3 * H * W * bo], bo, (3, H, W)) for k in range(n_t)]
        return pair, outs

    def forward_io(self, io, ws, stream=None):
        """The raw call; returns the code without raising (tests of the error contract)."""
        return self._yuv.fn("forward")(self.model._h, ctypes.byref(io), ctypes.c_void_p(ws.data_ptr()) if ws is not None else None,
                                       ws.numel() if ws is not None else 0, _stream_ptr(self.device, stream))

    def _t(self, t):
        """t as the float32 device tensor a forward reads: one that already is (contiguous, on a device) is used in place."""
        if torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous():
            return t
        return torch.as_tensor(t, dtype=torch.float32).reshape(-1).to(self.device)

    def make_io(self, frames, t, in_format, out_format, outs, H, W):
        io = self._yuv.IO()
        io.H, io.W = int(H), int(W)
        io.in_format, io.out_format = in_format, out_format
        for i, fr in enumerate(frames):
            io.in_[i] = self._yuv.frame_struct(fr)
        arr = self._yuv.frame_array(outs)
        io.n_t, io.t, io.out = len(outs), t.data_ptr(), ctypes.cast(arr, ctypes.POINTER(self._yuv.Frame))
        io._keep = arr
        return io

    def _yuv_forward(self, frames, t, in_format, out_format, outs, ws, H, W, stream):
        """What a subclass's forward does once it knows its formats and the frame size."""
        in_format = in_format or self._yuv.Format()
        out_format = out_format or in_format.copy()
        tt = self._t(t)
        n_t = tt.numel()
        if outs is None:
            outs = [self._yuv.empty_frame(out_format, H, W, self.device) for _ in range(n_t)]
        if ws is None:
            ws = self.workspace(H, W, n_t)
        io = self.make_io(frames, tt, in_format, out_format, outs, H, W)
        self._yuv.check(self.forward_io(io, ws, stream), "forward")
        return outs


class NativeVideo(YuvNative):
    """YUV forwards on a fldr_model.NativeModel (read-only: forwards on several streams, each with its own workspace, may run at once)."""

    _yuv = _YUV

    def forward(self, frames, t=0.5, in_format=None, out_format=None, outs=None, ws=None, stream=None):
        """frames: (I0, I1), each a tuple of plane tensors in in_format; t: n_t values (a float32 device tensor is used in place: a
        captured call reads it at replay).  -> the n_t output frames (`outs` when given; allocated packed otherwise)."""
        H, W = frames[0][0].shape
        return self._yuv_forward(frames, t, in_format, out_format, outs, ws, H, W, stream)


class HostStream:
    """What Session and fldr_rate.Converter share: the lifetime of the handle `_h` (a subclass names the library's `_destroy`) and the
    host planes the library writes a push's output frames into (frames of the library `_yuv`: 4:2:0 unless a subclass says otherwise)."""
    _h = None
    _yuv = _YUV

    def _stage(self, fmt, H, W, n):
        self._outs = [tuple(np.empty(s, self._yuv.plane_dtype(fmt, numpy=True)) for s in self._yuv.plane_shapes(fmt, H, W)) for _ in range(n)]

    def _out_structs(self):
        return self._yuv.frame_array(self._outs)

    def _taken(self, n):
        """The first n staged frames as fresh copies."""
        return [tuple(p.copy() for p in o) for o in self._outs[:n]]

    def close(self):
        if self._h is not None and self._h.value:
            self._destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ReportStream(HostStream):
    """What fldr_field.Stream and fldr_interlace.Interlacer share: push, flush and reset of a library whose calls fill one report per
    returned frame (last_reports: their dicts).  A subclass names `_lib` and `_check` of its module, its `_Report` struct and, in
    `_calls`, the library's destroy, push, flush and reset; its __init__ sets `_h` and `max_out` and stages the output frames."""

    def _destroy(self, h):
        getattr(self._lib(), self._calls[0])(h)

    def _run(self, what, *head):
        n = ctypes.c_int(-1)
        reps = (self._Report * self.max_out)()
        self._check(getattr(self._lib(), what)(self._h, *head, self._out_structs(), ctypes.byref(n), reps), what)
        self.last_reports = [reps[k].as_dict() for k in range(n.value)]
        return self._taken(n.value)

    def push(self, frame):
        """-> the list of frames due (tuples of numpy planes, fresh copies); self.last_reports: their report dicts."""
        fr = self._yuv.frame_struct(frame)
        return self._run(self._calls[1], ctypes.byref(fr))

    def flush(self):
        return self._run(self._calls[2])

    def reset(self):
        self._check(getattr(self._lib(), self._calls[3])(self._h), self._calls[3])


class YuvSession(HostStream):
    """The session of the library `_yuv`: host frames (tuples of numpy planes) pushed one by one; each push after the first returns n_t
    frames."""

    def _destroy(self, h):
        self._yuv.fn("session_destroy")(h)

    def __init__(self, native_model, H, W, n_t=1, in_format=None, out_format=None, t=None):
        in_format = in_format or self._yuv.Format()
        out_format = out_format or in_format.copy()
        cfg = self._yuv.SessionConfig()
        cfg.H, cfg.W, cfg.n_t, cfg.device = int(H), int(W), int(n_t), native_model.device.index or 0
        cfg.in_format, cfg.out_format = in_format, out_format
        if t is not None:
            ta = (ctypes.c_float * n_t)(*[float(v) for v in t])
            cfg.t = ctypes.cast(ta, ctypes.POINTER(ctypes.c_float))
        self._h = ctypes.c_void_p()
        self.model = native_model                                    # the session uses the model: keep it alive
        self._yuv.check(self._yuv.fn("session_create")(native_model._h, ctypes.byref(cfg), ctypes.byref(self._h)), "session_create")
        self.H, self.W, self.n_t, self.in_format, self.out_format = int(H), int(W), int(n_t), in_format, out_format
        self._stage(out_format, H, W, n_t)

    def push(self, frame):
        """-> [] or a list of n_t output frames (tuples of numpy planes, fresh copies)."""
        fr = self._yuv.frame_struct(frame)
        n = ctypes.c_int(-1)
        self._yuv.check(self._yuv.fn("session_push")(self._h, ctypes.byref(fr), self._out_structs(), ctypes.byref(n)), "session_push")
        self.last_n_out = n.value
        return self._taken(n.value)

    def reset(self):
        self._yuv.check(self._yuv.fn("session_reset")(self._h), "session_reset")


class Session(YuvSession):
    """fldr_video_session: host frames (tuples of numpy planes) pushed one by one; each push after the first returns n_t frames."""

