"""ctypes binding of libfldr_chroma.so (include/fldr_chroma.h) — frame interpolation on YUV 4:2:2 and 4:4:4 frames at 8 and 10 bits.

    nc = NativeChroma(fldr_model.NativeModel.from_npz(fldr_harness.DEFAULT_WEIGHTS))
    outs = nc.forward((f0, f1), t=[0.5], in_format=Format("422", "semiplanar", depth=10))      # P210 -> list of n_t output frames
    bgr = nc.to_planar([f0, f1], fmt)                 # the input converter alone: planar BGR [2,3,H,W]
    frame = nc.from_planar(bgr[0], fmt)               # the output converter alone
    s = Session(native_model, H, W, n_t=3, in_format=Format("422", "uyvy"))    # host frames (numpy planes), each uploaded once

A device frame is a tuple of 2-D device tensors, one per plane (planar: Y, U, V; semiplanar: Y, UV; uyvy / yuyv: one plane), uint8, or
uint16 at depth 10, each [rows, samples per row] with stride(1) == 1; the pitch is stride(0), so views into wider buffers work.  Host
frames of a Session are the same as numpy arrays.  Every call enqueues on torch's current stream of the model's device and returns
without synchronising.  No fallback: a missing library raises at load.
"""
import ctypes
import os

import numpy as np
import torch

from fldr_video import (YuvApi, YuvError, YuvNative, YuvSession, converter_signatures, frame_struct as _video_frame_struct, yuv_signatures,
                        yuv_structs)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfldr_chroma.so")
CHROMA_VERSION = 100              # include/fldr_chroma.h: FLDR_CHROMA_VERSION

SAMPLINGS = {"422": 0, "444": 1}
LAYOUTS = {"planar": 0, "semiplanar": 1, "uyvy": 2, "yuyv": 3}
MATRICES = {"bt601": 0, "bt709": 1}
RANGES = {"limited": 0, "full": 1}
E_ARG, E_FORMAT, E_PITCH, E_PLANE, E_WORKSPACE, E_DEVICE = -700, -701, -702, -703, -704, -705
RUN = {8: 16, 10: 8}              # chroma_internal.h: luma pixels per thread at each depth (the wide form needs W % RUN == 0)


class Format(ctypes.Structure):
    _fields_ = [("sampling", ctypes.c_int32), ("layout", ctypes.c_int32), ("matrix", ctypes.c_int32), ("range", ctypes.c_int32),
                ("depth", ctypes.c_int32), ("reserved", ctypes.c_int32 * 3)]

    def __init__(self, sampling="422", layout="planar", matrix="bt709", range="limited", depth=8):
        pick = lambda table, v: table[v] if isinstance(v, str) else int(v)
        super().__init__(pick(SAMPLINGS, sampling), pick(LAYOUTS, layout), pick(MATRICES, matrix), pick(RANGES, range), int(depth))

    def copy(self):
        return Format(self.sampling, self.layout, self.matrix, self.range, self.depth)

    @property
    def bits(self):
        """8 or 10: the depth with the 0 alias resolved."""
        return 10 if self.depth == 10 else 8


class Frame(ctypes.Structure):
    _fields_ = [("plane", ctypes.c_void_p * 3), ("pitch", ctypes.c_int64 * 3)]


IO, SessionConfig = yuv_structs(Format, Frame)
_SIGNATURES = {**yuv_signatures("fldr_chroma_", Frame, IO, SessionConfig), **converter_signatures("fldr_chroma_", Format, Frame)}
EXPORTS = tuple(_SIGNATURES)


class ChromaError(YuvError):
    pass


# ---- geometry ---------------------------------------------------------------------------------------------------------------------
def plane_shapes(fmt, H, W):
    """[(rows, samples per row)] of each plane of an H x W frame: bytes at depth 8, 16-bit words at depth 10 (plane_dtype)."""
    half = (W + 1) // 2
    if fmt.layout >= 2:
        return [(H, 4 * half)]
    cw = W if fmt.sampling == 1 else half
    return [(H, W), (H, 2 * cw)] if fmt.layout == 1 else [(H, W), (H, cw), (H, cw)]


def plane_dtype(fmt, numpy=False):
    """The element type of a frame's planes: uint8, or uint16 for a Format of depth 10."""
    if fmt.bits == 10:
        return np.uint16 if numpy else torch.uint16
    return np.uint8 if numpy else torch.uint8


def frame_struct(planes):
    """A Frame from a tuple of 2-D plane arrays (torch tensors or numpy arrays) with unit column stride."""
    v = _video_frame_struct(planes)
    f = Frame()
    for p in range(3):
        f.plane[p], f.pitch[p] = v.plane[p], v.pitch[p]
    return f


_YUV = YuvApi("chroma", LIB_PATH, CHROMA_VERSION, ChromaError, _SIGNATURES, Format, Frame, IO, SessionConfig, frame_struct, plane_shapes, plane_dtype)
lib, empty_frame = _YUV.lib, _YUV.empty_frame


def luma_size(frame, fmt):
    """(H, W) of a frame from its first plane; a packed plane tells W only up to its parity, so pass W where it is odd."""
    r, c = frame[0].shape
    return (r, c // 2) if fmt.layout >= 2 else (r, c)


# ---- the converters alone (they need no model) ---------------------------------------------------------------------------------------
def to_planar(frames, fmt, planar=None, W=None, stream=None):
    """fldr_chroma_to_planar: a list of frames in `fmt` (tuples of device plane tensors, pitches from their strides) -> planar BGR
    [n,3,H,W] (uint8; uint16 at depth 10; `planar` when given).  W: the luma width of a packed frame when it is odd."""
    H, w = luma_size(frames[0], fmt)
    return _YUV.to_planar(frames, fmt, H, w if W is None else W, planar, stream)


def from_planar(planar, fmt, out=None, stream=None):
    """fldr_chroma_from_planar: a planar BGR device tensor [3,H,W] with contiguous rows and planes (uint8; uint16 at depth 10) -> one
    frame in `fmt` (`out`: a tuple of plane tensors, pitches from their strides; allocated packed otherwise)."""
    return _YUV.from_planar(planar, fmt, out, stream)


class NativeChroma(YuvNative):
    """4:2:2 / 4:4:4 forwards and the two converters on a fldr_model.NativeModel (read-only: forwards on several streams, each with its
    own workspace, may run at once)."""

    _yuv = _YUV
    to_planar = staticmethod(to_planar)
    from_planar = staticmethod(from_planar)

    def forward(self, frames, t=0.5, in_format=None, out_format=None, outs=None, ws=None, W=None, stream=None):
        """frames: (I0, I1), each a tuple of plane tensors in in_format; t: n_t values (a float32 device tensor is used in place: a
        captured call reads it at replay).  -> the n_t output frames (`outs` when given; allocated packed otherwise)."""
        in_format = in_format or Format()
        H, w = luma_size(frames[0], in_format)
        return self._yuv_forward(frames, t, in_format, out_format, outs, ws, H, w if W is None else W, stream)


class Session(YuvSession):
    """fldr_chroma_session: host frames (tuples of numpy planes) pushed one by one; each push after the first returns n_t frames."""

    _yuv = _YUV
