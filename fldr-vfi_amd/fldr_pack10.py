"""ctypes binding of libfldr_pack10.so (include/fldr_pack10.h) — frame interpolation on the packed 10-bit containers v210, Y210 and Y410.

    np_ = NativePack10(fldr_model.NativeModel.from_npz(fldr_harness.DEFAULT_WEIGHTS))
    outs = np_.forward((f0, f1), t=[0.5], in_format=Format("v210"), W=1920)       # v210 -> list of n_t output frames
    bgr = to_planar([f0, f1], fmt, W=1920)            # the input converter alone: planar BGR [2,3,H,W] uint16
    frame = from_planar(bgr[0], fmt)                  # the output converter alone
    s = Session(native_model, H, W, n_t=3, in_format=Format("v210"), out_format=Format("y410"))   # host frames, each uploaded once

A device frame is a tuple of ONE 2-D device tensor with stride(1) == 1: uint32 for v210 ([H, 4 ceil(W/6)]: whole 16-byte groups) and
Y410 ([H, W]), uint16 for Y210 ([H, 4 ceil(W/2)]); the pitch is stride(0), so views into wider buffers work (a v210 row at the
customary pitch 128 ceil(W/48) is such a view).  Host frames of a Session are the same as numpy arrays.  A v210 row does not tell the
width, so W is an argument wherever a frame's size is taken from its plane.  Every call enqueues on torch's current stream of the
model's device and returns without synchronising.  No fallback: a missing library raises at load.
"""
import ctypes
import os

import numpy as np
import torch

from fldr_video import YuvApi, YuvError, YuvNative, YuvSession, converter_signatures, yuv_signatures, yuv_structs

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfldr_pack10.so")
PACK10_VERSION = 100              # include/fldr_pack10.h: FLDR_PACK10_VERSION

CONTAINERS = {"v210": 0, "y210": 1, "y410": 2}
MATRICES = {"bt601": 0, "bt709": 1}
RANGES = {"limited": 0, "full": 1}
E_ARG, E_FORMAT, E_PITCH, E_PLANE, E_WORKSPACE, E_DEVICE = -800, -801, -802, -803, -804, -805
RUN = {"v210": 6, "y210": 8, "y410": 8}           # pack10_internal.h: luma pixels per thread (RUN_V210, RUN_WORDS)


class Format(ctypes.Structure):
    _fields_ = [("container", ctypes.c_int32), ("matrix", ctypes.c_int32), ("range", ctypes.c_int32), ("depth", ctypes.c_int32),
                ("reserved", ctypes.c_int32 * 4)]

    def __init__(self, container="v210", matrix="bt709", range="limited", depth=10):
        pick = lambda table, v: table[v] if isinstance(v, str) else int(v)
        super().__init__(pick(CONTAINERS, container), pick(MATRICES, matrix), pick(RANGES, range), int(depth))

    def copy(self):
        return Format(self.container, self.matrix, self.range, self.depth)

    @property
    def bits(self):
        return 10

    @property
    def name(self):
        return {v: k for k, v in CONTAINERS.items()}.get(self.container, self.container)


class Frame(ctypes.Structure):
    _fields_ = [("plane", ctypes.c_void_p * 3), ("pitch", ctypes.c_int64 * 3)]


IO, SessionConfig = yuv_structs(Format, Frame)
_SIGNATURES = {**yuv_signatures("fldr_pack10_", Frame, IO, SessionConfig), **converter_signatures("fldr_pack10_", Format, Frame)}
EXPORTS = tuple(_SIGNATURES)


class Pack10Error(YuvError):
    pass


# ---- geometry ---------------------------------------------------------------------------------------------------------------------
def plane_shapes(fmt, H, W):
    """[(rows, words per row)] of the one plane of an H x W frame, in words of plane_dtype: v210 4 ceil(W/6) dwords (whole groups),
    Y210 4 ceil(W/2) 16-bit words, Y410 W dwords."""
    if fmt.container == 0:
        return [(H, 4 * ((W + 5) // 6))]
    return [(H, 4 * ((W + 1) // 2))] if fmt.container == 1 else [(H, W)]


def plane_dtype(fmt, numpy=False):
    """The element type of a frame's plane: uint32 (v210, Y410) or uint16 (Y210)."""
    if fmt.container == 1:
        return np.uint16 if numpy else torch.uint16
    return np.uint32 if numpy else torch.uint32


def v210_pitch(W):
    """The customary pitch of a v210 row in bytes (rows padded to 48 pixels): one valid pitch among many."""
    return 128 * ((W + 47) // 48)


def frame_struct(planes):
    """A Frame from a tuple of one 2-D plane array (a torch tensor or a numpy array, uint16 or uint32) with unit column stride."""
    f = Frame()
    a = planes[0]
    if torch.is_tensor(a):
        assert a.dtype in (torch.uint16, torch.uint32) and a.dim() == 2 and a.stride(1) == 1, "a plane is 2-D uint16 / uint32 with unit column stride"
        f.plane[0], f.pitch[0] = a.data_ptr(), a.stride(0) * a.element_size()          # pitches are in bytes
    else:
        assert a.dtype in (np.uint16, np.uint32) and a.ndim == 2 and a.strides[1] == a.itemsize, "a plane is 2-D uint16 / uint32 with unit column stride"
        f.plane[0], f.pitch[0] = a.ctypes.data, a.strides[0]
    return f


_YUV = YuvApi("pack10", LIB_PATH, PACK10_VERSION, Pack10Error, _SIGNATURES, Format, Frame, IO, SessionConfig, frame_struct, plane_shapes, plane_dtype,
              planar_dtype=lambda fmt: torch.uint16)
lib, empty_frame = _YUV.lib, _YUV.empty_frame


def luma_size(frame, fmt, W=None):
    """(H, W) of a frame.  H is the plane's rows; W must be given for v210 (a row is whole groups of six pixels whatever W is) and for an
    odd width of Y210 (a row tells W only up to its parity); Y410 tells it."""
    r, c = frame[0].shape
    if W is None:
        assert fmt.container != 0, "a v210 row does not tell the frame's width: pass W"
        W = c // 2 if fmt.container == 1 else c
    assert plane_shapes(fmt, r, W)[0][1] <= c, "the plane's rows are shorter than a row of W pixels"
    return r, int(W)


# ---- the converters alone (they need no model) ---------------------------------------------------------------------------------------
def to_planar(frames, fmt, planar=None, W=None, stream=None):
    """fldr_pack10_to_planar: a list of frames in `fmt` (tuples of one device plane tensor, pitches from their strides) -> planar BGR
    [n,3,H,W] uint16 (`planar` when given).  W: the luma width (required for v210)."""
    H, W = luma_size(frames[0], fmt, W)
    return _YUV.to_planar(frames, fmt, H, W, planar, stream)


def from_planar(planar, fmt, out=None, stream=None):
    """fldr_pack10_from_planar: a planar BGR device tensor [3,H,W] uint16 with contiguous rows and planes -> one frame in `fmt` (`out`: a
    tuple of one plane tensor, the pitch from its stride; allocated packed otherwise)."""
    return _YUV.from_planar(planar, fmt, out, stream)


class NativePack10(YuvNative):
    """v210 / Y210 / Y410 forwards and the two converters on a fldr_model.NativeModel (read-only: forwards on several streams, each with
    its own workspace, may run at once)."""

    _yuv = _YUV
    to_planar = staticmethod(to_planar)
    from_planar = staticmethod(from_planar)

    def planar(self, ws, H, W, n_t=1):
        """Views into a workspace after a forward: (pair [2,3,H,W], outputs [n_t][3,H,W]), uint16."""
        return super().planar(ws, H, W, n_t, 10, 10)

    def forward(self, frames, t=0.5, in_format=None, out_format=None, outs=None, ws=None, W=None, stream=None):
        """frames: (I0, I1), each a tuple of one plane tensor in in_format; t: n_t values (a float32 device tensor is used in place: a
        captured call reads it at replay); W: the luma width (required for v210).  -> the n_t output frames (`outs` when given;
        allocated packed otherwise)."""
        in_format = in_format or Format()
        H, W = luma_size(frames[0], in_format, W)
        return self._yuv_forward(frames, t, in_format, out_format, outs, ws, H, W, stream)


class Session(YuvSession):
    """fldr_pack10_session: host frames (tuples of one numpy plane) pushed one by one; each push after the first returns n_t frames."""

    _yuv = _YUV
