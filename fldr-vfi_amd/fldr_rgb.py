"""ctypes binding of libfldr_rgb.so (include/fldr_rgb.h) — frame interpolation on RGB frames: four bytes per pixel (BGRA, RGBA, ARGB,
ABGR), 10-bit RGB in one 32-bit word (x2rgb10le, x2bgr10le) and planar GBR(A) at 8 or 10 bits, with alpha.

    nr = NativeRgb(fldr_model.NativeModel.from_npz(fldr_harness.DEFAULT_WEIGHTS))
    outs = nr.forward((f0, f1), t=[0.5], in_format=Format("bgra", alpha="blend"))     # BGRA -> list of n_t output frames
    bgr = to_planar([f0, f1], fmt)                    # the input converter alone: planar BGR [2,3,H,W] uint8 (uint16 at depth 10)
    frame = from_planar(bgr[0], fmt)                  # the output converter alone (opaque alpha)
    alpha([f0, f1], fmt, [frame], Format("bgra", alpha="blend"), t_dev)        # the alpha pass alone, on a converted frame
    s = Session(native_model, H, W, n_t=3, in_format=Format("argb"), out_format=Format("gbrap", alpha="nearer"))

A device frame is a tuple of 2-D device tensors with stride(1) == 1: ONE uint8 tensor [H, 4 W] for the byte layouts (an [H, W, 4] tensor
with unit strides inside a row is taken as that), ONE uint32 tensor [H, W] for the 10-bit words, three or four uint8 / uint16 tensors
[H, W] in the order G, B, R(, A) for gbrp / gbrap; the pitch is stride(0), so views into wider buffers work.  Host frames of a Session are
the same as numpy arrays.  Every call enqueues on torch's current stream of the model's device and returns without synchronising.  No
fallback: a missing library raises at load.
"""
import ctypes
import os

import numpy as np
import torch

from fldr_video import YuvApi, YuvError, YuvNative, YuvSession, _stream_ptr, converter_signatures, yuv_signatures, yuv_structs

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfldr_rgb.so")
RGB_VERSION = 100                 # include/fldr_rgb.h: FLDR_RGB_VERSION

LAYOUTS = {"bgra": 0, "rgba": 1, "argb": 2, "abgr": 3, "x2rgb10": 4, "x2bgr10": 5, "gbrp": 6, "gbrap": 7}
ALPHAS = {"opaque": 0, "nearer": 1, "blend": 2}
E_ARG, E_FORMAT, E_PITCH, E_PLANE, E_WORKSPACE, E_DEVICE = -900, -901, -902, -903, -904, -905
RUN_WORDS = 4                     # rgb_internal.h: pixels of a word layout per thread


class Format(ctypes.Structure):
    _fields_ = [("layout", ctypes.c_int32), ("depth", ctypes.c_int32), ("alpha", ctypes.c_int32), ("reserved", ctypes.c_int32 * 5)]

    def __init__(self, layout="bgra", depth=None, alpha="opaque"):
        pick = lambda table, v: table[v] if isinstance(v, str) else int(v)
        lay = pick(LAYOUTS, layout)
        super().__init__(lay, int(depth) if depth is not None else (10 if lay in (4, 5) else 8), pick(ALPHAS, alpha))

    def copy(self):
        return Format(self.layout, self.depth, self.alpha)

    @property
    def bits(self):
        return 10 if self.depth == 10 else 8

    @property
    def name(self):
        return {v: k for k, v in LAYOUTS.items()}.get(self.layout, self.layout)


class Frame(ctypes.Structure):
    _fields_ = [("plane", ctypes.c_void_p * 4), ("pitch", ctypes.c_int64 * 4)]


IO, SessionConfig = yuv_structs(Format, Frame)
_SIGNATURES = {
    **yuv_signatures("fldr_rgb_", Frame, IO, SessionConfig),
    **converter_signatures("fldr_rgb_", Format, Frame),
    "fldr_rgb_alpha": (ctypes.c_int, [ctypes.POINTER(Frame), ctypes.POINTER(Format), ctypes.POINTER(Frame), ctypes.c_int, ctypes.POINTER(Format),
                                      ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
}
EXPORTS = tuple(_SIGNATURES)


class RgbError(YuvError):
    pass


# ---- geometry ---------------------------------------------------------------------------------------------------------------------
def plane_shapes(fmt, H, W):
    """[(rows, elements per row)] of each plane of an H x W frame, in elements of plane_dtype: 4 W bytes (byte layouts), W dwords (10-bit
    words), W samples in each of three or four planes (gbrp, gbrap)."""
    if fmt.layout <= 3:
        return [(H, 4 * W)]
    if fmt.layout <= 5:
        return [(H, W)]
    return [(H, W)] * (3 if fmt.layout == 6 else 4)


def plane_dtype(fmt, numpy=False):
    """The element type of a frame's planes: uint8 (byte layouts, planar depth 8), uint32 (10-bit words), uint16 (planar depth 10)."""
    if fmt.layout in (4, 5):
        return np.uint32 if numpy else torch.uint32
    if fmt.layout >= 6 and fmt.depth == 10:
        return np.uint16 if numpy else torch.uint16
    return np.uint8 if numpy else torch.uint8


def planar_dtype(fmt, numpy=False):
    """The sample type of the model's planar BGR frames for this format: uint16 at depth 10, uint8 otherwise."""
    if fmt.depth == 10:
        return np.uint16 if numpy else torch.uint16
    return np.uint8 if numpy else torch.uint8


def frame_struct(planes):
    """A Frame from a tuple of one, three or four plane arrays (torch tensors or numpy arrays; uint8, uint16 or uint32): 2-D with unit
    column stride, or for a byte layout [H, W, 4] uint8 with unit strides inside a row."""
    f = Frame()
    for p, a in enumerate(planes):
        is_t = torch.is_tensor(a)
        shape = tuple(a.shape)
        item = a.element_size() if is_t else a.itemsize
        strides = tuple(s * item for s in a.stride()) if is_t else a.strides                    # bytes
        assert a.dtype in ((torch.uint8, torch.uint16, torch.uint32) if is_t else (np.uint8, np.uint16, np.uint32)), "planes are uint8 / uint16 / uint32"
        assert (len(shape) == 2 and strides[1] == item) or (len(shape) == 3 and shape[2] == 4 and item == 1 and strides[1:] == (4, 1)), \
            "a plane is 2-D with unit column stride, or [H, W, 4] bytes"
        f.plane[p], f.pitch[p] = (a.data_ptr() if is_t else a.ctypes.data), strides[0]
    return f


_YUV = YuvApi("rgb", LIB_PATH, RGB_VERSION, RgbError, _SIGNATURES, Format, Frame, IO, SessionConfig, frame_struct, plane_shapes, plane_dtype,
              planar_dtype)
lib, empty_frame = _YUV.lib, _YUV.empty_frame


def frame_size(frame, fmt):
    """(H, W) of a frame, from its first plane."""
    shape = tuple(frame[0].shape)
    return (shape[0], shape[1]) if len(shape) == 3 or fmt.layout > 3 else (shape[0], shape[1] // 4)


# ---- the converters alone (they need no model) ---------------------------------------------------------------------------------------
def to_planar(frames, fmt, planar=None, stream=None):
    """fldr_rgb_to_planar: a list of frames in `fmt` (tuples of device plane tensors, pitches from their strides) -> planar BGR
    [n,3,H,W], uint8 or (depth 10) uint16 (`planar` when given)."""
    H, W = frame_size(frames[0], fmt)
    return _YUV.to_planar(frames, fmt, H, W, planar, stream)


def from_planar(planar, fmt, out=None, stream=None):
    """fldr_rgb_from_planar: a planar BGR device tensor [3,H,W] (uint8; uint16 at depth 10) with contiguous rows and planes -> one frame
    in `fmt` with opaque alpha (`out`: a tuple of plane tensors, pitches from their strides; allocated packed otherwise)."""
    return _YUV.from_planar(planar, fmt, out, stream)


def alpha(frames, in_format, outs, out_format, t, stream=None):
    """fldr_rgb_alpha: the alpha of the frames `outs` in out_format (as from_planar left them) by out_format's policy from the two frames
    `frames` in in_format at the times t (a float32 device tensor of len(outs) values).  -> outs."""
    H, W = frame_size(frames[0], in_format)
    assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == len(outs)
    _YUV.check(_YUV.fn("alpha")(_YUV.frame_array(frames), ctypes.byref(in_format), _YUV.frame_array(outs), len(outs), ctypes.byref(out_format),
                                ctypes.c_void_p(t.data_ptr()), int(H), int(W), _stream_ptr(t.device, stream)), "alpha")
    return outs


class NativeRgb(YuvNative):
    """RGB forwards and the two converters on a fldr_model.NativeModel (read-only: forwards on several streams, each with its own
    workspace, may run at once)."""

    _yuv = _YUV
    to_planar = staticmethod(to_planar)
    from_planar = staticmethod(from_planar)
    alpha = staticmethod(alpha)

    def forward(self, frames, t=0.5, in_format=None, out_format=None, outs=None, ws=None, stream=None):
        """frames: (I0, I1), each a tuple of plane tensors in in_format; t: n_t values (a float32 device tensor is used in place: a
        captured call reads it at replay); the alpha policy is out_format's.  -> the n_t output frames (`outs` when given; allocated
        packed otherwise)."""
        in_format = in_format or Format()
        H, W = frame_size(frames[0], in_format)
        return self._yuv_forward(frames, t, in_format, out_format, outs, ws, H, W, stream)


class Session(YuvSession):
    """fldr_rgb_session: host frames (tuples of numpy planes) pushed one by one; each push after the first returns n_t frames."""

    _yuv = _YUV
