"""ctypes binding of libfldr_model.so (C model API: include/fldr_model.h) — the whole default forward behind one C call.

    m = NativeModel.from_npz(fldr_harness.DEFAULT_WEIGHTS, device=0)        # or NativeModel.from_module(model)
    frame = m.forward_pyramid(pyr, t)                 # fp64 [n_t,3,Hp,Wp], the frame of DCTXVFInet.forward before its crop view
    img = m.interpolate_u8(frames_u8, t)              # uint8 [n_t,3,H,W], as fldr_harness.interpolate_u8
    img = m.interpolate_u8(pair=(a_hwc, b_hwc), t=t, order="bgr", out_layout="hwc")     # interleaved frames in and out
    frames = m.interpolate_multi(frames, [k / 8 for k in range(1, 8)])                  # as fldr_harness.interpolate_multi

Every call enqueues on torch's current stream of the model's device and returns without synchronising.  The workspace comes from
`workspace(H, W, n_t)` (a byte tensor; allocated per call when not given).  Like fldr_hip, there is no fallback: a missing library
raises at load.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfldr_model.so")
MODEL_VERSION = 101               # include/fldr_model.h: FLDR_MODEL_VERSION
MAX_LEVELS = 8

F32, F64 = 0, 1
IN_PYRAMID, IN_U8_PLANAR, IN_U8_INTERLEAVED, IN_U10_PLANAR = 0, 1, 2, 3
OUT_F64, OUT_U8_PLANAR, OUT_U8_INTERLEAVED, OUT_U10_PLANAR = 0, 1, 2, 3
ORDERS = {"bgr": 0, "rgb": 1}
E_ARG, E_SHAPE, E_STATUS, E_WORKSPACE, E_BATCH = -1, -2, -3, -10, -11
E_IO, E_FORMAT, E_COMPRESSED, E_TRUNCATED, E_MISSING, E_TENSOR_SHAPE, E_DTYPE, E_DEVICE = -12, -13, -14, -15, -16, -17, -18, -19


class Tensor(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("data", ctypes.c_void_p), ("dtype", ctypes.c_int32), ("ndim", ctypes.c_int32),
                ("shape", ctypes.c_int64 * 4)]


class Config(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("test_scales", ctypes.c_int32), ("reserved", ctypes.c_int32 * 6)]


class IO(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("input", ctypes.c_int32),
                ("pyramid", ctypes.c_void_p * MAX_LEVELS), ("frames_u8", ctypes.c_void_p), ("frame", ctypes.c_void_p * 2),
                ("frame_pitch", ctypes.c_int64 * 2), ("in_order", ctypes.c_int32), ("n_t", ctypes.c_int32), ("t", ctypes.c_void_p),
                ("output", ctypes.c_int32), ("out_order", ctypes.c_int32), ("out", ctypes.POINTER(ctypes.c_void_p)),
                ("out_pitch", ctypes.c_int64)]


_SIGNATURES = {
    "fldr_model_version": (ctypes.c_int, []),
    "fldr_model_error_string": (ctypes.c_char_p, [ctypes.c_int]),
    "fldr_model_sizeof": (ctypes.c_int, [ctypes.c_int]),
    "fldr_model_create": (ctypes.c_int, [ctypes.POINTER(Tensor), ctypes.c_int, ctypes.POINTER(Config), ctypes.POINTER(ctypes.c_void_p)]),
    "fldr_model_create_npz": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(Config), ctypes.POINTER(ctypes.c_void_p)]),
    "fldr_model_destroy": (None, [ctypes.c_void_p]),
    "fldr_model_workspace_bytes": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "fldr_model_forward": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(IO), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "fldr_model_interpolate_host": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                                   ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
}
EXPORTS = tuple(_SIGNATURES)
_lib = None


class ModelError(RuntimeError):
    def __init__(self, what, code):
        super().__init__("%s failed: %s (code %d)" % (what, lib().fldr_model_error_string(code).decode(), code))
        self.code = code


def load_library(path, signatures, structs, prefix, version):
    """ctypes.CDLL(path) with `signatures` set, checked against a binding: sizeof(structs[i]) == <prefix>_sizeof(i) and <prefix>_version()
    == version.  ImportError when the file has not been built or does not match.  fldr_video and fldr_rate load through it too."""
    if not os.path.exists(path):
        raise ImportError("%s is missing — build it with `make -C fldr-vfi_amd/csrc` (or __graft_entry__.build())" % path)
    l = ctypes.CDLL(path)
    for name, (res, args) in signatures.items():
        fn = getattr(l, name)
        fn.restype, fn.argtypes = res, args
    sizeof, reported = getattr(l, prefix + "_sizeof"), getattr(l, prefix + "_version")()
    for which, cls in enumerate(structs):
        if sizeof(which) != ctypes.sizeof(cls):
            raise ImportError("%s: sizeof(%s) is %d in the library, %d in this binding" % (path, cls.__name__, sizeof(which), ctypes.sizeof(cls)))
    if reported != version:
        raise ImportError("%s reports version %d, this binding is written for %d: rebuild it" % (path, reported, version))
    return l


def lib():
    """The loaded libfldr_model.so, checked against this binding (struct sizes, header version); raises when it has not been built."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, _SIGNATURES, (Tensor, Config, IO), "fldr_model", MODEL_VERSION)
    return _lib


def _check(code, what):
    if code != 0:
        raise ModelError(what, code)


def padded_size(H, W, test_scales=5):
    div = (2 ** test_scales) * 8
    return (H + div - 1) // div * div, (W + div - 1) // div * div


class NativeModel:
    """A created fldr_model (weights and prepacks resident on `device`).  Read-only after creation: forwards on several streams,
    each with its own workspace, may run at once."""

    def __init__(self, handle, device, test_scales):
        self._h = handle
        self.device = torch.device("cuda", device)
        self.test_scales = test_scales

    @classmethod
    def from_npz(cls, path, device=0, test_scales=5):
        cfg = Config(int(device), int(test_scales))
        h = ctypes.c_void_p()
        _check(lib().fldr_model_create_npz(os.fsencode(path), ctypes.byref(cfg), ctypes.byref(h)), "fldr_model_create_npz")
        return cls(h, int(device), int(test_scales))

    @classmethod
    def from_tensors(cls, state, device=0, test_scales=5):
        """state: {name: tensor} (state-dict names; fp32 weights, fp64 EV8 / Mean8 / meanVec8 / T_param / z_alpha), any device."""
        keep, arr = [], (Tensor * len(state))()
        for i, (k, v) in enumerate(state.items()):
            v = v.detach().to("cpu").contiguous()
            if v.dtype not in (torch.float32, torch.float64) or v.dim() > 4:
                v = v.reshape(-1)[:0].float()                                   # passed on as a zero-size tensor: the library reports it
            name = k.encode()
            keep += [v, name]
            arr[i].name, arr[i].data = name, (v.data_ptr() or None)
            arr[i].dtype, arr[i].ndim = (F64 if v.dtype == torch.float64 else F32), v.dim()
            for d in range(v.dim()):
                arr[i].shape[d] = v.shape[d]
        cfg = Config(int(device), int(test_scales))
        h = ctypes.c_void_p()
        _check(lib().fldr_model_create(arr, len(state), ctypes.byref(cfg), ctypes.byref(h)), "fldr_model_create")
        return cls(h, int(device), int(test_scales))

    @classmethod
    def from_module(cls, model):
        """The weights of a loaded DCTXVFInet (fLDRnet.py) and its pyramid depth; the model's device."""
        p = next(model.parameters())
        dev = p.device.index if p.is_cuda else torch.cuda.current_device()
        return cls.from_tensors(dict(model.state_dict()), device=dev, test_scales=model.args.S_tst)

    def close(self):
        if self._h is not None and self._h.value:
            lib().fldr_model_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- workspace / plumbing -------------------------------------------------------------------------------------------------
    def workspace_bytes(self, H, W, n_t=1):
        n = lib().fldr_model_workspace_bytes(self._h, int(H), int(W), int(n_t))
        if n < 0:
            raise ModelError("fldr_model_workspace_bytes", int(n))
        return int(n)

    def workspace(self, H, W, n_t=1):
        return torch.empty(self.workspace_bytes(H, W, n_t), dtype=torch.uint8, device=self.device)

    def _t(self, t):
        t = torch.as_tensor(t, dtype=torch.float32)
        t = t.to(self.device).reshape(-1)
        return t.contiguous()

    def forward(self, io, ws, stream=None):
        """The raw call: io (an IO structure), ws (a byte tensor or None: allocated here for io's size), stream (torch.cuda.Stream or
        None: the current stream).  Returns the code without raising (tests of the error contract); 0 on success."""
        if ws is None:
            ws = self.workspace(io.H, io.W, max(io.n_t, 1))
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        return lib().fldr_model_forward(self._h, ctypes.byref(io), ctypes.c_void_p(ws.data_ptr()), ws.numel(), ctypes.c_void_p(st.cuda_stream))

    def _run(self, io, H, W, outs, ws, stream):
        ptrs = (ctypes.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        io.out = ctypes.cast(ptrs, ctypes.POINTER(ctypes.c_void_p))
        io.H, io.W = int(H), int(W)
        if ws is None:
            ws = self.workspace(H, W, io.n_t)
        _check(self.forward(io, ws, stream), "fldr_model_forward")

    # ---- forms ----------------------------------------------------------------------------------------------------------------
    def forward_pyramid(self, pyr, t, H=None, W=None, ws=None, stream=None, out=None):
        """pyr: DCTXVFInet's normInput (test_scales + 1 fp32 tensors [1,3,2,h_i,w_i] on the model's device); t: n_t values (a device
        tensor of n_t floats is used in place: a captured call reads it at replay).  H, W: the frame size (default: the padded size).
        -> fp64 [n_t,3,Hp,Wp] (`out` when given)."""
        Hp, Wp = pyr[0].shape[3], pyr[0].shape[4]
        H, W = int(H or Hp), int(W or Wp)
        if padded_size(H, W, self.test_scales) != (Hp, Wp) or len(pyr) != self.test_scales + 1:
            raise ValueError("pyramid of %d levels at %dx%d does not match a %dx%d frame at test_scales=%d" % (len(pyr), Hp, Wp, H, W, self.test_scales))
        tt = t if (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()) else self._t(t)
        n_t = tt.numel()
        if out is None:
            out = torch.empty(n_t, 3, Hp, Wp, dtype=torch.float64, device=self.device)
        io = IO()
        io.batch, io.input = 1, IN_PYRAMID
        for i, p in enumerate(pyr):
            assert p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.shape[0] == 1
            io.pyramid[i] = p.data_ptr()
        io.n_t, io.t, io.output = n_t, tt.data_ptr(), OUT_F64
        self._run(io, H, W, [out[k] for k in range(n_t)], ws, stream)
        return out

    def interpolate_u8(self, frames_u8=None, t=0.5, *, pair=None, order="bgr", out_layout="planar", out_order=None, ws=None, stream=None,
                       pyramid_out=None):
        """8-bit frames in, rounded 8-bit frames out.  Input: frames_u8 [1,2,3,H,W] (planar, as fldr_harness.interpolate_u8), or
        pair = (I0, I1): two [H,W,3] uint8 device tensors (rows may be `pitch` apart: any stride(0) >= 3W, stride(1) 3, stride(2) 1) in
        channel order `order`.  Output: out_layout "planar" -> [n_t,3,H,W] (BGR planes), "hwc" -> [n_t,H,W,3] in out_order (default: order).
        pyramid_out: optional list of fp32 tensors [1,3,2,Hp>>i,Wp>>i] that receive the ingested pyramid (normInput)."""
        tt = self._t(t)
        n_t = tt.numel()
        io = IO()
        io.batch = 1
        keep = []
        if pair is not None:
            a, b = pair
            H, W = a.shape[0], a.shape[1]
            for k, f in enumerate((a, b)):
                if not (f.is_cuda and f.dtype == torch.uint8 and tuple(f.shape) == (H, W, 3) and f.stride(2) == 1 and f.stride(1) == 3):
                    raise ValueError("pair frames must be uint8 [H,W,3] device tensors with interleaved pixels")
                io.frame[k], io.frame_pitch[k] = f.data_ptr(), f.stride(0)
            io.input, io.in_order = IN_U8_INTERLEAVED, ORDERS[order]
        else:
            B, T, C, H, W = frames_u8.shape
            if T != 2 or C != 3 or frames_u8.dtype != torch.uint8:
                raise ValueError("frames_u8 must be uint8 [1,2,3,H,W]")
            f = frames_u8.contiguous()
            keep.append(f)
            io.input, io.frames_u8 = IN_U8_PLANAR, f.data_ptr()
            io.batch = B                                                     # != 1: the library refuses it (FLDR_MODEL_E_BATCH)
        io.n_t, io.t = n_t, tt.data_ptr()
        for i, p in enumerate(pyramid_out or []):
            assert p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()
            io.pyramid[i] = p.data_ptr()
        if out_layout == "planar":
            out = torch.empty(n_t, 3, H, W, dtype=torch.uint8, device=self.device)
            io.output = OUT_U8_PLANAR
        elif out_layout == "hwc":
            out = torch.empty(n_t, H, W, 3, dtype=torch.uint8, device=self.device)
            io.output, io.out_pitch = OUT_U8_INTERLEAVED, 3 * W
            io.out_order = ORDERS[out_order or order]
        else:
            raise ValueError("out_layout must be 'planar' or 'hwc'")
        self._run(io, H, W, [out[k] for k in range(n_t)], ws, stream)
        return out

    def interpolate_u10(self, frames, t=0.5, *, out="u10", ws=None, stream=None, pyramid_out=None):
        """The 10-bit forms.  frames: uint16 [1,2,3,H,W] with code values 0 .. 1023 (FLDR_MODEL_IN_U10_PLANAR), or uint8 [1,2,3,H,W]
        (8-bit in, 10-bit out).  out: "u10" -> uint16 [n_t,3,H,W] (FLDR_MODEL_OUT_U10_PLANAR), "u8" -> uint8 [n_t,3,H,W], "f64" -> the
        fp64 frames [n_t,3,Hp,Wp].  pyramid_out as interpolate_u8."""
        tt = t if (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()) else self._t(t)
        n_t = tt.numel()
        B, T, C, H, W = frames.shape
        if T != 2 or C != 3 or frames.dtype not in (torch.uint16, torch.uint8):
            raise ValueError("frames must be uint16 or uint8 [1,2,3,H,W]")
        f = frames.contiguous()
        io = IO()
        io.batch, io.input, io.frames_u8 = B, (IN_U10_PLANAR if f.dtype == torch.uint16 else IN_U8_PLANAR), f.data_ptr()
        io.n_t, io.t = n_t, tt.data_ptr()
        for i, p in enumerate(pyramid_out or []):
            assert p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()
            io.pyramid[i] = p.data_ptr()
        if out == "u10":
            res = torch.empty(n_t, 3, H, W, dtype=torch.uint16, device=self.device)
            io.output = OUT_U10_PLANAR
        elif out == "u8":
            res = torch.empty(n_t, 3, H, W, dtype=torch.uint8, device=self.device)
            io.output = OUT_U8_PLANAR
        elif out == "f64":
            Hp, Wp = padded_size(H, W, self.test_scales)
            res = torch.empty(n_t, 3, Hp, Wp, dtype=torch.float64, device=self.device)
            io.output = OUT_F64
        else:
            raise ValueError("out must be 'u10', 'u8' or 'f64'")
        self._run(io, H, W, [res[k] for k in range(n_t)], ws, stream)
        return res

    def interpolate_multi(self, frames, t_values, pyramid=None, ws=None, stream=None):
        """fldr_harness.interpolate_multi through one native call: frames [1,3,2,H,W] in [-1,1] on the model's device (pyramid built
        as the harness builds it, unless given) -> list of fp64 frames [1,3,H,W] (views of one [n_t,3,Hp,Wp] tensor)."""
        import fldr_harness as Hn
        B, C, T, H, W = frames.shape
        if pyramid is None:
            with torch.no_grad():
                pyramid = Hn.build_pyramid(Hn.pad_frames(frames, Hn.args_config(test_scales=self.test_scales)),
                                           Hn.args_config(test_scales=self.test_scales))
        out = self.forward_pyramid(pyramid, list(t_values), H, W, ws=ws, stream=stream)
        return [out[k:k + 1, :, :H, :W] for k in range(out.shape[0])]
