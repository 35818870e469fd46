"""CPU checks of the interlace API (include/fldr_interlace.h, libfldr_interlace.so): the library's symbol table and link, the header as
plain C99 / C++, the C example, the code-generation guard, the binding's struct mirrors, the argument checks of the three layers — which
happen before any device call, so they run without a GPU —, the schedule against a brute-force statement in fractions, and the oracle
(tests/interlace_oracle.py) alone on hand-worked planes."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import interlace_oracle as O
from lib_checks import declared as _declared, syms as _syms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fldr-vfi_amd")
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "fldr_interlace.h")
LIB = os.path.join(PKG, "libfldr_interlace.so")
EXAMPLE = os.path.join(ROOT, "examples", "fldr_interlace.c")
BARRED = ("fldr_field", "fldr_chroma", "fldr_cadence", "fldr_repeat", "fldr_pipe", "fldr_pulldown", "fldr_probe")
NAMES = ("version", "error_string", "sizeof", "weave", "workspace_bytes", "field_frame", "scene_state", "forward", "plan", "create", "max_out", "push",
         "flush", "reset", "destroy")


# ---- the library ------------------------------------------------------------------------------------------------------------------------
def test_library_exports_exactly_the_header():
    """The functions the issue names: the nine of every stream library, the weave, the forward with its three companions, and the plan."""
    declared = _declared(HDR, "FLDR_INTERLACE_API")
    assert declared == set("fldr_interlace_" + n for n in NAMES), sorted(declared)
    assert _syms(LIB, ["--defined-only"]) == declared
    import fldr_interlace
    assert set(fldr_interlace.EXPORTS) == declared


def test_library_links_only_the_rate_video_and_model_apis():
    dyn = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    needed = set(re.findall(r"NEEDED.*\[(libfldr_\w+\.so)\]", dyn))
    assert needed == {"libfldr_rate.so", "libfldr_video.so"}, dyn
    assert re.search(r"R(UN)?PATH.*\[\$ORIGIN\b", dyn), dyn
    used = set(n for n in _syms(LIB, ["--undefined-only"]) if n.startswith("fldr_"))
    allowed = (_declared(os.path.join(INC, "fldr_rate.h"), "FLDR_RATE_API") | _declared(os.path.join(INC, "fldr_video.h"), "FLDR_VIDEO_API") |
               _declared(os.path.join(INC, "fldr_model.h"), "FLDR_MODEL_API"))
    assert used and used <= allowed, sorted(used)
    assert {"fldr_rate_forward", "fldr_video_forward", "fldr_rate_workspace_bytes", "fldr_rate_error_string"} <= used
    assert not used & {"fldr_rate_create", "fldr_rate_push", "fldr_rate_flush"}          # the stream is this library's own: it holds fields, not frames


def test_header_and_library_name_none_of_the_libraries_beside_them():
    text = open(HDR).read().lower()
    raw = open(LIB, "rb").read().lower()
    for other in BARRED:
        assert other not in text and other.encode() not in raw, other
    for name in os.listdir(INC):
        if name != "fldr_interlace.h":
            assert "fldr_interlace" not in open(os.path.join(INC, name)).read().lower(), name
    for name in os.listdir(PKG):
        if re.fullmatch(r"libfldr_\w+\.so", name) and name != "libfldr_interlace.so":
            assert b"fldr_interlace" not in open(os.path.join(PKG, name), "rb").read(), name


@pytest.mark.parametrize("compiler", [["gcc", "-std=c99", "-x", "c"], ["g++", "-std=c++11", "-x", "c++"]])
def test_header_is_plain_c99_and_cxx(compiler, tmp_path):
    assert shutil.which(compiler[0]), compiler[0] + " not installed"
    src = tmp_path / "h.c"
    src.write_text('#include <stddef.h>\n#include "fldr_interlace.h"\nint main(void) { fldr_interlace_config c; fldr_interlace_report r; fldr_interlace_io io;\n'
                   '  fldr_interlace_schedule s; c.tff = 1; r.held = 0; io.filter = FLDR_INTERLACE_COMPLEX; s.B = 5;\n'
                   '  return fldr_interlace_sizeof(1) == (int)sizeof(c) && c.tff == 1 && r.held == 0 && io.filter == 2 && s.B == 5 &&\n'
                   '         FLDR_INTERLACE_NONE == 0 && FLDR_INTERLACE_LINEAR == 1 && sizeof(fldr_interlace_report) == 64 &&\n'
                   '         sizeof(fldr_interlace_schedule) == 72 && offsetof(fldr_interlace_config, tff) == sizeof(fldr_rate_config) ? 0 : 1; }\n')
    r = subprocess.run(compiler + ["-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I" + INC, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "hip" not in re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S).lower()


def test_header_defines_no_error_code_and_says_whose_it_returns():
    text = open(HDR).read()
    assert not re.findall(r"#define\s+FLDR_[A-Z0-9]+_E_[A-Z]+", text)
    for s in ("defines no code of its own", "FLDR_RATE_E_ARG", "FLDR_RATE_E_STATE", "FLDR_RATE_E_RATIO", "FLDR_RATE_E_DEVICE",
              "fldr_interlace_error_string is fldr_rate_error_string"):
        assert s in text, s
    import fldr_interlace as K
    import fldr_rate as R
    l = K.lib()
    for code in (R.E_ARG, R.E_STATE, R.E_RATIO, R.E_DEVICE, -101, -3, 0, -999):
        assert l.fldr_interlace_error_string(code) == R.lib().fldr_rate_error_string(code)
    assert (K.E_ARG, K.E_STATE, K.E_RATIO, K.E_DEVICE) == (R.E_ARG, R.E_STATE, R.E_RATIO, R.E_DEVICE)


def test_header_states_the_rule_the_siting_the_limit_and_what_is_out_of_scope():
    text = open(HDR).read()
    for s in ("(s(y-1) + 2 s(y) + s(y+1) + 2) >> 2", "-s(y-2) + 2 s(y-1) + 6 s(y) + 2 s(y+1) - s(y+2) + 4) >> 3", "NEVER\n *    WRITTEN",
              "4j + 0.5", "4j + 2.5", "no quarter-line error", "4294967296", "2147483647", "not motion-adaptive", "the stream is synchronous",
              "one weave launch per field", "delivered woven only", "4:2:2, packed and RGB formats are out of scope",
              "no threshold is introduced here", "Checked in this order", "Validation order"):
        assert s in text, s


def test_example_builds_with_cc(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    exe = tmp_path / "fldr_interlace"
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + INC, "-o", str(exe), EXAMPLE, "-L" + PKG,
                        "-l:libfldr_interlace.so", "-l:libfldr_rate.so", "-l:libfldr_video.so", "-l:libfldr_model.so", "-Wl,-rpath," + PKG],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    src = open(EXAMPLE).read()
    assert "hip" not in re.sub(r"/\*.*?\*/", "", src, flags=re.S).lower()
    u = subprocess.run([str(exe)], capture_output=True, text=True)            # no arguments: usage, no device touched
    assert u.returncode == 2 and "usage" in u.stderr and "filter=none|linear|complex" in u.stderr and "scene=0|1" in u.stderr and "bff" in u.stderr
    for bad in (["w.npz", "64", "64", "24", "30", "in.yuv"],                  # no output
                ["w.npz", "66", "64", "24", "30", "in.yuv", "out.yuv"],       # H not a multiple of 4
                ["w.npz", "64", "1", "24", "30", "in.yuv", "out.yuv"],
                ["w.npz", "64", "64", "24/0", "30", "in.yuv", "out.yuv"],
                ["w.npz", "64", "64", "24", "x", "in.yuv", "out.yuv"],
                ["w.npz", "64", "64", "1", "100", "in.yuv", "out.yuv"],       # 200 fields per frame: a ratio the converter does not take
                ["w.npz", "64", "64", "24", "30", "in.yuv", "out.yuv", "filter=sharp"],
                ["w.npz", "64", "64", "24", "30", "in.yuv", "out.yuv", "scene=2"],
                ["w.npz", "64", "64", "24", "30", "in.yuv", "out.yuv", "tff"],
                ["-", "64", "64", "24", "30", "in.yuv", "out.yuv"]):          # fields to interpolate and no weights
        u = subprocess.run([str(exe)] + bad, capture_output=True, text=True)
        assert u.returncode == 2 and "usage" in u.stderr, bad


def test_no_unsafe_packed_fp32_in_the_interlace_library():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_pk_opsel.py"), LIB], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    ks = KR.kernels(LIB)
    assert len(ks) == 9, [k["name"] for k in ks]          # three sample forms x three filters; wide and per-sample access in each
    for k in ks:
        assert "interlace_weave_kernel" in k["name"], k["name"]
        assert k.get("scratch", -1) == 0 and k.get("vgpr_spills", -1) == 0 and k.get("sgpr_spills", -1) == 0 and k.get("lds", 0) == 0, k


def test_binding_struct_sizes_and_version():
    import fldr_interlace as K
    l = K.lib()
    text = open(HDR).read()
    assert l.fldr_interlace_version() == K.INTERLACE_VERSION == int(re.search(r"#define FLDR_INTERLACE_VERSION (\d+)", text).group(1)) == 100
    for which, cls in enumerate((K.InterlaceIO, K.InterlaceConfig, K.Schedule, K.Report)):
        assert l.fldr_interlace_sizeof(which) == ctypes.sizeof(cls)
    assert ctypes.sizeof(K.Report) == 64 and ctypes.sizeof(K.Schedule) == 72 and ctypes.sizeof(K.InterlaceConfig) == ctypes.sizeof(K.RateConfig) + 24
    assert l.fldr_interlace_sizeof(4) == K.E_ARG and l.fldr_interlace_sizeof(-1) == K.E_ARG
    for macro, v in (("FLDR_INTERLACE_NONE", K.NONE), ("FLDR_INTERLACE_LINEAR", K.LINEAR), ("FLDR_INTERLACE_COMPLEX", K.COMPLEX)):
        assert int(re.search(r"#define %s\s+(\d+)" % macro, text).group(1)) == v, macro
    assert (K.NONE, K.LINEAR, K.COMPLEX) == (O.NONE, O.LINEAR, O.COMPLEX)


# ---- argument errors without a device ---------------------------------------------------------------------------------------------------
H0 = W0 = 64


def _host(V, layout, depth, H=H0, W=W0, count=4):
    """`count` frames whose planes all point into one zeroed, 256-byte aligned host buffer, each frame in a part of its own."""
    b = 2 if depth == 10 else 1
    part = H * W * 2 * b
    buf = np.zeros(count * part + 512, np.uint8)
    base = (buf.ctypes.data + 255) // 256 * 256
    frames = []
    for k in range(count):
        f = V.Frame()
        off = base + k * part
        for p, (r, c) in enumerate(V.plane_shapes(layout, H, W)):
            f.plane[p], f.pitch[p] = off, c * b
            off += r * c * b
        frames.append(f)
    return buf, base, frames


@pytest.mark.parametrize("layout", ["nv12", "i420"])
@pytest.mark.parametrize("depth", [8, 10])
def test_weave_argument_errors_before_any_device_call(layout, depth):
    import fldr_interlace as K
    import fldr_video as V
    b = 2 if depth == 10 else 1
    buf, base, _ = _host(V, layout, depth)
    shapes = V.plane_shapes(layout, H0, W0)

    def call(mutate=lambda fr, fmt: None, H=H0, W=W0, filter=0, which=2, use=(True, True, True)):
        _, _, fr = _host(V, layout, depth)
        fmt = V.Format(layout, depth=depth)
        mutate(fr[which], fmt)
        fr = [f if u else None for f, u in zip(fr, use)]
        return K.weave_raw(H, W, fmt, fr[0], fr[1], filter, fr[2], None)
    bad_format = lambda fr, fmt: setattr(fmt, "layout", 2)
    # every argument error comes before the format, so a call that is otherwise valid is shown to pass them by reaching it
    assert call(bad_format) == V.E_FORMAT
    for H in (0, 2, 6, 62, 66, -4):
        assert call(H=H) == K.E_ARG and call(bad_format, H=H) == K.E_ARG, H
    assert call(W=0) == K.E_ARG and call(W=-1) == K.E_ARG
    assert call(filter=3) == K.E_ARG and call(filter=-1) == K.E_ARG and call(bad_format, filter=3) == K.E_ARG
    assert call(use=(False, False, True)) == K.E_ARG and call(bad_format, use=(False, False, True)) == K.E_ARG      # both sources NULL
    assert call(use=(True, True, False)) == K.E_ARG
    assert K.weave_raw(H0, W0, None, None, None, 0, None, None) == K.E_ARG
    for f in (0, 1, 2):
        assert call(bad_format, filter=f, use=(True, False, True)) == V.E_FORMAT and call(bad_format, filter=f, use=(False, True, True)) == V.E_FORMAT
    for field, val in (("layout", 2), ("matrix", 2), ("range", -1), ("depth", 9), ("depth", 12)):
        assert call(lambda fr, fmt: setattr(fmt, field, val)) == V.E_FORMAT, field
    assert call(lambda fr, fmt: fmt.reserved.__setitem__(3, 1)) == V.E_FORMAT
    # then planes, then pitches, of even, odd, out
    for which in range(3):
        for q in range(len(shapes)):
            assert call(lambda fr, fmt: fr.plane.__setitem__(q, None), which=which) == V.E_PLANE, (which, q)
            assert call(lambda fr, fmt: fr.pitch.__setitem__(q, shapes[q][1] * b - b), which=which) == V.E_PITCH, (which, q)
            if depth == 10:
                assert call(lambda fr, fmt: fr.plane.__setitem__(q, base + 1), which=which) == V.E_PLANE, (which, q)
                assert call(lambda fr, fmt: fr.pitch.__setitem__(q, shapes[q][1] * b + 1), which=which) == V.E_PITCH, (which, q)
    _, _, fr = _host(V, layout, depth)
    fr[0].pitch[0] = 2
    fr[2].plane[1] = None                                                   # a missing plane of out before a short pitch of even
    assert K.weave_raw(H0, W0, V.Format(layout, depth=depth), fr[0], fr[1], 0, fr[2], None) == V.E_PLANE
    # last: the frame-size limit, and out overlapping a source — the whole frame, the last byte of a plane
    fmt = V.Format(layout, depth=depth)
    _, _, fr = _host(V, layout, depth)
    big = 2 ** 20                                                           # 65536 groups (or twice that) in a row: g x g x R is beyond 2^32
    for f in fr:
        for q in range(3):
            f.pitch[q] = big * 2 * b
    assert K.weave_raw(4, big, fmt, fr[0], fr[1], 0, fr[2], None) == K.E_ARG
    for k in range(2):
        _, _, fr = _host(V, layout, depth)
        assert K.weave_raw(H0, W0, fmt, fr[0], fr[1], 1, fr[k], None) == K.E_ARG, k
        _, _, fr = _host(V, layout, depth)
        fr[2].plane[1] = fr[k].plane[0] + H0 * W0 * b - b
        assert K.weave_raw(H0, W0, fmt, fr[0], fr[1], 2, fr[2], None) == K.E_ARG, k
    assert not buf.any()


def _io(K, V, layout, depth, n_t=2, H=H0, W=W0):
    buf, base, fr = _host(V, layout, depth, H, W, count=6)
    io = K.InterlaceIO()
    io.pair.H, io.pair.W = H, W
    io.pair.in_format = V.Format(layout, depth=depth)
    io.pair.out_format = V.Format(layout, depth=depth)
    io.pair.in_[0], io.pair.in_[1] = fr[0], fr[1]
    outs = (V.Frame * n_t)(*fr[2:2 + n_t])
    par = (ctypes.c_int32 * n_t)(*[k & 1 for k in range(n_t)])
    io.pair.n_t, io.pair.t, io.pair.out = n_t, base, ctypes.cast(outs, ctypes.POINTER(V.Frame))
    io.parity = ctypes.cast(par, ctypes.POINTER(ctypes.c_int32))
    io.filter, io.scene = 1, 1
    io._keep = (buf, outs, par)
    return io, buf, base, outs, par


@pytest.mark.parametrize("layout,depth", [("nv12", 8), ("i420", 10)])
def test_forward_argument_errors_before_any_device_call(layout, depth):
    """Without a model every otherwise valid call ends at the null model (E_ARG), which comes after the formats and frames: a bad format
    or frame that is reported shows that everything before it passed."""
    import fldr_interlace as K
    import fldr_rate as R
    import fldr_video as V
    l = K.lib()

    def call(mutate=lambda io, outs, par: None, **kw):
        io, buf, base, outs, par = _io(K, V, layout, depth, **kw)
        mutate(io, outs, par)
        rc = l.fldr_interlace_forward(None, ctypes.byref(io), ctypes.c_void_p(base), 1 << 40, None)
        assert not buf.any()
        return rc
    bad_format = lambda io: setattr(io.pair.in_format, "layout", 2)
    assert l.fldr_interlace_forward(None, None, None, 0, None) == K.E_ARG
    assert call() == K.E_ARG                                                 # valid, no model
    assert call(lambda io, o, p: bad_format(io)) == V.E_FORMAT               # ... and what comes before the model is seen through this
    for H in (0, 2, 6, 66):
        assert call(lambda io, o, p: (bad_format(io), setattr(io.pair, "H", H))) == K.E_ARG, H
    assert call(lambda io, o, p: (bad_format(io), setattr(io.pair, "W", 0))) == K.E_ARG
    for n_t in (0, -1, 65):
        assert call(lambda io, o, p: (bad_format(io), setattr(io.pair, "n_t", n_t))) == K.E_ARG, n_t
    assert call(lambda io, o, p: (bad_format(io), setattr(io.pair, "t", None))) == K.E_ARG
    assert call(lambda io, o, p: (bad_format(io), setattr(io.pair, "out", ctypes.POINTER(V.Frame)()))) == K.E_ARG
    assert call(lambda io, o, p: (bad_format(io), setattr(io, "parity", ctypes.POINTER(ctypes.c_int32)()))) == K.E_ARG
    for f in (-1, 3):
        assert call(lambda io, o, p: (bad_format(io), setattr(io, "filter", f))) == K.E_ARG, f
    for s in (-1, 2):
        assert call(lambda io, o, p: (bad_format(io), setattr(io, "scene", s))) == K.E_ARG, s
    for i in range(4):
        assert call(lambda io, o, p: (bad_format(io), io.reserved.__setitem__(i, 1))) == K.E_ARG, i
    for k in range(2):
        assert call(lambda io, o, p: (bad_format(io), p.__setitem__(k, 2))) == K.E_ARG and call(lambda io, o, p: (bad_format(io), p.__setitem__(k, -1))) == K.E_ARG
    assert call(lambda io, o, p: (bad_format(io), setattr(io.scene_params, "sad_permille", 1001))) == K.E_ARG
    assert call(lambda io, o, p: (bad_format(io), io.scene_params.reserved.__setitem__(1, 1))) == K.E_ARG
    for f in (0, 1, 2):
        for s in (0, 1):
            assert call(lambda io, o, p: (bad_format(io), setattr(io, "filter", f), setattr(io, "scene", s))) == V.E_FORMAT
    # the formats: each checked, then compared
    assert call(lambda io, o, p: setattr(io.pair.out_format, "depth", 9)) == V.E_FORMAT
    assert call(lambda io, o, p: setattr(io.pair.out_format, "depth", 18 - depth)) == R.E_FORMAT
    assert call(lambda io, o, p: setattr(io.pair.out_format, "layout", 1 - io.pair.in_format.layout)) == R.E_FORMAT
    # planes, then pitches, of in[0], in[1] and every out[k]
    assert call(lambda io, o, p: io.pair.in_[1].plane.__setitem__(1, None)) == V.E_PLANE
    assert call(lambda io, o, p: io.pair.in_[0].pitch.__setitem__(0, 2)) == V.E_PITCH
    assert call(lambda io, o, p: o[1].plane.__setitem__(0, None)) == V.E_PLANE
    assert call(lambda io, o, p: o[1].pitch.__setitem__(1, 2)) == V.E_PITCH
    assert call(lambda io, o, p: (io.pair.in_[0].pitch.__setitem__(0, 2), o[1].plane.__setitem__(1, None))) == V.E_PLANE
    assert l.fldr_interlace_workspace_bytes(None, 6, 64, 1) == K.E_ARG and l.fldr_interlace_workspace_bytes(None, 64, 64, 0) == K.E_ARG
    assert l.fldr_interlace_workspace_bytes(None, 64, 64, 65) == K.E_ARG and l.fldr_interlace_workspace_bytes(None, 64, 64, 1) < 0
    fr = V.Frame()
    assert l.fldr_interlace_field_frame(None, 64, 64, None, 1, 0, None, ctypes.byref(fr)) == K.E_ARG
    fmt = V.Format(layout, depth=depth)
    assert l.fldr_interlace_field_frame(None, 64, 64, ctypes.byref(fmt), 2, 2, None, ctypes.byref(fr)) == K.E_ARG
    assert l.fldr_interlace_field_frame(None, 64, 64, ctypes.byref(fmt), 2, -1, None, ctypes.byref(fr)) == K.E_ARG
    assert l.fldr_interlace_scene_state(None, 64, 64, 1, None) is None


def _create(l, h, model=None, **kw):
    import fldr_interlace as K
    import fldr_video as V
    cfg = K.make_config(64, 64, V.Format("i420"), 24, 30)
    for k, v in kw.items():
        if k == "mutate":
            v(cfg)
        elif k in ("tff", "filter"):
            setattr(cfg, k, v)
        else:
            setattr(cfg.rate, k, v)
    return l.fldr_interlace_create(model, ctypes.byref(cfg), ctypes.byref(h))


def test_stream_argument_errors_before_any_device_call():
    import fldr_interlace as K
    import fldr_rate as R
    import fldr_video as V
    l = K.lib()
    h = ctypes.c_void_p()
    create = lambda **kw: _create(l, h, **kw)
    ratio_bad = dict(in_num=1, in_den=1, out_num=33, out_den=1)              # 66 fields per pushed frame: one too many at the doubled rate
    assert create() == K.E_ARG                                               # valid (24 -> 30i: B = 5), no model
    assert create(**ratio_bad) == R.E_RATIO                                  # ... and what comes before the model is seen through this
    assert create(in_num=1, in_den=1, out_num=32, out_den=1) == K.E_ARG      # 64 fields per frame is what fldr_rate_create takes at 1 -> 64
    # fldr_rate_create's checks with its codes, in its order
    assert create(H=1) == R.E_ARG and create(device=-1) == R.E_ARG and create(scene=2) == R.E_ARG
    assert create(mutate=lambda c: c.rate.reserved.__setitem__(2, 1)) == R.E_ARG
    assert create(mutate=lambda c: setattr(c.rate.scene_params, "sad_permille", 1001)) == R.E_ARG
    assert create(mutate=lambda c: setattr(c.rate.format, "layout", 3)) == V.E_FORMAT
    for term in ("in_num", "in_den", "out_num", "out_den"):
        assert create(**{term: 0}) == R.E_RATIO and create(**{term: -24}) == R.E_RATIO, term
    assert create(mutate=lambda c: setattr(c.rate.format, "layout", 3), tff=2) == V.E_FORMAT
    assert create(in_num=0, tff=2) == R.E_RATIO and create(in_num=0, H=66) == R.E_RATIO
    # this library's, all before the ratio: H a multiple of 4, tff, filter, the reserved words
    for H in (2, 6, 62, 66):
        assert create(H=H, **ratio_bad) == K.E_ARG, H
    for field, bad in (("tff", 2), ("tff", -1), ("filter", 3), ("filter", -1)):
        assert create(**dict(ratio_bad, **{field: bad})) == K.E_ARG, field
    for i in range(4):
        assert create(mutate=lambda c: c.reserved.__setitem__(i, 1), **ratio_bad) == K.E_ARG
    assert create(tff=0, filter=2, **ratio_bad) == R.E_RATIO
    # the ratio: out_num above 2^30, reduced terms above 2^24 at the doubled rate
    assert create(in_num=2 ** 31 - 1, in_den=1, out_num=2 ** 30 + 1, out_den=1) == R.E_RATIO
    assert create(in_num=2 ** 25 + 1, in_den=1, out_num=2 ** 24, out_den=1) == R.E_RATIO
    assert create(in_num=2 ** 30, in_den=1, out_num=2 ** 30, out_den=1) == K.E_ARG       # 1 / 2: allowed, and then no model
    # a NULL model is an argument error exactly where a field is interpolated (B != 1)
    assert create(in_num=25, out_num=25) == K.E_ARG and create(in_num=60, out_num=25) == K.E_ARG
    assert l.fldr_interlace_create(None, None, ctypes.byref(h)) == K.E_ARG
    n = ctypes.c_int()
    assert l.fldr_interlace_push(None, None, None, ctypes.byref(n), None) == K.E_ARG
    assert l.fldr_interlace_flush(None, None, ctypes.byref(n), None) == K.E_ARG
    assert l.fldr_interlace_reset(None) == K.E_ARG
    assert l.fldr_interlace_max_out(None) == K.E_ARG
    l.fldr_interlace_destroy(None)


def test_plan_argument_errors():
    import fldr_interlace as K
    import fldr_video as V
    cfg = lambda **kw: K.make_config(0, 0, V.Format(), kw.pop("in_rate", 24), kw.pop("out_rate", 30), **kw)     # H, W, format are not looked at
    assert K.plan_raw(cfg(), 0)[0] == 0 and K.plan_raw(cfg(), 2 ** 36)[0] == 0
    assert K.plan_raw(cfg(), -1)[0] == K.E_ARG and K.plan_raw(cfg(), 2 ** 36 + 1)[0] == K.E_ARG
    assert K.plan_raw(None, 0)[0] == K.E_ARG and K.lib().fldr_interlace_plan(ctypes.byref(cfg()), 0, None) == K.E_ARG
    c = cfg()
    c.tff = 2
    assert K.plan_raw(c, 0)[0] == K.E_ARG
    c = cfg()
    c.filter = 3
    assert K.plan_raw(c, 0)[0] == K.E_ARG
    c = cfg()
    c.reserved[0] = 1
    assert K.plan_raw(c, 0)[0] == K.E_ARG
    c = cfg()
    c.rate.in_den = 0
    assert K.plan_raw(c, 0)[0] == K.E_RATIO
    assert K.plan_raw(cfg(in_rate=1, out_rate=33), 0)[0] == K.E_RATIO and K.plan_raw(cfg(in_rate=1, out_rate=32), 0)[0] == 0
    assert K.plan_raw(cfg(in_rate=2 ** 31 - 1, out_rate=2 ** 30 + 1), 0)[0] == K.E_RATIO


# ---- the schedule -------------------------------------------------------------------------------------------------------------------------
CONVERSIONS = [(24, 30, 2, 5), ((24000, 1001), (30000, 1001), 2, 5), (25, 25, 1, 2), (50, 25, 1, 1), (60, 25, 6, 5), (24, 25, 12, 25), (120, 25, 12, 5),
               ((60000, 1001), (30000, 1001), 1, 1), (30, 25, 3, 5), (24, (30000, 1001), 1001, 2500),
               (2 ** 30, 2 ** 30, 1, 2)]                                     # the doubled rate is 2^31: no int32


def _frac(r):
    return Fraction(*r) if isinstance(r, tuple) else Fraction(r)


@pytest.mark.parametrize("in_rate,out_rate,A,B", CONVERSIONS)
@pytest.mark.parametrize("tff", [True, False])
def test_plan_and_max_out_against_fractions(in_rate, out_rate, A, B, tff):
    import fldr_interlace as K
    step = _frac(in_rate) / (2 * _frac(out_rate))
    assert (step.numerator, step.denominator) == (A, B) and O.field_step(in_rate, out_rate) == step
    for k in list(range(40)) + [10 ** 6 + 7, 2 ** 36]:
        s = K.plan(k, in_rate, out_rate, tff)
        assert s == O.plan(k, in_rate, out_rate, tff), k
        assert s["B"] == B and s["frame"] == k and s["parity"] == ([0, 1] if tff else [1, 0])
        for f in range(2):
            assert Fraction(s["input"][f]) + Fraction(s["r"][f], B) == (2 * k + f) * step and 0 <= s["r"][f] < B
        assert s["push"] == s["input"][1] + 1
    assert O.max_out(in_rate, out_rate) == (-(-B // A) + 1) // 2


def _returned_by_plan(n_frames, in_rate, out_rate):
    """What the pushes return by the library's plan: frame k at push plan(k).push where that push exists."""
    import fldr_interlace as K
    per = [[] for _ in range(n_frames)]
    k = 0
    while True:
        p = K.plan(k, in_rate, out_rate)["push"]
        if p >= n_frames:
            return per
        per[p].append(k)
        k += 1


@pytest.mark.parametrize("in_rate,out_rate,A,B", CONVERSIONS)
def test_frames_per_push_by_brute_force(in_rate, out_rate, A, B):
    n = 26
    brute = O.stream_frames(n, in_rate, out_rate)
    per = [[k for k, held in p] for p in brute[:n]]
    assert per == _returned_by_plan(n, in_rate, out_rate)
    assert [k for p in brute for k, _ in p] == list(range(sum(len(p) for p in brute)))       # every frame once, in order
    assert max(len(p) for p in per) <= O.max_out(in_rate, out_rate) and all(not held for p in brute[:n] for _, held in p)
    assert len(brute[n]) <= 1
    counts = [len(p) for p in per]
    if (A, B) == (2, 5):
        assert counts[:11] == [0, 1, 1, 2, 1, 1, 1, 2, 1, 1, 1] and 2 in counts and O.max_out(in_rate, out_rate) == 2
    elif (A, B) == (1, 2):
        assert counts == [0] + [1] * (n - 1)
    elif (A, B) == (1, 1):
        assert counts[:6] == [0, 0, 1, 0, 1, 0] and O.max_out(in_rate, out_rate) == 1
    elif (A, B) == (12, 25):
        assert max(counts) == 2 == O.max_out(in_rate, out_rate)
    elif (A, B) in ((6, 5), (12, 5)):
        assert max(counts) == 1 == O.max_out(in_rate, out_rate) and 0 in counts[1:]
    # the flush: a frame left with its first field only is completed and marked held
    for m in range(1, 9):
        last = O.stream_frames(m, in_rate, out_rate)[m]
        fields = sum(1 for f in range(m * B + 1) if f * A <= (m - 1) * B)                        # the fields at or before the last frame
        assert [held for _, held in last] == ([True] if fields % 2 else [False] if (fields - 1) * A == (m - 1) * B else [])


# ---- the oracle alone ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,depth", [("nv12", 8), ("i420", 8), ("nv12", 10), ("i420", 10)])
def test_oracle_flat_planes_stay_flat_and_none_is_the_identity(layout, depth):
    mx = 1023 if depth == 10 else 255
    for v in (0, 1, mx // 2, mx - 1, mx):
        word = (v << 6) if (layout, depth) == ("nv12", 10) else v
        flat = (np.full((8, 6), word, np.uint16 if depth == 10 else np.uint8),)
        for filt in (O.LINEAR, O.COMPLEX, O.NONE):
            assert np.array_equal(O.weave(flat, flat, layout, depth, filt)[0], flat[0]), (v, filt)
    g = np.random.default_rng(3)
    f = (g.integers(0, 65536 if depth == 10 else 256, (8, 5)).astype(np.uint16 if depth == 10 else np.uint8),)
    assert np.array_equal(O.weave(f, f, layout, depth, O.NONE)[0], f[0])                      # dirty bits and all
    e, o = (np.zeros_like(f[0]),), (np.ones_like(f[0]),)
    w = O.weave(e, o, layout, depth, O.NONE)[0]
    assert not w[0::2].any() and (w[1::2] == 1).all()
    keep = (np.full_like(f[0], 7),)
    w = O.weave(None, o, layout, depth, O.NONE, out=keep)[0]
    assert (w[0::2] == 7).all() and (w[1::2] == 1).all() and (keep[0] == 7).all()              # the absent parity is left as it is


def test_oracle_hand_worked_rows():
    y = np.zeros((12, 2), np.uint8)
    y[5] = 255
    lin = O.weave((y,), (y,), "nv12", 8, O.LINEAR)[0][:, 0].tolist()
    assert lin[3:8] == [0, 64, 128, 64, 0] and sum(lin) == 256
    cpx = O.weave((y,), (y,), "nv12", 8, O.COMPLEX)[0][:, 0].tolist()
    assert cpx[2:9] == [0, 0, 64, 191, 64, 0, 0]
    # the outer zeros are floor((-255 + 4) / 8) = -32 before the clamp: floor, not truncation (-31), then the clamp
    assert (-255 + 4) >> 3 == -32 and int(np.int64(-251) >> 3) == -32
    # a 0 -> mx step: the row behind the edge overshoots, (9 mx + 4) >> 3 > mx, and is clamped; the row before it undershoots
    for layout, depth, mx in (("nv12", 8, 255), ("i420", 10, 1023), ("nv12", 10, 1023)):
        sh = 6 if (layout, depth) == ("nv12", 10) else 0
        s = np.zeros((12, 1), np.uint16 if depth == 10 else np.uint8)
        s[6:] = mx << sh
        assert (9 * mx + 4) >> 3 > mx
        out = (O.weave((s,), (s,), layout, depth, O.COMPLEX)[0][:, 0] >> sh).tolist()
        # row 4 sees -s(6) alone: (-mx + 4) >> 3, negative, clamped to 0; row 5: (2 - 1) mx; row 6: (6 + 2 - 1) mx; row 7: (2 + 6 + 2 - 1) mx,
        # clamped; row 8: 8 mx
        assert (-mx + 4) >> 3 < 0 and out[3:5] == [0, 0] and out[5] == (mx + 4) >> 3 and out[6] == (7 * mx + 4) >> 3 and out[7:9] == [mx, mx]
    # the plane's edges: rows clamp, so a bright first row stays brighter than (1 2 1) of a zero-padded plane would leave it
    e = np.zeros((4, 1), np.uint8)
    e[0] = 200
    assert O.weave((e,), (e,), "nv12", 8, O.LINEAR)[0][:, 0].tolist() == [150, 50, 0, 0]
    assert O.weave((e,), (e,), "nv12", 8, O.COMPLEX)[0][:, 0].tolist() == [175, 25, 0, 0]      # (7 x 200 + 4) >> 3, (-200 + 400 + 4) >> 3, (-200 + 4) >> 3 -> 0
    # P010: dirty low bits are ignored by the filters and come out canonical; yuv420p10le: the high bits are masked
    w = np.array([[(100 << 6) | 63], [(200 << 6) | 1], [(300 << 6) | 32], [(400 << 6)]], np.uint16)
    assert O.weave((w,), (w,), "nv12", 10, O.LINEAR)[0][:, 0].tolist() == [v << 6 for v in (125, 200, 300, 375)]
    v = np.array([[100 | 0xfc00], [200 | 0x8000], [300], [400 | 0x0400]], np.uint16)
    assert O.weave((v,), (v,), "i420", 10, O.LINEAR)[0][:, 0].tolist() == [125, 200, 300, 375]
    # even rows from `even`, odd rows from `odd`, each filtered inside its own source
    a, b = np.full((4, 1), 40, np.uint8), np.full((4, 1), 80, np.uint8)
    assert O.weave((a,), (b,), "nv12", 8, O.COMPLEX)[0][:, 0].tolist() == [40, 80, 40, 80]
