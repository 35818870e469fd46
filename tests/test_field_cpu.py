"""CPU checks of the field API (include/fldr_field.h, libfldr_field.so): the library's symbol table and link, the header as plain C99 /
C++, the C example, the code-generation guards, the binding's struct mirrors, the argument checks of every layer — which happen before
any device call, so they run without a GPU —, the schedule against a brute-force statement, and the oracle (tests/field_oracle.py)
alone: the properties the weave is there for.  A misaligned or short workspace is not here: fldr_field_forward checks the model before
the workspace (the size of which only a model can say), so those two errors need a model and are in tests/test_gpu_field.py."""
import ctypes
import glob
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import field_oracle as F
from lib_checks import declared as _declared, disassemble as _disassemble, syms as _syms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fldr-vfi_amd")
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "fldr_field.h")
LIB = os.path.join(PKG, "libfldr_field.so")
EXAMPLE = os.path.join(ROOT, "examples", "fldr_deint.c")
FORBIDDEN = ("fldr_chroma", "fldr_pack10", "fldr_cadence", "fldr_repeat", "fldr_pipe", "fldr_shutter", "fldr_light")
FORMATS = [("nv12", 8), ("nv12", 10), ("i420", 8), ("i420", 10)]


# ---- the library ------------------------------------------------------------------------------------------------------------------------
def test_library_exports_exactly_the_header():
    declared = _declared(HDR, "FLDR_FIELD_API")
    assert len(declared) == 15, sorted(declared)
    assert _syms(LIB, ["--defined-only"]) == declared
    import fldr_field
    assert set(fldr_field.EXPORTS) == declared
    assert all(n.startswith("fldr_field_") for n in declared)
    for name in ("version", "error_string", "sizeof", "weave", "workspace_bytes", "temporal", "forward", "plan", "create", "destroy",
                 "max_out", "push", "flush", "reset"):
        assert "fldr_field_" + name in declared, name


def test_library_links_only_the_rate_video_and_model_apis():
    dyn = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    needed = re.findall(r"NEEDED.*\[(libfldr_[a-z0-9_]+\.so)\]", dyn)
    assert sorted(needed) == ["libfldr_rate.so", "libfldr_video.so"], dyn
    assert re.search(r"R(UN)?PATH.*\$ORIGIN", dyn), dyn
    used = set(n for n in _syms(LIB, ["--undefined-only"]) if n.startswith("fldr_"))
    allowed = (_declared(os.path.join(INC, "fldr_rate.h"), "FLDR_RATE_API") | _declared(os.path.join(INC, "fldr_video.h"), "FLDR_VIDEO_API") |
               _declared(os.path.join(INC, "fldr_model.h"), "FLDR_MODEL_API"))
    assert used and used <= allowed, sorted(used)
    # the enqueue-only entry points, and none of the synchronising converter underneath
    assert {"fldr_scene_measure", "fldr_video_forward", "fldr_video_workspace_bytes"} <= used
    assert not [n for n in used if n.startswith(("fldr_rate_push", "fldr_rate_create", "fldr_rate_forward", "fldr_video_session"))], sorted(used)


def test_header_and_library_name_no_library_beside_them():
    text = open(HDR).read().lower()
    strings = subprocess.run(["strings", LIB], capture_output=True, text=True, check=True).stdout.lower()
    names = [n.lower() for n in _syms(LIB, [])]
    raw = open(LIB, "rb").read().lower()
    for other in FORBIDDEN:
        assert other not in text and other not in strings and other.encode() not in raw and not [n for n in names if other in n], other


def test_nothing_else_names_the_field_api():
    for h in glob.glob(os.path.join(INC, "*.h")):
        if h != HDR:
            assert "fldr_field" not in open(h).read().lower(), h
    libs = [l for l in glob.glob(os.path.join(PKG, "libfldr_*.so")) if l != LIB]
    assert len(libs) >= 10, libs
    for l in libs:
        assert not [n for n in _syms(l, []) if "fldr_field" in n], l
        assert b"fldr_field" not in open(l, "rb").read(), l


@pytest.mark.parametrize("compiler", [["gcc", "-std=c99", "-x", "c"], ["g++", "-std=c++11", "-x", "c++"]])
def test_header_is_plain_c99_and_cxx(compiler, tmp_path):
    assert shutil.which(compiler[0]), compiler[0] + " not installed"
    src = tmp_path / "h.c"
    src.write_text('#include "fldr_field.h"\nint main(void) { fldr_field_config c; fldr_field_report r; fldr_field_params p; c.rate = 2; r.cut = 0;\n'
                   '  p.still = FLDR_FIELD_STILL_DEFAULT8; p.slack = FLDR_FIELD_SLACK_DEFAULT8;\n'
                   '  return fldr_field_sizeof(2) == (int)sizeof(c) && c.rate == 2 && r.cut == 0 && p.still == 2 && p.slack == 16 &&\n'
                   '         FLDR_FIELD_E_ARG == -1000 && FLDR_FIELD_MOTION == 0 && FLDR_FIELD_INTRA == 1 && sizeof(fldr_field_params) == 16 ? 0 : 1; }\n')
    r = subprocess.run(compiler + ["-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I" + INC, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "hip" not in re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S).lower()


def test_header_says_where_the_defaults_come_from_and_what_is_out_of_scope():
    text = open(HDR).read()
    assert "synthetic content only" in text and "not on footage" in text
    for s in ("quarter line", "4:2:2, packed and RGB", "declared (tff), not detected", "one frame late", "no fused path", "pad < size"):
        assert s in text, s
    assert F.defaults(8) == (2, 16) and F.defaults(10) == (8, 64)


def test_example_builds_with_cc(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    exe = tmp_path / "fldr_deint"
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + INC, "-o", str(exe), EXAMPLE, "-L" + PKG,
                        "-l:libfldr_field.so", "-l:libfldr_rate.so", "-l:libfldr_video.so", "-l:libfldr_model.so", "-Wl,-rpath," + PKG],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    src = open(EXAMPLE).read()
    assert "hip" not in re.sub(r"/\*.*?\*/", "", src, flags=re.S).lower()
    u = subprocess.run([str(exe)], capture_output=True, text=True)            # no arguments: usage, no device touched
    assert u.returncode == 2 and "usage" in u.stderr and "rate=" in u.stderr and "bff" in u.stderr
    for bad in (["w.npz", "64", "66", "-", "-"],                              # H not a multiple of 4
                ["w.npz", "64", "64", "-", "-", "rate=3"],
                ["w.npz", "64", "64", "-", "-", "still=x"],
                ["w.npz", "64", "64", "-", "-", "tff"]):
        u = subprocess.run([str(exe)] + bad, capture_output=True, text=True)
        assert u.returncode == 2 and "usage" in u.stderr, bad


def test_no_unsafe_packed_fp32_in_the_field_library():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_pk_opsel.py"), LIB], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_kernel_uses_16_byte_accesses_and_no_float_lds_or_atomics():
    txt = "\n".join(_disassemble(LIB))
    assert "field_weave_kernel" in txt
    assert re.search(r"\bglobal_load_dwordx4\b", txt) and re.search(r"\bglobal_store_dwordx4\b", txt)      # 16 bytes per lane
    assert not re.search(r"\bv_(cvt_f|rcp|add_f|mul_f|fma_f|mac_f|pk_\w+_f)", txt)                         # integers only
    assert not re.search(r"\bds_(read|write|load|store)", txt) and not re.search(r"\b\w+_atomic_", txt)


def test_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    ks = KR.kernels(LIB)
    assert len(ks) == 3, [k["name"] for k in ks]          # one per sample form; wide / per-sample and the component stride are decided per plane
    for k in ks:
        assert k.get("scratch", -1) == 0 and k.get("vgpr_spills", -1) == 0 and k.get("sgpr_spills", -1) == 0 and k.get("lds", -1) == 0, k


def test_binding_struct_sizes_and_version():
    import fldr_field as K
    l = K.lib()
    text = open(HDR).read()
    assert l.fldr_field_version() == K.FIELD_VERSION == int(re.search(r"#define FLDR_FIELD_VERSION (\d+)", text).group(1)) == 100
    for which, cls in enumerate((K.Params, K.IO, K.Config, K.Schedule, K.Report)):
        assert l.fldr_field_sizeof(which) == ctypes.sizeof(cls)
    assert ctypes.sizeof(K.Params) == 16 and ctypes.sizeof(K.Report) == 56 and ctypes.sizeof(K.Schedule) == 40
    assert l.fldr_field_sizeof(5) == K.E_ARG
    for name, v in (("E_ARG", K.E_ARG), ("E_SIZE", K.E_SIZE), ("E_WORKSPACE", K.E_WORKSPACE), ("E_DEVICE", K.E_DEVICE)):
        assert re.search(r"#define FLDR_FIELD_%s\s+\((-?\d+)\)" % name, text).group(1) == str(v)
        assert -1100 < v <= -1000                                             # the next free block of one hundred
        assert l.fldr_field_error_string(v).decode().startswith("fldr_field")
    lowest = min(int(v) for h in glob.glob(os.path.join(INC, "*.h")) if h != HDR
                 for v in re.findall(r"#define FLDR_[A-Z0-9]+_E_[A-Z]+\s+\((-\d+)\)", open(h).read()))
    assert -1000 < lowest <= -900                                             # ... below the blocks the other headers use
    for macro, v in (("FLDR_FIELD_STILL_DEFAULT8", K.STILL_DEFAULT8), ("FLDR_FIELD_SLACK_DEFAULT8", K.SLACK_DEFAULT8)):
        assert int(re.search(r"#define %s\s+(\d+)" % macro, text).group(1)) == v, macro
    assert (K.MOTION, K.INTRA) == (F.MOTION, F.INTRA) == (0, 1)
    assert l.fldr_field_error_string(-202).decode().startswith("fldr_rate")      # rate codes pass through,
    assert l.fldr_field_error_string(-101).decode().startswith("fldr_video")     # video codes through it,
    assert l.fldr_field_error_string(-3).decode().startswith("fldr_model")       # and model codes through that
    assert l.fldr_field_error_string(-600).decode() == "fldr_field: unknown error"


# ---- argument errors without a device ---------------------------------------------------------------------------------------------------
def _host_frame(V, layout, depth, H, W, base):
    b = 2 if depth == 10 else 1
    f = V.Frame()
    for p, (r, c) in enumerate(V.plane_shapes(layout, H, W)):
        f.plane[p], f.pitch[p] = base, c * b
    return f


@pytest.mark.parametrize("layout,depth", FORMATS)
def test_weave_argument_errors_before_any_device_call(layout, depth):
    import fldr_field as K
    import fldr_video as V
    H = W = 16
    b = 2 if depth == 10 else 1
    top = F.mx(depth)
    buf = np.zeros(H * W * 4 + 512, np.uint8)
    base = (buf.ctypes.data + 255) // 256 * 256
    shapes = V.plane_shapes(layout, H, W)

    def call(mutate=lambda fr, fmt: None, params=None, H=H, W=W, parity=0, mode=K.MOTION, drop=(), which="prev"):
        fr = {k: _host_frame(V, layout, depth, H if k != "temporal" else H // 2, W, base) for k in ("cur", "prev", "next", "temporal", "out")}
        fmt = V.Format(layout, depth=depth)
        mutate(fr[which], fmt)
        for k in drop:
            fr[k] = None
        return K.weave_raw(H, W, fmt, fr["cur"], fr["prev"], fr["next"], fr["temporal"], parity, mode, None, params, fr["out"], None)
    for h in (0, 2, 3, 5, 6, 18, -4):
        assert call(H=h) == K.E_SIZE, h
    assert call(W=0) == K.E_ARG and call(W=-1) == K.E_ARG
    for bad in (-1, 2):
        assert call(parity=bad) == K.E_ARG and call(mode=bad) == K.E_ARG
    for k in ("cur", "out", "prev", "next", "temporal"):
        assert call(drop=(k,)) == K.E_ARG, k
    assert K.weave_raw(H, W, None, V.Frame(), None, None, None, 0, K.INTRA, None, None, V.Frame(), None) == K.E_ARG
    for still, slack in ((-2, 0), (top + 1, 0), (0, -1), (0, top + 1), (2 ** 31 - 1, 0)):
        assert call(params=K.Params(still, slack)) == K.E_ARG, (still, slack)
    for q in range(2):
        p = K.Params()
        p.reserved[q] = 1
        assert call(params=p) == K.E_ARG
    for field, val in (("layout", 2), ("matrix", 2), ("range", -1), ("depth", 9), ("depth", 12)):
        assert call(lambda fr, fmt: setattr(fmt, field, val)) == V.E_FORMAT, field
    assert call(lambda fr, fmt: fmt.reserved.__setitem__(3, 1)) == V.E_FORMAT
    for which in ("cur", "out", "prev", "next", "temporal"):                  # every plane of every frame the mode reads
        for q in range(len(shapes)):
            assert call(lambda fr, fmt: fr.plane.__setitem__(q, None), which=which) == V.E_PLANE, (which, q)
            assert call(lambda fr, fmt: fr.pitch.__setitem__(q, shapes[q][1] * b - b), which=which) == V.E_PITCH, (which, q)
            if depth == 10:
                assert call(lambda fr, fmt: fr.plane.__setitem__(q, base + 1), which=which) == V.E_PLANE, (which, q)
                assert call(lambda fr, fmt: fr.pitch.__setitem__(q, shapes[q][1] * b + 1), which=which) == V.E_PITCH, (which, q)
    # the stated order: null pointers, size, W / parity / mode, format, params, planes, pitches
    assert call(lambda fr, fmt: setattr(fmt, "layout", 2), H=6, W=0, drop=("cur",)) == K.E_ARG
    assert call(lambda fr, fmt: setattr(fmt, "layout", 2), H=6, W=0) == K.E_SIZE
    assert call(lambda fr, fmt: setattr(fmt, "layout", 2), W=0) == K.E_ARG
    assert call(lambda fr, fmt: (setattr(fmt, "layout", 2), fr.plane.__setitem__(0, None)), params=K.Params(-2, 0)) == V.E_FORMAT
    assert call(lambda fr, fmt: fr.plane.__setitem__(0, None), params=K.Params(-2, 0)) == K.E_ARG
    assert call(lambda fr, fmt: (fr.plane.__setitem__(0, None), fr.pitch.__setitem__(0, 1)), which="cur") == V.E_PLANE
    assert call(lambda fr, fmt: fr.pitch.__setitem__(0, 1), which="cur") == V.E_PITCH
    # last: a frame beyond the kernel's 32-bit index arithmetic (the header names these sizes)
    assert call(H=8640, W=16384 if depth == 8 else 15360) == K.E_ARG
    assert call(H=8640, W=16384 if depth == 8 else 15360, mode=K.INTRA, drop=("prev", "next", "temporal")) == K.E_ARG
    assert not buf.any()


def _io(K, V, layout, depth, H, W, base):
    io = K.IO()
    io.H, io.W, io.format = H, W, V.Format(layout, depth=depth)
    for k in ("cur", "prev", "next", "out"):
        setattr(io, k, _host_frame(V, layout, depth, H, W, base))
    return io


@pytest.mark.parametrize("layout,depth", FORMATS)
def test_forward_argument_errors_before_any_device_call(layout, depth):
    import fldr_field as K
    import fldr_rate as R
    import fldr_video as V
    l = K.lib()
    H, W = 400, 64
    b = 2 if depth == 10 else 1
    buf = np.zeros(4096, np.uint8)
    base = (buf.ctypes.data + 255) // 256 * 256
    shapes = V.plane_shapes(layout, H, W)

    def call(mutate=lambda io: None, ws=base, ws_bytes=1 << 40):
        io = _io(K, V, layout, depth, H, W, base)
        keep = mutate(io)                                                     # noqa: F841  (a Params the io points at)
        return l.fldr_field_forward(None, ctypes.byref(io), ws, ws_bytes, None)
    assert l.fldr_field_forward(None, None, base, 1 << 40, None) == K.E_ARG
    assert call() == K.E_ARG                                                  # valid, no model: the last of the argument checks
    for h in (0, 2, 6, 402, -4):
        assert call(lambda io: setattr(io, "H", h)) == K.E_SIZE, h
    assert call(lambda io: setattr(io, "W", 1)) == K.E_ARG
    for bad in (-1, 2):
        assert call(lambda io: setattr(io, "parity", bad)) == K.E_ARG and call(lambda io: setattr(io, "scene", bad)) == K.E_ARG
    for q in range(4):
        assert call(lambda io: io.reserved.__setitem__(q, 1)) == K.E_ARG

    def with_params(still, slack, rq=None):
        def m(io):
            p = K.Params(still, slack)
            if rq is not None:
                p.reserved[rq] = 1
            io.params = ctypes.pointer(p)
            return p
        return m
    top = F.mx(depth)
    for still, slack in ((-2, 0), (top + 1, 0), (0, -1), (0, top + 1)):
        assert call(with_params(still, slack)) == K.E_ARG
    assert call(with_params(0, 0, 1)) == K.E_ARG
    assert call(with_params(-1, top)) == K.E_ARG and call(with_params(top, 0)) == K.E_ARG     # allowed (and then no model)
    assert call(lambda io: setattr(io.scene_params, "sad_permille", 1001)) == R.E_ARG
    assert call(lambda io: io.scene_params.reserved.__setitem__(1, 1)) == R.E_ARG
    assert call(lambda io: setattr(io.format, "layout", 2)) == V.E_FORMAT
    assert call(lambda io: setattr(io.format, "depth", 12)) == V.E_FORMAT
    for which in ("cur", "prev", "next", "out"):
        for q in range(len(shapes)):
            assert call(lambda io: getattr(io, which).plane.__setitem__(q, None)) == V.E_PLANE, (which, q)
            assert call(lambda io: getattr(io, which).pitch.__setitem__(q, shapes[q][1] * b - b)) == V.E_PITCH, (which, q)
    # the stated order: size, W / parity / scene / reserved, format, params, thresholds, frames, model
    assert call(lambda io: (setattr(io, "H", 6), setattr(io, "W", 1))) == K.E_SIZE
    assert call(lambda io: (setattr(io, "W", 1), setattr(io.format, "layout", 2))) == K.E_ARG
    assert call(lambda io: (setattr(io.format, "layout", 2), setattr(io.scene_params, "sad_permille", 1001))) == V.E_FORMAT
    assert call(lambda io: (setattr(io.scene_params, "sad_permille", 1001), io.cur.plane.__setitem__(0, None))) == R.E_ARG
    assert call(lambda io: io.out.plane.__setitem__(0, None), ws=None) == V.E_PLANE
    # without a model nothing about the workspace is known: a null model comes first
    assert call(ws=None) == K.E_ARG and call(ws=base + 16) == K.E_ARG and call(ws_bytes=0) == K.E_ARG
    assert l.fldr_field_workspace_bytes(None, H, W) == K.E_ARG and l.fldr_field_workspace_bytes(None, 6, W) == K.E_SIZE
    fr = V.Frame()
    fmt = V.Format(layout, depth=depth)
    assert l.fldr_field_temporal(None, H, W, ctypes.byref(fmt), base, ctypes.byref(fr)) == K.E_ARG
    assert l.fldr_field_temporal(None, 6, W, ctypes.byref(fmt), base, ctypes.byref(fr)) == K.E_SIZE
    assert l.fldr_field_temporal(None, H, W, None, base, ctypes.byref(fr)) == K.E_ARG
    assert l.fldr_field_scene_state(None, H, W, base) is None
    assert not buf.any()


def test_stream_argument_errors_before_any_device_call():
    import fldr_field as K
    import fldr_rate as R
    import fldr_video as V
    l = K.lib()
    h = ctypes.c_void_p()

    def create(mutate=lambda c: None, **kw):
        cfg = K.make_config(400, 64, V.Format("i420"), **kw)
        keep = mutate(cfg)                                                    # noqa: F841
        return l.fldr_field_create(None, ctypes.byref(cfg), ctypes.byref(h))
    assert create() == K.E_ARG                                               # valid, no model
    for bad in (0, 2, 6, 402):
        assert create(lambda c: setattr(c, "H", bad)) == K.E_SIZE, bad
    assert create(lambda c: setattr(c, "W", 1)) == K.E_ARG
    for bad in (0, 3, -1):
        assert create(lambda c: setattr(c, "rate", bad)) == K.E_ARG, bad
    for bad in (2, -1):
        assert create(lambda c: setattr(c, "tff", bad)) == K.E_ARG and create(lambda c: setattr(c, "scene", bad)) == K.E_ARG
    assert create(lambda c: setattr(c, "device", -1)) == K.E_ARG
    for q in range(4):
        assert create(lambda c: c.reserved.__setitem__(q, 1)) == K.E_ARG
    assert create(lambda c: setattr(c.format, "layout", 3)) == V.E_FORMAT
    assert create(params=(256, 0)) == K.E_ARG and create(params=(0, -1)) == K.E_ARG and create(params=(-1, 255)) == K.E_ARG
    assert create(lambda c: setattr(c.scene_params, "hist_permille", -1)) == R.E_ARG
    assert create(lambda c: (setattr(c, "H", 6), setattr(c, "rate", 3))) == K.E_SIZE      # the size first
    assert create(lambda c: (setattr(c, "rate", 3), setattr(c.format, "layout", 3))) == K.E_ARG
    assert create(lambda c: (setattr(c.format, "layout", 3), setattr(c.scene_params, "hist_permille", -1))) == V.E_FORMAT
    assert l.fldr_field_create(None, None, ctypes.byref(h)) == K.E_ARG
    n = ctypes.c_int()
    assert l.fldr_field_push(None, None, None, ctypes.byref(n), None) == K.E_ARG
    assert l.fldr_field_flush(None, None, ctypes.byref(n), None) == K.E_ARG
    assert l.fldr_field_reset(None) == K.E_ARG
    assert l.fldr_field_max_out(None) == K.E_ARG
    l.fldr_field_destroy(None)
    assert not h.value


# ---- the schedule -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tff", [True, False])
@pytest.mark.parametrize("rate", [1, 2])
def test_plan_equals_the_brute_force_statement(tff, rate):
    import fldr_field as K
    for j in range(41):
        want = F.plan(j, tff, rate)
        code, got = K.plan_raw(j, tff, rate)
        assert code == 0 and got == want == K.plan(j, tff, rate), j
        m = want["field"]
        assert want["parity"] == (m % 2 if tff else 1 - m % 2)
        assert want["cur"] - 1 <= want["prev"] <= want["cur"] <= want["next"] <= want["cur"] + 1
    assert K.plan_raw(0, tff, rate)[1]["prev"] == -1


def test_plan_refuses_what_is_out_of_range():
    import fldr_field as K
    for tff, rate, j in ((2, 2, 0), (-1, 1, 0), (1, 0, 0), (1, 3, 0), (1, 2, -1), (1, 2, 2 ** 62)):
        assert K.plan_raw(j, tff, rate)[0] == K.E_ARG, (tff, rate, j)
    assert K.lib().fldr_field_plan(None, 0, None) == K.E_ARG
    assert K.plan_raw(2 ** 61, 1, 1) == (0, {"field": 2 ** 62, "parity": 0, "cur": 2 ** 61, "prev": 2 ** 61 - 1, "next": 2 ** 61})


@pytest.mark.parametrize("tff", [True, False])
@pytest.mark.parametrize("rate", [1, 2])
def test_push_and_flush_counts_follow_from_the_plan(tff, rate):
    import fldr_field as K
    for N in (0, 1, 2, 6):
        got, want = K.pushes(N, tff, rate), F.stream_outputs(N, tff, rate)
        assert got == want
        counts = [len(c) for c in want]
        if rate == 2:
            assert counts == ([1] + [2] * (N - 1) + [1] if N else [0]) and sum(counts) == 2 * N
            if N:
                assert want[0][0][1] == F.INTRA and want[N][0][1] == F.INTRA and want[N][0][0]["field"] == 2 * N - 1
                assert all(mode == F.MOTION for c in want[1:N] for _, mode in c)
                assert [[p["field"] for p, _ in c] for c in want[1:N]] == [[2 * n - 1, 2 * n] for n in range(1, N)]
        else:
            assert counts == [1] * N + [0]
            assert [c[0][0]["field"] for c in want[:N]] == [2 * n for n in range(N)]
            assert [c[0][1] for c in want[:N]] == [F.INTRA] + [F.MOTION] * (N - 1) if N else True
        fields = [p["field"] for c in want for p, _ in c]
        assert fields == sorted(fields)                                       # in order
        for n, c in enumerate(want[:N]):
            for p, mode in c:                                                 # only the last two frames pushed are needed
                assert {p["cur"], p["next"]} <= {n - 1, n} and (mode == F.INTRA or p["prev"] in (n - 1, n))


# ---- the oracle alone -------------------------------------------------------------------------------------------------------------------
def _noise(rng, layout, depth, H, W, dirty=False):
    import field_frames as FF
    return FF.noise(rng, layout, depth, H, W, dirty)


@pytest.mark.parametrize("layout,depth", FORMATS)
@pytest.mark.parametrize("parity", [0, 1])
def test_oracle_own_rows_intra_and_bounds(layout, depth, parity):
    rng = np.random.default_rng(7 + parity)
    H, W = 12, 11
    top = F.mx(depth)
    cur, prev, nxt = (_noise(rng, layout, depth, H, W, dirty=True) for _ in range(3))
    temporal = _noise(rng, layout, depth, H // 2, W, dirty=True)
    val = lambda pl: F.value(pl, layout, depth)
    for mode, still, slack in ((F.INTRA, 0, 0), (F.MOTION, None, None), (F.MOTION, -1, 0), (F.MOTION, -1, 5), (F.MOTION, top, 3)):
        out = F.weave(cur, prev, nxt, temporal, layout, depth, parity, mode, still, slack)
        for p, o in enumerate(out):
            assert o.dtype == cur[p].dtype and o.shape == cur[p].shape
            assert np.array_equal(o[parity::2], cur[p][parity::2])            # own-parity rows are the input's, dirty bits included
            missing = o[1 - parity::2]
            assert np.array_equal(F.canonical(val(missing), layout, depth), missing)      # canonical words
            R = o.shape[0]
            v = val(cur[p])
            for y in range(1 - parity, R, 2):
                a = v[y - 1] if y > 0 else v[y + 1]
                b = v[y + 1] if y < R - 1 else v[y - 1]
                if mode == F.INTRA:
                    assert np.array_equal(val(o[y]), (a + b + 1) // 2)        # the line average, mirrored at the edges
                elif still == -1:
                    lo, hi = np.maximum(np.minimum(a, b) - slack, 0), np.minimum(np.maximum(a, b) + slack, top)
                    assert ((val(o[y]) >= lo) & (val(o[y]) <= hi)).all()
    # slack = mx with the static rule off returns temporal
    out = F.weave(cur, prev, nxt, temporal, layout, depth, parity, F.MOTION, -1, top)
    for p, o in enumerate(out):
        assert np.array_equal(val(o[1 - parity::2]), val(temporal[p]))
    # still = mx: every sample is static, the output is the average of prev and next whatever temporal says
    out = F.weave(cur, prev, nxt, temporal, layout, depth, parity, F.MOTION, top, 0)
    for p, o in enumerate(out):
        assert np.array_equal(val(o[1 - parity::2]), (val(prev[p][1 - parity::2]) + val(nxt[p][1 - parity::2]) + 1) // 2)


@pytest.mark.parametrize("layout,depth", FORMATS)
@pytest.mark.parametrize("parity", [0, 1])
def test_oracle_a_still_woven_picture_comes_back_exactly(layout, depth, parity):
    rng = np.random.default_rng(11)
    H, W = 8, 9
    picture = _noise(rng, layout, depth, H, W)
    for still in (0, 1, F.defaults(depth)[0], F.mx(depth)):
        for _ in range(2):
            temporal = _noise(rng, layout, depth, H // 2, W)                  # any temporal
            out = F.weave(picture, picture, picture, temporal, layout, depth, parity, F.MOTION, still, 0)
            assert all(np.array_equal(o, p) for o, p in zip(out, picture))


def test_oracle_static_rule_looks_one_column_to_either_side_per_component():
    import fldr_video as V
    H, W = 4, 8
    for layout in ("nv12", "i420"):
        cur = tuple(np.full(s, 100, np.uint8) for s in V.plane_shapes(layout, H, W))
        prev = tuple(p.copy() for p in cur)
        nxt = tuple(p.copy() for p in cur)
        temporal = tuple(np.full((p.shape[0] // 2, p.shape[1]), 60, np.uint8) for p in cur)
        nxt[0][1, 3] = 103                                                    # luma: d = 3 at x = 3, row 1
        out = F.weave(cur, prev, nxt, temporal, layout, 8, 0, F.MOTION, 2, 0)
        assert out[0][1].tolist() == [100, 100, 100, 100, 100, 100, 100, 100]      # moving at x = 2 .. 4: clamped to [100, 100]
        out = F.weave(cur, prev, nxt, temporal, layout, 8, 0, F.MOTION, 2, 50)
        assert out[0][1].tolist() == [100, 100, 60, 60, 60, 100, 100, 100]         # the static average elsewhere; (100 + 103 + 1) >> 1 never shows
        out = F.weave(cur, prev, nxt, temporal, layout, 8, 0, F.MOTION, 3, 50)
        assert out[0][1].tolist() == [100, 100, 100, 102, 100, 100, 100, 100]      # d == still: static
        if layout == "nv12":                                                  # U moves at chroma x = 1: V does not, nor does U two bytes on
            nxt[1][1, 2] = 110
            out = F.weave(cur, prev, nxt, temporal, layout, 8, 0, F.MOTION, 2, 50)
            assert out[1][1].tolist() == [60, 100, 60, 100, 60, 100, 100, 100]
