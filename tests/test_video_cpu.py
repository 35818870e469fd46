"""CPU checks of the video API (include/fldr_video.h, libfldr_video.so): the library's symbol table and link, the header as plain C99 /
C++, the C example, the packed-fp32 guard, the binding's struct mirrors, the colour definition of tests/yuv_oracle.py against the
constants table of the kernels, and the argument checks — which happen before any device call, so they run without a GPU."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import yuv_float_ref as F
import yuv_oracle as O
from lib_checks import declared as _declared, disassemble as _disassemble, syms as _syms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fldr-vfi_amd")
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "fldr_video.h")
LIB = os.path.join(PKG, "libfldr_video.so")
TEST_LIB = os.path.join(PKG, "libfldr_video_test.so")                          # -DFLDR_TEST_HOOKS: + include/fldr_video_test_hooks.h
HOOKS_HDR = os.path.join(INC, "fldr_video_test_hooks.h")
COLOR_H = os.path.join(PKG, "video", "yuv_color.h")


# ---- the library ----------------------------------------------------------------------------------------------------------------
def test_library_exports_exactly_the_header():
    declared = _declared(HDR, "FLDR_VIDEO_API")
    assert len(declared) == 9, sorted(declared)
    assert _syms(LIB, ["--defined-only"]) == declared
    import fldr_video
    assert set(fldr_video.EXPORTS) == declared


def test_library_links_only_the_model_api():
    dyn = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    assert re.search(r"NEEDED.*\[libfldr_model\.so\]", dyn), dyn
    assert not re.search(r"NEEDED.*\[libfldr_hip\.so\]", dyn), dyn
    assert re.search(r"R(UN)?PATH.*\$ORIGIN", dyn), dyn
    used = set(n for n in _syms(LIB, ["--undefined-only"]) if n.startswith("fldr_"))
    assert used and used <= _declared(os.path.join(INC, "fldr_model.h"), "FLDR_MODEL_API"), sorted(used)
    assert "fldr_model_forward" in used


def test_model_and_hip_libraries_keep_their_exports():
    model = _declared(os.path.join(INC, "fldr_model.h"), "FLDR_MODEL_API")
    assert len(model) == 9
    assert _syms(os.path.join(PKG, "libfldr_model.so"), ["--defined-only"]) == model
    hip = _declared(os.path.join(INC, "fldr_hip.h"), "FLDR_API")
    assert _syms(os.path.join(PKG, "libfldr_hip.so"), ["--defined-only"]) == hip
    assert not any(n.startswith("fldr_video") for n in model | hip)


@pytest.mark.parametrize("compiler", [["gcc", "-std=c99", "-x", "c"], ["g++", "-std=c++11", "-x", "c++"]])
def test_header_is_plain_c99_and_cxx(compiler, tmp_path):
    if not shutil.which(compiler[0]):
        pytest.skip(compiler[0] + " not installed")
    src = tmp_path / "h.c"
    src.write_text('#include "fldr_video.h"\nint main(void) { return fldr_video_sizeof(0) > 0 ? 0 : 1; }\n')
    r = subprocess.run(compiler + ["-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I" + INC, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_example_builds_with_cc(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if not cc:
        pytest.skip("no C compiler")
    exe = tmp_path / "fldr_slowmo"
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + INC, "-o", str(exe),
                        os.path.join(ROOT, "examples", "fldr_slowmo.c"), "-L" + PKG, "-l:libfldr_video.so", "-l:libfldr_model.so",
                        "-Wl,-rpath," + PKG], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    src = open(os.path.join(ROOT, "examples", "fldr_slowmo.c")).read()
    assert "hip" not in re.sub(r"/\*.*?\*/", "", src, flags=re.S).lower()
    u = subprocess.run([str(exe)], capture_output=True, text=True)            # no arguments: usage, no device touched
    assert u.returncode == 2 and "usage" in u.stderr


def _no_unsafe_packed_fp32(lib):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_pk_opsel.py"), lib], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def _no_ashr_pk(lib):
    n = 0
    for txt in _disassemble(lib):
        assert "yuv420_to_planar_pair_kernel" in txt
        n += len(re.findall(r"\bv_ashr_pk_[ui]8_i32\b", txt))
    assert n == 0


def test_no_unsafe_packed_fp32_in_the_video_library():
    _no_unsafe_packed_fp32(LIB)


def test_no_ashr_pk_in_the_video_library():
    """v_ashr_pk_u8_i32 / v_ashr_pk_i8_i32 leave bits 16..31 of their result stale on gfx950, while hipcc ORs that result with other
    bytes (video_kernels.hip, pack4): none may be in the library."""
    _no_ashr_pk(LIB)


# ---- the test build: libfldr_video_test.so, the binary tests/test_gpu_video_convert.py executes ------------------------------------------
def test_test_library_exports_exactly_the_header_and_the_hooks():
    declared = _declared(HDR, "FLDR_VIDEO_API")
    hooks = _declared(HOOKS_HDR, "FLDR_VIDEO_API")
    assert hooks == {"fldr_video_debug_to_planar", "fldr_video_debug_from_planar", "fldr_video_debug_last_path"}
    assert _syms(TEST_LIB, ["--defined-only"]) == declared | hooks
    import fldr_video
    assert set(fldr_video.HOOKS) == hooks and not set(fldr_video.HOOKS) & set(fldr_video.EXPORTS)


def test_product_library_has_no_hook():
    names = _syms(LIB, []) | _syms(os.path.join(PKG, "libfldr_model.so"), [])
    assert not [n for n in names if "debug" in n.lower()], sorted(names)
    assert "debug" not in open(HDR).read().lower()


def test_test_library_links_like_the_product():
    dyn = subprocess.run(["readelf", "-d", TEST_LIB], capture_output=True, text=True, check=True).stdout
    assert re.search(r"NEEDED.*\[libfldr_model\.so\]", dyn) and not re.search(r"NEEDED.*\[libfldr_(hip|video)\.so\]", dyn), dyn
    assert re.search(r"R(UN)?PATH.*\$ORIGIN", dyn), dyn
    assert _syms(TEST_LIB, ["--undefined-only"]) == _syms(LIB, ["--undefined-only"])       # the hooks call nothing the product does not


@pytest.mark.parametrize("compiler", [["gcc", "-std=c99", "-x", "c"], ["g++", "-std=c++11", "-x", "c++"]])
def test_hooks_header_is_plain_c99_and_cxx(compiler, tmp_path):
    if not shutil.which(compiler[0]):
        pytest.skip(compiler[0] + " not installed")
    src = tmp_path / "h.c"
    src.write_text('#include "fldr_video_test_hooks.h"\n'
                   'int main(void) { fldr_video_frame in[2]; fldr_video_format f; fldr_video_frame o;\n'
                   '  return fldr_video_debug_to_planar(in, &f, 0, 2, 2, 0) + fldr_video_debug_from_planar(0, &o, &f, 2, 2, 0) + fldr_video_debug_last_path(); }\n')
    r = subprocess.run(compiler + ["-Wall", "-Wextra", "-Werror", "-pedantic", "-Wno-uninitialized", "-fsyntax-only", "-I" + INC, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_no_unsafe_packed_fp32_in_the_video_test_library():
    _no_unsafe_packed_fp32(TEST_LIB)


def test_no_ashr_pk_in_the_video_test_library():
    _no_ashr_pk(TEST_LIB)


def test_hook_sources_stay_out_of_the_product_build():
    """Everything the test build adds sits behind FLDR_TEST_HOOKS: with the macro undefined the preprocessor drops every line that names
    a hook, so libfldr_video.so is compiled from the text it was compiled from before the hooks existed."""
    for name in ("video_host.hip", "video_kernels.hip", "video_internal.h", "frame_host.h", "yuv_stream_host.h", "yuv_run_device.h"):
        depth, live = [], []
        for line in open(os.path.join(PKG, "video", name)).read().splitlines():
            t = line.strip()
            if t.startswith("#ifdef FLDR_TEST_HOOKS"):
                depth.append("hooks")
            elif t.startswith(("#if", "#ifdef", "#ifndef")):
                depth.append("other")
            elif t.startswith("#else") and depth and depth[-1] == "hooks":
                depth[-1] = "other"
            elif t.startswith("#endif"):
                depth.pop()
            elif "hooks" not in depth:
                live.append(t)
        text = "\n".join(l for l in live if not l.startswith("//"))
        assert "g_last_path" not in text and "fldr_video_debug" not in text and "test_hooks.h" not in text, name


def test_binding_struct_sizes_and_version():
    import fldr_video as V
    l = V.lib()
    assert l.fldr_video_version() == V.VIDEO_VERSION
    m = re.search(r"#define FLDR_VIDEO_VERSION (\d+)", open(HDR).read())
    assert int(m.group(1)) == V.VIDEO_VERSION
    for which, cls in enumerate((V.Format, V.Frame, V.IO, V.SessionConfig)):
        assert l.fldr_video_sizeof(which) == ctypes.sizeof(cls)
    assert l.fldr_video_sizeof(4) == V.E_ARG
    for name, v in (("E_ARG", V.E_ARG), ("E_FORMAT", V.E_FORMAT), ("E_PITCH", V.E_PITCH), ("E_PLANE", V.E_PLANE),
                    ("E_WORKSPACE", V.E_WORKSPACE), ("E_DEVICE", V.E_DEVICE)):
        assert re.search(r"#define FLDR_VIDEO_%s\s+\((-?\d+)\)" % name, open(HDR).read()).group(1) == str(v)
        assert v <= -100                                                       # apart from the FLDR_MODEL_E_* range
    assert l.fldr_video_error_string(-3).decode().startswith("fldr_model")    # model codes pass through


# ---- the colour definition --------------------------------------------------------------------------------------------------------
def _table():
    """YUV_COEFFS of yuv_color.h -> {(matrix, range): dict}."""
    body = open(COLOR_H).read().split("YUV_COEFFS[2][2] = {", 1)[1]
    rows = re.findall(r"\{([-0-9, ]+)\}", body)[:4]
    names = ["KYR", "KYG", "KYB", "KUR", "KUG", "KUB", "KVR", "KVG", "KVB", "KY", "KRV", "KBU", "KGU", "KGV", "YOFF"]
    out = {}
    for i, row in enumerate(rows):
        out[(("bt601", "bt709")[i // 2], ("limited", "full")[i % 2])] = dict(zip(names, (int(v) for v in row.split(","))))
    return out


def test_constants_table_is_derived_from_kr_kb():
    t = _table()
    assert len(t) == 4
    for (mat, rng), row in t.items():
        assert row == O.constants(mat, rng), (mat, rng)
        sy = 219 / 255 if rng == "limited" else 1.0
        assert row["KYR"] + row["KYG"] + row["KYB"] == round(sy * 65536)
        assert row["KUR"] + row["KUG"] == -row["KUB"] and row["KVG"] + row["KVB"] == -row["KVR"]
    b = t[("bt709", "limited")]
    assert (b["KYR"], b["KYG"], b["KYB"], b["KUB"]) == (11966, 40254, 4064, 28784)
    assert (b["KY"], b["KRV"], b["KBU"], b["KGU"], b["KGV"]) == (76309, 117489, 138438, 13975, 34925)


@pytest.mark.parametrize("mat", list(O.MATRICES))
@pytest.mark.parametrize("rng", O.RANGES)
def test_int32_headroom_over_all_triples(mat, rng):
    """Every accumulator of both kernels, over all 2^24 (Y, U, V) and (R, G, B) triples (the chroma sums at their extremes: all taps
    equal), stays inside int32."""
    k = O.constants(mat, rng)
    v = np.arange(256, dtype=np.int64)
    A, B_, C = np.meshgrid(v, v, v, indexing="ij")
    # upsampling: Y = A, U = B_, V = C
    yv = (A - k["YOFF"]) * 8 * k["KY"]
    cu, cv = 8 * B_ - 1024, 8 * C - 1024
    m = 0
    for acc in (yv + k["KRV"] * cv + (1 << 18), yv - k["KGU"] * cu - k["KGV"] * cv + (1 << 18), yv + k["KBU"] * cu + (1 << 18),
                yv - k["KGU"] * cu, k["KRV"] * cv, k["KBU"] * cu, k["KGV"] * cv):
        m = max(m, int(np.abs(acc).max()))
    # downsampling: R = A, G = B_, B = C; eight taps of one pixel's value
    for kr, kg, kb in ((k["KYR"], k["KYG"], k["KYB"]), (k["KUR"], k["KUG"], k["KUB"]), (k["KVR"], k["KVG"], k["KVB"])):
        p = kr * A + kg * B_ + kb * C
        m = max(m, int(np.abs(8 * p + (1 << 18)).max()), int(np.abs(kr * A + kg * B_).max()))
    assert m < 2 ** 31 - 1, m
    assert m <= 2.9e8


@pytest.mark.parametrize("mat", list(O.MATRICES))
@pytest.mark.parametrize("rng", O.RANGES)
def test_known_colours(mat, rng):
    lim = rng == "limited"
    Y, U, V = O.rgb_to_yuv444([0, 255, 128, 77], [0, 255, 128, 77], [0, 255, 128, 77], mat, rng)
    assert list(Y[:2]) == ([16, 235] if lim else [0, 255])
    assert list(U) == [128] * 4 and list(V) == [128] * 4                      # grey has no chroma
    # the six primaries and secondaries through the 4:2:0 path on a flat 4 x 4 frame: Y from the matrix, flat chroma, back within 2
    kr, kb = O.MATRICES[mat]
    for rgb in ((255, 0, 0), (0, 255, 0), (0, 0, 255), (0, 255, 255), (255, 0, 255), (255, 255, 0)):
        bgr = np.stack([np.full((4, 4), c, np.uint8) for c in rgb[::-1]])
        y, u, v = O.bgr_to_yuv420(bgr, mat, rng)
        r, g, b = rgb
        ey = (kr * r + (1 - kr - kb) * g + kb * b) * (219 / 255 if lim else 1) + (16 if lim else 0)
        sc = 224 / 255 if lim else 1
        eu = min(max(128 + sc * (b - (ey - (16 if lim else 0)) / (219 / 255 if lim else 1)) / (2 * (1 - kb)), 0), 255)
        ev = min(max(128 + sc * (r - (ey - (16 if lim else 0)) / (219 / 255 if lim else 1)) / (2 * (1 - kr)), 0), 255)
        assert np.all(np.abs(y.astype(float) - ey) <= 0.5 + 1e-9) and np.all(np.abs(u.astype(float) - eu) <= 1) and \
            np.all(np.abs(v.astype(float) - ev) <= 1), (rgb, y[0, 0], ey, u[0, 0], eu, v[0, 0], ev)
        back = O.yuv420_to_bgr(y, u, v, mat, rng)
        assert np.abs(back.astype(int) - bgr.astype(int)).max() <= 2, (rgb, back[:, 0, 0])


@pytest.mark.parametrize("mat", list(O.MATRICES))
@pytest.mark.parametrize("rng", O.RANGES)
def test_round_trip_444(mat, rng):
    v = np.arange(256, dtype=np.int64)
    R, G, B = np.meshgrid(v, v, v, indexing="ij")
    R2, G2, B2 = O.yuv444_to_rgb(*O.rgb_to_yuv444(R, G, B, mat, rng), mat, rng)
    err = max(np.abs(R2 - R).max(), np.abs(G2 - G).max(), np.abs(B2 - B).max())
    assert err <= (2 if rng == "limited" else 1), err


def test_weights_on_a_hand_worked_3x3_frame():
    """An odd-size frame (3 x 3: chroma 2 x 2), worked by hand from the siting rules."""
    mat, rng = "bt709", "full"
    k = O.constants(mat, rng)
    # upsampling: Y = 128 everywhere; U = [[a, b], [c, d]], V = 128 -> B - Y follows the weighted U
    U = np.array([[100, 160], [40, 220]], np.uint8)
    Vp = np.full((2, 2), 128, np.uint8)
    Y = np.full((3, 3), 128, np.uint8)
    bgr = O.yuv420_to_bgr(Y, U, Vp, mat, rng)
    # pixel (x, y): horizontal weights x=0: col0 x2; x=1: col0 + col1; x=2: col1 x2.  vertical y=0: rows 0(1, clamped) + 0(3);
    # y=1: row0 x3 + row1 x1; y=2: row0 x1 + row1 x3
    hw = {0: {0: 2}, 1: {0: 1, 1: 1}, 2: {1: 2}}
    vw = {0: {0: 4}, 1: {0: 3, 1: 1}, 2: {0: 1, 1: 3}}
    for yy in range(3):
        for xx in range(3):
            su = sum(wv * wh * int(U[r, c]) for r, wv in vw[yy].items() for c, wh in hw[xx].items())
            cu = su - 1024
            b = min(max((128 * 8 * k["KY"] + k["KBU"] * cu + (1 << 18)) >> 19, 0), 255)
            assert bgr[0, yy, xx] == b, (xx, yy)
    # downsampling: chroma (i, j) from columns 2i-1, 2i, 2i+1 (weights 1, 2, 1, clamped) and rows 2j, 2j+1 (1, 1, clamped)
    rng_ = np.random.default_rng(0)
    bgr = rng_.integers(0, 256, (3, 3, 3)).astype(np.uint8)
    _, u, v = O.bgr_to_yuv420(bgr, mat, rng)
    B, G, R = (bgr[c].astype(np.int64) for c in range(3))
    up = k["KUR"] * R + k["KUG"] * G + k["KUB"] * B
    cols = {0: {0: 3, 1: 1}, 1: {1: 1, 2: 3}}                               # i=0: cols -1->0 (1) + 0 (2) + 1 (1); i=1: 1 (1) + 2 (2) + 3->2 (1)
    rows = {0: {0: 1, 1: 1}, 1: {2: 2}}                                      # j=1: rows 2, 3->2
    for j in range(2):
        for i in range(2):
            s = sum(wr * wc * int(up[r, c]) for r, wr in rows[j].items() for c, wc in cols[i].items())
            assert u[j, i] == min(max(((s + (1 << 18)) >> 19) + 128, 0), 255), (i, j)
    assert u.shape == v.shape == (2, 2)


# ---- argument errors without a device ---------------------------------------------------------------------------------------------
def _io(V, H=64, W=64, layout="nv12"):
    buf = np.zeros(H * W * 4, np.uint8)
    io = V.IO()
    io.H, io.W = H, W
    io.in_format, io.out_format = V.Format(layout), V.Format(layout)
    shapes = V.plane_shapes(layout, H, W)
    for f in range(2):
        for p, (r, c) in enumerate(shapes):
            io.in_[f].plane[p], io.in_[f].pitch[p] = buf.ctypes.data, c
    outs = (V.Frame * 1)()
    for p, (r, c) in enumerate(shapes):
        outs[0].plane[p], outs[0].pitch[p] = buf.ctypes.data, c
    io.n_t, io.t, io.out = 1, buf.ctypes.data, ctypes.cast(outs, ctypes.POINTER(V.Frame))
    io._keep = (buf, outs)
    return io


@pytest.mark.parametrize("layout", ["nv12", "i420"])
def test_argument_errors_before_any_device_call(layout):
    import fldr_video as V
    l = V.lib()
    call = lambda io: l.fldr_video_forward(None, ctypes.byref(io), None, 0, None)
    assert call(_io(V, layout=layout)) == V.E_ARG                           # valid io, no model
    cases = []
    for field, val in (("layout", 2), ("matrix", 2), ("range", 2), ("matrix", -1)):
        io = _io(V, layout=layout); setattr(io.in_format, field, val); cases.append((io, V.E_FORMAT))
        io = _io(V, layout=layout); setattr(io.out_format, field, val); cases.append((io, V.E_FORMAT))
    io = _io(V, layout=layout); io.in_format.reserved[4] = 1; cases.append((io, V.E_FORMAT))
    io = _io(V, layout=layout); io.out_format.reserved[0] = 7; cases.append((io, V.E_FORMAT))
    io = _io(V, layout=layout); io.in_[0].pitch[0] = 63; cases.append((io, V.E_PITCH))
    io = _io(V, layout=layout); io.out[0].pitch[1] = (32 if layout == "i420" else 64) - 1; cases.append((io, V.E_PITCH))
    io = _io(V, layout=layout); io.in_[1].pitch[1] = 63 if layout == "nv12" else 31; cases.append((io, V.E_PITCH))
    io = _io(V, layout=layout); io.in_[1].plane[1] = None; cases.append((io, V.E_PLANE))
    io = _io(V, layout=layout); io.out[0].plane[0] = None; cases.append((io, V.E_PLANE))
    if layout == "i420":
        io = _io(V, layout=layout); io.in_[0].plane[2] = None; cases.append((io, V.E_PLANE))
    io = _io(V, layout=layout); io.n_t = 0; cases.append((io, V.E_ARG))
    io = _io(V, layout=layout); io.t = None; cases.append((io, V.E_ARG))
    io = _io(V, layout=layout); io.W = 1; cases.append((io, V.E_ARG))
    for io, code in cases:
        assert call(io) == code
    assert l.fldr_video_forward(None, None, None, 0, None) == V.E_ARG
    # NV12 needs 2 ceil(W/2) bytes per chroma row: W = 63 -> 64
    io = _io(V, W=63, layout=layout)
    io.in_[0].pitch[1] = 63 if layout == "nv12" else 31
    assert call(io) == V.E_PITCH
    assert l.fldr_video_workspace_bytes(None, 64, 64, 1) == V.E_ARG


def test_session_argument_errors_before_any_device_call():
    import fldr_video as V
    l = V.lib()
    h = ctypes.c_void_p()
    cfg = V.SessionConfig()
    cfg.H, cfg.W, cfg.n_t = 64, 64, 1
    cfg.in_format, cfg.out_format = V.Format("nv12"), V.Format("i420")
    assert l.fldr_video_session_create(None, ctypes.byref(cfg), ctypes.byref(h)) == V.E_ARG
    cfg.reserved[1] = 1
    assert l.fldr_video_session_create(None, ctypes.byref(cfg), ctypes.byref(h)) == V.E_FORMAT
    cfg.reserved[1] = 0
    cfg.out_format.range = 3
    assert l.fldr_video_session_create(None, ctypes.byref(cfg), ctypes.byref(h)) == V.E_FORMAT
    cfg.out_format.range = 0
    cfg.n_t = 0
    assert l.fldr_video_session_create(None, ctypes.byref(cfg), ctypes.byref(h)) == V.E_ARG
    n = ctypes.c_int()
    assert l.fldr_video_session_push(None, None, None, ctypes.byref(n)) == V.E_ARG
    assert l.fldr_video_session_reset(None) == V.E_ARG
    l.fldr_video_session_destroy(None)


@pytest.mark.parametrize("layout", ["nv12", "i420"])
@pytest.mark.parametrize("depth", [8, 10])
def test_hook_argument_errors_before_any_device_call(layout, depth):
    """The converter hooks of libfldr_video_test.so validate as fldr_video_forward does (format, frame, H, W >= 2) and want the planar
    side 256-byte aligned; every refusal comes back before a device call, so this runs without a GPU."""
    import fldr_video as V
    l = V.test_hooks()
    assert l.fldr_video_debug_last_path() == -1                                # nothing launched in this process
    H, W, b = 64, 64, depth // 8 if depth == 8 else 2
    buf = np.zeros(H * W * 16 + 512, np.uint8)
    base = (buf.ctypes.data + 255) // 256 * 256
    shapes = V.plane_shapes(layout, H, W)

    def frame():
        f = V.Frame()
        for p, (r, c) in enumerate(shapes):
            f.plane[p], f.pitch[p] = base, c * b
        return f

    def call(mutate=lambda fr, fmt: None, planar=base, H=H, W=W, which="both"):
        codes = []
        fmt = V.Format(layout, depth=depth)
        frames = (V.Frame * 2)(frame(), frame())
        mutate(frames[1], fmt)
        if which in ("both", "in"):
            codes.append(l.fldr_video_debug_to_planar(frames, ctypes.byref(fmt), planar, H, W, None))
        if which in ("both", "out"):
            codes.append(l.fldr_video_debug_from_planar(planar, ctypes.byref(frames[1]), ctypes.byref(fmt), H, W, None))
        assert len(set(codes)) == 1, codes
        return codes[0]
    assert call(planar=None) == V.E_ARG
    assert call(planar=base + 128) == V.E_ARG and call(planar=base + 8) == V.E_ARG          # the workspace's alignment: 256 bytes
    assert call(H=1) == V.E_ARG and call(W=1) == V.E_ARG
    assert l.fldr_video_debug_to_planar(None, ctypes.byref(V.Format(layout)), base, H, W, None) == V.E_ARG
    assert l.fldr_video_debug_from_planar(base, None, ctypes.byref(V.Format(layout)), H, W, None) == V.E_ARG
    assert l.fldr_video_debug_to_planar((V.Frame * 2)(frame(), frame()), None, base, H, W, None) == V.E_ARG
    for field, val in (("layout", 2), ("matrix", 2), ("range", -1), ("depth", 9), ("depth", 12)):
        assert call(lambda fr, fmt: setattr(fmt, field, val)) == V.E_FORMAT, field
    assert call(lambda fr, fmt: fmt.reserved.__setitem__(3, 1)) == V.E_FORMAT
    for p in range(len(shapes)):
        assert call(lambda fr, fmt: fr.plane.__setitem__(p, None)) == V.E_PLANE, p
        assert call(lambda fr, fmt: fr.pitch.__setitem__(p, shapes[p][1] * b - b)) == V.E_PITCH, p
        if depth == 10:
            assert call(lambda fr, fmt: fr.plane.__setitem__(p, base + 1)) == V.E_PLANE, p
            assert call(lambda fr, fmt: fr.pitch.__setitem__(p, shapes[p][1] * b + 1)) == V.E_PITCH, p
    assert l.fldr_video_debug_last_path() == -1                                # and still nothing was launched


# ---- the integer definition against the standard in float64 (tests/yuv_float_ref.py) ------------------------------------------------------
@pytest.mark.parametrize("mat", list(O.MATRICES))
@pytest.mark.parametrize("rng", O.RANGES)
def test_all_triples_are_within_half_a_code_of_the_float_definition(mat, rng):
    """Every 8-bit (Y, U, V) and (R, G, B) triple through the integer 4:4:4 forms against the clipped float64 value of the definition
    written from the standard: 0.5 for the rounding plus the quantisation of the 16-bit coefficients.  Bound 0.51; measured maximum over the
    four formats 0.5016 (to RGB: BT.601 limited) and 0.5020 (to YUV: BT.709 limited)."""
    v = np.arange(256, dtype=np.int64)
    A, B_, C = (a.ravel() for a in np.meshgrid(v, v, v, indexing="ij"))
    worst = {}
    for name, got, ref in (("to RGB", O.yuv444_to_rgb(A, B_, C, mat, rng), F.ycbcr_to_rgb(A, B_, C, mat, rng)),
                           ("to YUV", O.rgb_to_yuv444(A, B_, C, mat, rng), F.rgb_to_ycbcr(A, B_, C, mat, rng))):
        worst[name] = max(float(np.abs(g - F.clip(r)).max()) for g, r in zip(got, ref))
    print("8-bit 4:4:4, %s %s: max |integer - float| = %.4f (to RGB), %.4f (to YUV)" % (mat, rng, worst["to RGB"], worst["to YUV"]))
    assert max(worst.values()) <= 0.51, worst


@pytest.mark.parametrize("mat", list(O.MATRICES))
@pytest.mark.parametrize("rng", O.RANGES)
def test_noise_frames_are_within_the_derived_bound_of_the_float_definition(mat, rng):
    """Full 4:2:0 noise frames (odd and even sizes) in both directions, depth 8: the integer oracle against the float64 definition with its
    own statement of the siting and the filters.  The bound is derived from the table: 0.5 + sum over the expression's coefficients of
    2^-17 x the largest |operand| (yuv_float_ref.coefficient_bound): 0.5039 to RGB, 0.5058 to YUV.  Measured maxima over the four formats: 0.5013 to RGB, 0.5010 to YUV."""
    k = O.constants(mat, rng)
    up_bound, down_bound = 0.5 + F.coefficient_bound(k, 8, "to_rgb"), 0.5 + F.coefficient_bound(k, 8, "to_yuv")
    assert 0.5 < up_bound < 0.504 and 0.5 < down_bound < 0.506
    eu = ed = 0.0
    for H, W in ((203, 301), (64, 96), (2, 2), (3, 5)):
        g = np.random.default_rng(H * W)
        ch, cw = O.chroma_size(H, W)
        Y, U, V = (g.integers(0, 256, s).astype(np.uint8) for s in ((H, W), (ch, cw), (ch, cw)))
        eu = max(eu, float(np.abs(O.yuv420_to_bgr(Y, U, V, mat, rng) - F.yuv420_to_bgr(Y, U, V, mat, rng)).max()))
        bgr = g.integers(0, 256, (3, H, W)).astype(np.uint8)
        ed = max(ed, max(float(np.abs(i - f).max()) for i, f in zip(O.bgr_to_yuv420(bgr, mat, rng), F.bgr_to_yuv420(bgr, mat, rng))))
    print("8-bit 4:2:0 noise, %s %s: max |integer - float| = %.4f (to RGB, bound %.4f), %.4f (to YUV, bound %.4f)" % (mat, rng, eu, up_bound, ed, down_bound))
    assert eu <= up_bound and ed <= down_bound, (eu, up_bound, ed, down_bound)
