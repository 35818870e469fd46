"""CPU checks of the RGB API (include/fldr_rgb.h, libfldr_rgb.so): the library's symbol table and link, the header as plain C99 / C++,
the C example, the binding's struct mirrors, the argument checks (decided before any device call, so they run without a GPU), the
listing of the kernels, and the layout and alpha statement of tests/rgb_oracle.py: the header's two worked words, pack / unpack as
inverses, dirt, and the worked alpha numbers."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import rgb_oracle as R
from lib_checks import declared as _declared, disassemble as _disassemble, syms as _syms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fldr-vfi_amd")
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "fldr_rgb.h")
LIB = os.path.join(PKG, "libfldr_rgb.so")
EXAMPLE_C = os.path.join(ROOT, "examples", "fldr_slowmo_rgb.c")
# the functions of the packed 10-bit library's header, one for one, and the alpha pass alone
FUNCTIONS = {"fldr_rgb_" + n for n in ("version", "error_string", "sizeof", "to_planar", "from_planar", "alpha", "workspace_bytes", "forward",
                                       "session_create", "session_push", "session_reset", "session_destroy")}
R_ALPHAS = ("opaque", "nearer", "blend")
OTHER_LIBRARIES = ("fldr_chroma", "fldr_pack10", "fldr_cadence", "fldr_repeat", "fldr_pipe", "fldr_rate", "fldr_scene", "fldr_shutter", "fldr_light")


# ---- the library ----------------------------------------------------------------------------------------------------------------
def test_library_exports_exactly_the_header():
    declared = _declared(HDR, "FLDR_RGB_API")
    assert declared == FUNCTIONS, sorted(declared)
    assert _syms(LIB, ["--defined-only"]) == declared
    import fldr_rgb
    assert set(fldr_rgb.EXPORTS) == declared and len(fldr_rgb.EXPORTS) == len(FUNCTIONS)
    import fldr_pack10
    assert {n.replace("fldr_pack10_", "fldr_rgb_") for n in fldr_pack10.EXPORTS} == declared - {"fldr_rgb_alpha"}


def test_library_links_only_the_model_api_and_names_no_other_library():
    dyn = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    needed = re.findall(r"NEEDED.*\[(libfldr_[a-z0-9_]+\.so)\]", dyn)
    assert needed == ["libfldr_model.so"], dyn
    assert re.search(r"R(UN)?PATH.*\$ORIGIN", dyn), dyn
    used = set(n for n in _syms(LIB, ["--undefined-only"]) if n.startswith("fldr_"))
    assert used and used <= _declared(os.path.join(INC, "fldr_model.h"), "FLDR_MODEL_API"), sorted(used)
    assert "fldr_model_forward" in used
    text = open(HDR).read().lower()
    strings = subprocess.run(["strings", LIB], capture_output=True, text=True, check=True).stdout.lower()
    names = [n.lower() for n in _syms(LIB, [])]
    for other in OTHER_LIBRARIES:
        assert other not in text and other not in strings and not [n for n in names if other in n], other


@pytest.mark.parametrize("compiler", [["gcc", "-std=c99", "-x", "c"], ["g++", "-std=c++11", "-x", "c++"]])
def test_header_is_plain_c99_and_cxx(compiler, tmp_path):
    assert shutil.which(compiler[0]), compiler[0] + " not installed"
    src = tmp_path / "h.c"
    src.write_text('#include "fldr_rgb.h"\nint main(void) { return fldr_rgb_sizeof(0) > 0 && sizeof(fldr_rgb_format) == 32 && '
                   'sizeof(fldr_rgb_frame) == 64 ? 0 : 1; }\n')
    r = subprocess.run(compiler + ["-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I" + INC, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "hip" not in re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S).lower()


def test_header_states_the_worked_words_the_alpha_numbers_and_what_is_out_of_scope():
    text = open(HDR).read()
    for s in ("0xFFF00001", "0xC01003FF", "128 at t = 0.5", "191 at t = 0.25", "rgb48", "rgba64", "r210", "x2rgb10be", "float formats",
              "premultiplied"):
        assert s in text, s


def test_binding_struct_sizes_version_and_codes():
    import fldr_rgb as V
    l = V.lib()
    assert l.fldr_rgb_version() == V.RGB_VERSION
    text = open(HDR).read()
    assert int(re.search(r"#define FLDR_RGB_VERSION (\d+)", text).group(1)) == V.RGB_VERSION
    for which, cls in enumerate((V.Format, V.Frame, V.IO, V.SessionConfig)):
        assert l.fldr_rgb_sizeof(which) == ctypes.sizeof(cls)
    assert ctypes.sizeof(V.Format) == 32 and ctypes.sizeof(V.Frame) == 64
    assert l.fldr_rgb_sizeof(4) == V.E_ARG
    for name, v in (("E_ARG", V.E_ARG), ("E_FORMAT", V.E_FORMAT), ("E_PITCH", V.E_PITCH), ("E_PLANE", V.E_PLANE),
                    ("E_WORKSPACE", V.E_WORKSPACE), ("E_DEVICE", V.E_DEVICE)):
        assert re.search(r"#define FLDR_RGB_%s\s+\((-?\d+)\)" % name, text).group(1) == str(v)
        assert v <= -900                                                       # below every other library's range
        assert l.fldr_rgb_error_string(v).decode().startswith("fldr_rgb")
    assert (V.E_ARG, V.E_FORMAT, V.E_PITCH, V.E_PLANE, V.E_WORKSPACE, V.E_DEVICE) == (-900, -901, -902, -903, -904, -905)
    assert l.fldr_rgb_error_string(-3).decode().startswith("fldr_model")      # model codes pass through
    for name, v in V.LAYOUTS.items():
        assert re.search(r"FLDR_RGB_%s = %d\b" % (name.upper(), v), text), name
    for name, v in V.ALPHAS.items():
        assert re.search(r"FLDR_RGB_ALPHA_%s = %d\b" % (name.upper(), v), text), name
    assert tuple(V.LAYOUTS) == R.LAYOUTS
    body = open(os.path.join(PKG, "rgb", "rgb_internal.h")).read()
    assert int(re.search(r"RUN_WORDS = (\d+)", body).group(1)) == V.RUN_WORDS
    for layout, depth in R.FORMATS:                                            # the binding's geometry is the oracle's
        fmt = V.Format(layout, depth)
        item = np.dtype(V.plane_dtype(fmt, numpy=True)).itemsize
        for W in range(1, 20):
            shapes = V.plane_shapes(fmt, 3, W)
            assert len(shapes) == R.planes(layout) and all(s == (3, R.row_bytes(layout, depth, W) // item) for s in shapes)


def test_example_builds_with_cc_prints_usage_and_rejects_bad_arguments(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    exe = tmp_path / "fldr_slowmo_rgb"
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + INC, "-o", str(exe), EXAMPLE_C, "-L" + PKG,
                        "-l:libfldr_rgb.so", "-l:libfldr_model.so", "-Wl,-rpath," + PKG], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    source = open(EXAMPLE_C).read()
    assert "hip" not in re.sub(r"/\*.*?\*/", "", source, flags=re.S).lower()
    for name in R.FFMPEG.values():                                             # every pixel format name of the usage is taken
        assert '"%s"' % name in source, name
    u = subprocess.run([str(exe)], capture_output=True, text=True)            # no arguments: usage, no device touched
    assert u.returncode == 2 and "usage" in u.stderr
    for bad in (["w.npz", "64", "64"], ["w.npz", "64", "64", "2"], ["w.npz", "64", "64", "1", "bgra"], ["w.npz", "1", "64", "2", "bgra"],
                ["w.npz", "64", "64", "2", "rgb24"], ["w.npz", "64", "64", "2", "x2rgb10be"], ["w.npz", "64", "64", "2", "bgra", "blend"],
                ["w.npz", "64", "64", "2", "bgra", "alpha=premultiplied"], ["w.npz", "64", "64", "2", "gbrap10le", "alpha=blend", "more"]):
        u = subprocess.run([str(exe)] + bad, capture_output=True, text=True)
        assert u.returncode == 2 and "usage" in u.stderr, bad


# ---- argument errors without a device ---------------------------------------------------------------------------------------------
def _io(V, fin=None, fout=None, H=64, W=64):
    fin = fin or V.Format()
    fout = fout or fin.copy()
    buf = np.zeros(H * W * 8 + 64, np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    io = V.IO()
    io.H, io.W = H, W
    io.in_format, io.out_format = fin.copy(), fout.copy()

    def fill(fr, fmt):
        item = np.dtype(V.plane_dtype(fmt, numpy=True)).itemsize
        for p, (_, n) in enumerate(V.plane_shapes(fmt, H, W)):
            fr.plane[p], fr.pitch[p] = base, n * item
    for f in range(2):
        fill(io.in_[f], fin)
    outs = (V.Frame * 1)()
    fill(outs[0], fout)
    io.n_t, io.t, io.out = 1, base, ctypes.cast(outs, ctypes.POINTER(V.Frame))
    io._keep = (buf, outs)
    return io


def _formats(V, alpha="opaque"):
    return [V.Format(l, d, alpha) for l, d in R.FORMATS]


def test_every_layout_depth_alpha_triple_is_accepted_and_every_other_is_a_format_error():
    import fldr_rgb as V
    l = V.lib()
    call = lambda io: l.fldr_rgb_forward(None, ctypes.byref(io), None, 0, None)
    assert len(_formats(V)) == 10
    create = lambda cfg: l.fldr_rgb_session_create(None, ctypes.byref(cfg), ctypes.byref(ctypes.c_void_p()))

    def session_code(fin, fout):
        cfg = V.SessionConfig()
        cfg.H, cfg.W, cfg.n_t = 64, 64, 1
        cfg.in_format, cfg.out_format = fin.copy(), fout.copy()
        return create(cfg)
    # the valid pairs: every format with itself under every policy, every pair under OPAQUE, NEARER / BLEND where the alpha widths agree
    # or the out layout has none; everything else about alpha is a format error, from the forward and from session_create alike
    for alpha in R_ALPHAS:
        for fin in _formats(V):
            for fout in _formats(V, alpha):
                bi, bo = R.alpha_bits(fin.name, fin.depth), R.alpha_bits(fout.name, fout.depth)
                ok = alpha == "opaque" or bo == 0 or bi == bo
                want = V.E_ARG if ok else V.E_FORMAT                           # valid io, no model
                assert call(_io(V, fin, fout)) == want, (fin.name, fin.depth, fout.name, fout.depth, alpha)
                assert session_code(fin, fout) == want, (fin.name, fin.depth, fout.name, fout.depth, alpha)
    io = _io(V, V.Format("bgra", 0), V.Format("abgr", 0, "blend"))             # depth 0 is 8 on the byte layouts
    assert call(io) == V.E_ARG
    # every other layout / depth pair, policy and reserved word
    bad_depths = {"bgra": (10, 16, 1), "rgba": (10,), "argb": (10,), "abgr": (10, 12), "x2rgb10": (8, 0, 12), "x2bgr10": (8, 0),
                  "gbrp": (0, 12, 16), "gbrap": (0, 9, 16)}
    for fmt in _formats(V):
        for side in ("in_format", "out_format"):
            fields = [("layout", 8), ("layout", -1), ("alpha", 3), ("alpha", -1)] + [("depth", d) for d in bad_depths[fmt.name]]
            for field, val in fields:
                io = _io(V, fmt); setattr(getattr(io, side), field, val)
                assert call(io) == V.E_FORMAT, (fmt.name, side, field, val)
            for w in range(5):
                io = _io(V, fmt); getattr(io, side).reserved[w] = 1
                assert call(io) == V.E_FORMAT
    # the converters refuse the same formats, before looking at anything else they would touch
    fr, bad = V.Frame(), V.Format("bgra", 10)
    buf = np.zeros(256, np.uint8)
    fr.plane[0], fr.pitch[0] = buf.ctypes.data, 64
    assert l.fldr_rgb_to_planar(ctypes.byref(fr), 1, ctypes.byref(bad), ctypes.c_void_p(buf.ctypes.data), 4, 4, None) == V.E_FORMAT
    assert l.fldr_rgb_from_planar(ctypes.c_void_p(buf.ctypes.data), ctypes.byref(bad), ctypes.byref(fr), 4, 4, None) == V.E_FORMAT


def test_pitch_plane_and_argument_errors_before_any_device_call():
    import fldr_rgb as V
    l = V.lib()
    call = lambda io: l.fldr_rgb_forward(None, ctypes.byref(io), None, 0, None)
    W = 63
    for fmt in _formats(V):
        rb = R.row_bytes(fmt.name, fmt.depth, W)
        unit = 4 if fmt.layout <= 5 else 2 if fmt.depth == 10 else 1          # what planes and pitches are multiples of
        np_ = R.planes(fmt.name)
        assert _io(V, fmt, W=W).in_[0].pitch[0] == rb
        assert call(_io(V, fmt, W=W)) == V.E_ARG
        for p in range(np_):
            io = _io(V, fmt, W=W); io.in_[1].pitch[p] = rb - unit             # shorter than the row
            assert call(io) == V.E_PITCH
            io = _io(V, fmt, W=W); io.out[0].pitch[p] = rb - unit
            assert call(io) == V.E_PITCH
            for extra in (1, 2, 3, 4):                                         # long enough: the unit decides
                io = _io(V, fmt, W=W); io.in_[0].pitch[p] = rb + extra
                assert call(io) == (V.E_ARG if extra % unit == 0 else V.E_PITCH), (fmt.name, fmt.depth, p, extra)
                io = _io(V, fmt, W=W); io.out[0].pitch[p] = rb + extra
                assert call(io) == (V.E_ARG if extra % unit == 0 else V.E_PITCH), (fmt.name, fmt.depth, p, extra)
            io = _io(V, fmt, W=W); io.in_[0].plane[p] = None
            assert call(io) == V.E_PLANE
            io = _io(V, fmt, W=W); io.out[0].plane[p] = None
            assert call(io) == V.E_PLANE
            for side in ("in", "out"):
                for off in (1, 2, 4):
                    io = _io(V, fmt, W=W)
                    fr = io.in_[1] if side == "in" else io.out[0]
                    fr.plane[p] = fr.plane[p] + off
                    assert call(io) == (V.E_ARG if off % unit == 0 else V.E_PLANE), (fmt.name, fmt.depth, side, p, off)
        # two faults at once: every plane and then every pitch by the sample size (null, too short, odd at depth 10), then every plane and
        # then every pitch by the word layouts' unit of 4
        for p in range(np_):
            for side in ("in", "out"):
                def two(off, pitch, pitch_plane=p):
                    io = _io(V, fmt, W=W)
                    fr = io.in_[1] if side == "in" else io.out[0]
                    fr.plane[p] = fr.plane[p] + off if off is not None else None
                    fr.pitch[pitch_plane] = pitch
                    return call(io)
                where = (fmt.name, fmt.depth, side, p)
                assert two(2, rb - unit) == V.E_PITCH, where                   # an address = 2 mod 4 and a short pitch: the pitch
                assert two(1, rb - unit) == (V.E_PLANE if fmt.depth == 10 else V.E_PITCH), where   # odd: a fault of 16-bit samples only
                assert two(2, rb + 2) == (V.E_PLANE if unit == 4 else V.E_ARG), where              # both = 2 mod 4, the pitch covers the row
                assert two(4, rb + 2) == (V.E_PITCH if unit == 4 else V.E_ARG), where
                assert two(None, rb - unit) == V.E_PLANE, where                # a null plane and a bad pitch: the plane
                assert two(None, rb + 1, 0) == V.E_PLANE, where                # ... whichever plane has the bad pitch
                assert two(None, rb - unit, np_ - 1) == V.E_PLANE, where
        for p in range(np_, 4):                                                # only the layout's planes are looked at
            io = _io(V, fmt, W=W); io.in_[0].plane[p] = None; io.in_[0].pitch[p] = 0; io.out[0].plane[p] = None
            assert call(io) == V.E_ARG
        io = _io(V, fmt); io.n_t = 0
        assert call(io) == V.E_ARG
        io = _io(V, fmt); io.t = None
        assert call(io) == V.E_ARG
        io = _io(V, fmt); io.W = 1
        assert call(io) == V.E_ARG
        io = _io(V, fmt); io.out = None
        assert call(io) == V.E_ARG
    assert l.fldr_rgb_forward(None, None, None, 0, None) == V.E_ARG
    assert l.fldr_rgb_workspace_bytes(None, 64, 64, 1) == V.E_ARG
    # the converters alone
    buf = np.zeros(4096 + 64, np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    ok = ctypes.c_void_p(base)
    for fmt in (V.Format("bgra"), V.Format("x2rgb10"), V.Format("gbrap", 10)):
        rb = R.row_bytes(fmt.name, fmt.depth, 8)
        fr = V.Frame()
        for p in range(R.planes(fmt.name)):
            fr.plane[p], fr.pitch[p] = base, rb
        to = lambda fr_, planar, H=4, W=8, n=1: l.fldr_rgb_to_planar(ctypes.byref(fr_), n, ctypes.byref(fmt), planar, H, W, None)
        frm = lambda fr_, planar, H=4, W=8: l.fldr_rgb_from_planar(planar, ctypes.byref(fmt), ctypes.byref(fr_), H, W, None)
        assert to(fr, None) == V.E_ARG and frm(fr, None) == V.E_ARG
        assert to(fr, ok, H=0) == V.E_ARG and frm(fr, ok, W=0) == V.E_ARG and to(fr, ok, n=0) == V.E_ARG
        if fmt.depth == 10:                                                    # uint16 planar frames at an odd address
            assert to(fr, ctypes.c_void_p(base + 1)) == V.E_ARG and frm(fr, ctypes.c_void_p(base + 1)) == V.E_ARG
        last = R.planes(fmt.name) - 1
        fr.pitch[last] = rb - 4
        assert to(fr, ok) == V.E_PITCH and frm(fr, ok) == V.E_PITCH
        fr.pitch[last] = rb + 1
        assert to(fr, ok) == V.E_PITCH and frm(fr, ok) == V.E_PITCH
        fr.pitch[last] = rb; fr.plane[last] = base + 1
        assert to(fr, ok) == V.E_PLANE and frm(fr, ok) == V.E_PLANE


def test_alpha_pass_argument_errors_before_any_device_call():
    import fldr_rgb as V
    l = V.lib()
    buf = np.zeros(4096 + 64, np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16

    def frames(fmt, n, W=8):
        arr = (V.Frame * n)()
        for fr in arr:
            for p in range(R.planes(fmt.name)):
                fr.plane[p], fr.pitch[p] = base, R.row_bytes(fmt.name, fmt.depth, W)
        return arr

    def call(fin, fout, fi=None, fo=None, n=1, t=base, H=4, W=8):
        fi = frames(fin, 2) if fi is None else fi
        fo = frames(fout, max(n, 1)) if fo is None else fo
        return l.fldr_rgb_alpha(fi, ctypes.byref(fin), fo, n, ctypes.byref(fout), ctypes.c_void_p(t) if t else None, H, W, None)
    bgra, blend = V.Format("bgra"), V.Format("bgra", alpha="blend")
    assert call(bgra, bgra) == 0 and call(bgra, V.Format("gbrp", 10, "nearer")) == 0      # OPAQUE / nowhere to put alpha: nothing to enqueue
    assert call(V.Format("gbrp"), V.Format("x2rgb10")) == 0
    assert call(bgra, blend, n=0) == V.E_ARG and call(bgra, blend, t=None) == V.E_ARG and call(bgra, blend, H=0) == V.E_ARG
    assert l.fldr_rgb_alpha(None, ctypes.byref(bgra), frames(bgra, 1), 1, ctypes.byref(blend), ctypes.c_void_p(base), 4, 8, None) == V.E_ARG
    assert l.fldr_rgb_alpha(frames(bgra, 2), ctypes.byref(bgra), None, 1, ctypes.byref(blend), ctypes.c_void_p(base), 4, 8, None) == V.E_ARG
    for fin, fout in ((V.Format("gbrp"), blend), (V.Format("x2rgb10"), blend), (bgra, V.Format("gbrap", 10, "nearer")),
                      (V.Format("bgra", 10), blend), (bgra, V.Format("bgra", alpha=3))):
        assert call(fin, fout) == V.E_FORMAT, (fin.name, fout.name)
    fi = frames(bgra, 2); fi[1].pitch[0] = 28
    assert call(bgra, blend, fi=fi) == V.E_PITCH
    fo = frames(V.Format("gbrap"), 3); fo[2].plane[3] = None
    assert call(bgra, V.Format("gbrap", alpha="nearer"), fo=fo, n=3) == V.E_PLANE
    fo = frames(blend, 1); fo[0].plane[0] = base + 2
    assert call(bgra, blend, fo=fo) == V.E_PLANE


def test_workspace_and_session_argument_errors_before_any_device_call():
    import fldr_rgb as V
    l = V.lib()
    h = ctypes.c_void_p()
    cfg = V.SessionConfig()
    cfg.H, cfg.W, cfg.n_t = 64, 64, 1
    cfg.in_format, cfg.out_format = V.Format("argb"), V.Format("gbrap", 8, "blend")
    create = lambda: l.fldr_rgb_session_create(None, ctypes.byref(cfg), ctypes.byref(h))
    assert create() == V.E_ARG
    cfg.reserved[1] = 1
    assert create() == V.E_FORMAT
    cfg.reserved[1] = 0
    cfg.out_format.depth = 10                                                  # 8-bit alpha in, 10-bit alpha out
    assert create() == V.E_FORMAT
    cfg.out_format.alpha = 0
    assert create() == V.E_ARG
    cfg.out_format.depth = 12
    assert create() == V.E_FORMAT
    cfg.out_format.depth = 8
    cfg.in_format.layout = 8
    assert create() == V.E_FORMAT
    cfg.in_format.layout = 0
    cfg.n_t = 0
    assert create() == V.E_ARG
    assert l.fldr_rgb_session_create(None, None, ctypes.byref(h)) == V.E_ARG
    assert l.fldr_rgb_session_push(None, None, None, None) == V.E_ARG and l.fldr_rgb_session_reset(None) == V.E_ARG
    l.fldr_rgb_session_destroy(None)
    assert l.fldr_rgb_workspace_bytes(None, 64, 64, 1) == V.E_ARG
    assert l.fldr_rgb_error_string(V.E_WORKSPACE).decode().startswith("fldr_rgb: workspace")


# ---- the listing ----------------------------------------------------------------------------------------------------------------
def test_kernels_use_no_scratch_no_lds_and_leave_four_waves_per_simd():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    ks = KR.kernels(LIB)
    names = [k["name"] for k in ks]
    # word layouts: one input and one output kernel for six layouts in two forms; planes: two sample types in two forms; alpha: five
    # pairs of places in two forms
    for stem, n in (("rgb_words_to_planar_kernel", 12), ("rgb_words_from_planar_kernel", 12), ("rgb_planes_kernel", 4), ("rgb_alpha_kernel", 10)):
        assert sum(stem in name for name in names) == n, names
    assert len(ks) == 38
    for k in ks:
        assert k["scratch"] == 0 and k["vgpr_spills"] == 0 and k["sgpr_spills"] == 0 and k["lds"] == 0, k
        assert k["vgpr"] + k["agpr"] <= 128, k                                 # 512 / 128: four waves per SIMD


def test_listing_has_the_wide_accesses_and_no_stale_half_packing():
    """v_ashr_pk_* / v_cvt_pk_[ui]16_* leave upper bits stale on gfx950 (video/yuv_run_device.h): none may be in the library; the wide
    forms show as 16-byte loads and stores, the byte shuffles as v_perm_b32."""
    texts = _disassemble(LIB)
    assert texts and any("rgb_words_to_planar_kernel" in t and "rgb_words_from_planar_kernel" in t and "rgb_alpha_kernel" in t for t in texts)
    n = sum(len(re.findall(r"\bv_ashr_pk_\w+|\bv_cvt_pk_[ui]16_\w+", t)) for t in texts)
    assert n == 0
    for ins in ("global_load_dwordx4", "global_store_dwordx4", "v_perm_b32"):
        assert any(ins in t for t in texts), ins


def test_no_unsafe_packed_fp32_in_the_library():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_pk_opsel.py"), LIB], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


# ---- the layouts and the alpha rules (the oracle alone) ---------------------------------------------------------------------------
def test_the_two_worked_words():
    one = lambda v: np.array([[v]])
    for layout, word in (("x2rgb10", 0xFFF00001), ("x2bgr10", 0xC01003FF)):
        got = R.pack(layout, 10, b=one(1), g=one(0), r=one(1023), a=one(3))[0]
        assert got.dtype == np.uint32 and got.tolist() == [[word]], (layout, hex(int(got[0, 0])))
        b, g, r, a = R.unpack(layout, 10, (np.array([[word]], np.uint32),))
        assert (int(b[0, 0]), int(g[0, 0]), int(r[0, 0]), int(a[0, 0])) == (1, 0, 1023, 3)
    assert R.pack("x2rgb10", 10, one(1), one(0), one(1023))[0].tobytes() == bytes([0x01, 0x00, 0xF0, 0xFF])      # little-endian, opaque
    # the byte layouts are their names in memory
    for layout in ("bgra", "rgba", "argb", "abgr"):
        ch = {"b": 1, "g": 2, "r": 3, "a": 4}
        got = R.pack(layout, 8, one(1), one(2), one(3), one(4))[0]
        assert got.dtype == np.uint8 and got.tolist() == [[ch[c] for c in layout]]
    g_, b_, r_, a_ = R.pack("gbrap", 10, one(1), one(2), one(3), one(4))       # planes G, B, R, A
    assert (int(g_[0, 0]), int(b_[0, 0]), int(r_[0, 0]), int(a_[0, 0])) == (2, 1, 3, 4) and g_.dtype == np.uint16
    assert len(R.pack("gbrp", 8, one(1), one(2), one(3))) == 3


@pytest.mark.parametrize("layout,depth", R.FORMATS)
def test_pack_and_unpack_are_inverse_and_dirt_stays_out_of_the_values(layout, depth):
    g = np.random.default_rng(3)
    top = 1 << depth
    for W in list(range(1, 10)) + [31, 32, 33]:
        for H in (1, 3):
            b, gr, r = (g.integers(0, top, (H, W)).astype(R.sample_dtype(depth)) for _ in range(3))
            bits = R.alpha_bits(layout, depth)
            a = g.integers(0, 1 << bits, (H, W)) if bits else None
            frame = R.pack(layout, depth, b, gr, r, a)
            assert len(frame) == R.planes(layout)
            for p in frame:
                assert p.shape[0] == H and p.shape[1] * p.itemsize == R.row_bytes(layout, depth, W)
            for got, want in zip(R.unpack(layout, depth, frame), (b, gr, r, a)):
                assert (got is None and want is None) or np.array_equal(got, want), (layout, depth, W)
            assert np.array_equal(R.planar_bgr(layout, depth, frame), np.stack([b, gr, r]))
            # dirt: bits 10-15 of a planar 16-bit word; the alpha a colour reader ignores
            dirty = R.pack(layout, depth, b, gr, r, a, dirt=g)
            if layout in R.PLANES and depth == 10:
                assert not np.array_equal(dirty[0], frame[0])
            assert np.array_equal(R.planar_bgr(layout, depth, dirty), np.stack([b, gr, r]))
            if bits:
                other = R.pack(layout, depth, b, gr, r, g.integers(0, 1 << bits, (H, W)))
                assert np.array_equal(R.planar_bgr(layout, depth, other), np.stack([b, gr, r]))
                opaque = R.unpack(layout, depth, R.pack(layout, depth, b, gr, r))[3]
                assert (opaque == R.alpha_max(layout, depth)).all() and R.alpha_max(layout, depth) in (255, 1023, 3)


def test_the_alpha_rules_and_their_worked_numbers():
    a0, a1 = np.array([[255, 0, 7]]), np.array([[0, 255, 9]])
    assert R.alpha_blend(a0, a1, 0.5).tolist() == [[128, 128, 8]]
    assert R.alpha_blend(a0, a1, 0.25).tolist() == [[191, 64, 8]]            # 7.5 + 0.5 -> 8
    assert R.alpha_blend(a0, a1, 0.0).tolist() == a0.tolist() and R.alpha_blend(a0, a1, 1.0).tolist() == a1.tolist()
    assert R.alpha_blend(a0, a1, -0.25).tolist() == a0.tolist()                # a negative time and NaN: w = 0
    assert R.alpha_blend(a0, a1, float("nan")).tolist() == a0.tolist()
    assert R.alpha_blend(a0, a1, 7.0).tolist() == a1.tolist()                  # w stops at 65536
    assert [R.blend_weight(t) for t in (0.0, 0.25, 0.5, 1.0, 2.0, -1.0, float("nan"), float("inf"))] == [0, 16384, 32768, 65536, 65536, 0, 0, 65536]
    assert R.blend_weight(np.float32(1.0 / 3.0)) == int(np.rint(np.float32(1.0 / 3.0) * np.float32(65536)))
    assert R.alpha_blend(np.array([[1023]]), np.array([[1023]]), 0.3).tolist() == [[1023]]      # no overflow in uint32 at 10 bits
    assert R.alpha_nearer(a0, a1, 0.25).tolist() == a0.tolist() and R.alpha_nearer(a0, a1, 0.5).tolist() == a1.tolist()
    assert R.alpha_nearer(a0, a1, np.nextafter(np.float32(0.5), np.float32(0))).tolist() == a0.tolist()
    assert R.alpha_nearer(a0, a1, float("nan")).tolist() == a1.tolist()
    assert [R.alpha_max(l, d) for l, d in (("bgra", 8), ("x2rgb10", 10), ("gbrap", 10), ("gbrap", 8))] == [255, 3, 1023, 255]
    assert R.alpha_bits("gbrp", 8) == 0 and R.alpha_bits("gbrp", 10) == 0
