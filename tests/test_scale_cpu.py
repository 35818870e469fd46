"""CPU checks of the scale API (include/fldr_scale.h, libfldr_scale.so): the library's symbol table and link, the header as plain C99 /
C++, the C example, the code-generation guards, the binding's struct mirrors, the tables against the float64 statement of
tests/scale_oracle.py, the limits, the argument checks of the map, the kernel entry, the forward and the stream — which happen before any
device call, so they run without a GPU —, the table builder as a stand-alone program under the host sanitizers, and the oracle alone on
hand-worked rows."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import scale_oracle as O
from lib_checks import declared as _declared, syms as _syms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fldr-vfi_amd")
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "fldr_scale.h")
LIB = os.path.join(PKG, "libfldr_scale.so")
EXAMPLE = os.path.join(ROOT, "examples", "fldr_scale.c")
BARRED = ("fldr_field", "fldr_chroma", "fldr_cadence", "fldr_repeat", "fldr_pipe", "fldr_pulldown", "fldr_probe", "fldr_interlace")
NAMES = ("version", "error_string", "sizeof", "taps_count", "taps", "map_create", "map_destroy", "frame", "workspace_bytes", "temp_frame", "forward",
         "create", "max_out", "push", "flush", "reset", "destroy")
FILTERS = (O.BILINEAR, O.BICUBIC, O.LANCZOS3)
KINDS = (O.LUMA, O.CHROMA_H, O.CHROMA_V)
PAIRS = [(1, 1), (1, 9), (9, 1), (2, 5), (5, 2), (16, 17), (17, 16), (64, 16), (48, 5), (480, 576), (576, 480), (720, 1080), (1080, 2160),
         (2160, 1080), (16384, 16384), (16384, 1537), (33, 32), (200, 19)]


# ---- the library ------------------------------------------------------------------------------------------------------------------------
def test_library_exports_exactly_the_header():
    declared = _declared(HDR, "FLDR_SCALE_API")
    assert len(NAMES) == 17 and declared == set("fldr_scale_" + n for n in NAMES), sorted(declared)
    assert _syms(LIB, ["--defined-only"]) == declared
    import fldr_scale
    assert set(fldr_scale.EXPORTS) == declared


def test_library_links_only_the_rate_video_and_model_apis():
    dyn = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    needed = set(re.findall(r"NEEDED.*\[(libfldr_\w+\.so)\]", dyn))
    assert needed == {"libfldr_rate.so", "libfldr_video.so"}, dyn
    assert re.search(r"R(UN)?PATH.*\[\$ORIGIN\b", dyn), dyn
    used = set(n for n in _syms(LIB, ["--undefined-only"]) if n.startswith("fldr_"))
    allowed = (_declared(os.path.join(INC, "fldr_rate.h"), "FLDR_RATE_API") | _declared(os.path.join(INC, "fldr_video.h"), "FLDR_VIDEO_API") |
               _declared(os.path.join(INC, "fldr_model.h"), "FLDR_MODEL_API"))
    assert used and used <= allowed, sorted(used)
    assert {"fldr_rate_forward", "fldr_video_forward", "fldr_rate_workspace_bytes", "fldr_rate_error_string", "fldr_scene_measure"} <= used
    assert not used & {"fldr_rate_create", "fldr_rate_push", "fldr_rate_flush"}          # the stream is this library's own: it holds two sizes


def test_header_and_library_name_none_of_the_libraries_beside_them():
    text = open(HDR).read().lower()
    raw = open(LIB, "rb").read().lower()
    for other in BARRED:
        assert other not in text and other.encode() not in raw, other
    for name in os.listdir(INC):
        if name != "fldr_scale.h":
            assert "fldr_scale" not in open(os.path.join(INC, name)).read().lower(), name
    for name in os.listdir(PKG):
        if re.fullmatch(r"libfldr_\w+\.so", name) and name != "libfldr_scale.so":
            assert b"fldr_scale" not in open(os.path.join(PKG, name), "rb").read(), name


@pytest.mark.parametrize("compiler", [["gcc", "-std=c99", "-x", "c"], ["g++", "-std=c++11", "-x", "c++"]])
def test_header_is_plain_c99_and_cxx(compiler, tmp_path):
    assert shutil.which(compiler[0]), compiler[0] + " not installed"
    src = tmp_path / "h.c"
    src.write_text('#include <stddef.h>\n#include "fldr_scale.h"\nint main(void) { fldr_scale_config c; fldr_scale_map m; fldr_scale_io io;\n'
                   '  fldr_scale_map_config mc; c.where = FLDR_SCALE_AUTO; m.live = 0; io.scene = 1; mc.filter = FLDR_SCALE_LANCZOS3;\n'
                   '  return fldr_scale_sizeof(3) == (int)sizeof(c) && c.where == 2 && m.live == 0 && io.scene == 1 && mc.filter == 2 &&\n'
                   '         FLDR_SCALE_BILINEAR == 0 && FLDR_SCALE_BICUBIC == 1 && FLDR_SCALE_BEFORE == 0 && FLDR_SCALE_AFTER == 1 &&\n'
                   '         FLDR_SCALE_MAX_TAPS == 64 && FLDR_SCALE_MAX_SIZE == 16384 && FLDR_SCALE_CHROMA_V == 2 &&\n'
                   '         offsetof(fldr_scale_config, out_H) == sizeof(fldr_rate_config) && offsetof(fldr_scale_io, scene) == sizeof(fldr_video_io) ? 0 : 1; }\n')
    r = subprocess.run(compiler + ["-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I" + INC, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "hip" not in re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S).lower()


def test_header_defines_no_error_code_and_says_whose_it_returns():
    text = open(HDR).read()
    assert not re.findall(r"#define\s+FLDR_[A-Z0-9]+_E_[A-Z]+", text)
    for s in ("defines no code of its own", "FLDR_RATE_E_ARG", "FLDR_RATE_E_STATE", "FLDR_RATE_E_RATIO", "FLDR_RATE_E_DEVICE",
              "fldr_scale_error_string is fldr_rate_error_string"):
        assert s in text, s
    import fldr_scale as K
    import fldr_rate as R
    l = K.lib()
    for code in (R.E_ARG, R.E_STATE, R.E_RATIO, R.E_DEVICE, -101, -3, 0, -999):
        assert l.fldr_scale_error_string(code) == R.lib().fldr_rate_error_string(code)
    assert (K.E_ARG, K.E_STATE, K.E_RATIO, K.E_DEVICE) == (R.E_ARG, R.E_STATE, R.E_RATIO, R.E_DEVICE)


def test_header_states_the_rule_the_limits_and_what_is_out_of_scope():
    text = open(HDR).read()
    for s in ("EXACTLY 16384", "c = (o + 1/2) r - 1/2", "c = o r + (r - 1) / 4", "left = floor(c) - n/2 + 1", "half to even", "the lowest k among equals",
              "(1 << (13 - e))) >> (14 - e)", "(1 << (13 + e))) >> (14 + e)", "sum|q| > 32767", "FLDR_SCALE_MAX_SIZE = 16384", "FLDR_SCALE_MAX_TAPS = 64",
              "at\n *   most 10.66", "no linear-light scaling and no ringing control", 'chroma siting is "left" only',
              "4:2:2, 4:4:4, packed and RGB formats are out of scope", "no cropping or aspect handling", "the stream is synchronous",
              "the host's sin", "equal pixel counts resolve to AFTER", "Checked in this order", "Validation order"):
        assert s in text, s


def test_example_builds_with_cc(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    exe = tmp_path / "fldr_scale"
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + INC, "-o", str(exe), EXAMPLE, "-L" + PKG,
                        "-l:libfldr_scale.so", "-l:libfldr_rate.so", "-l:libfldr_video.so", "-l:libfldr_model.so", "-Wl,-rpath," + PKG],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    src = open(EXAMPLE).read()
    assert "hip" not in re.sub(r"/\*.*?\*/", "", src, flags=re.S).lower()
    u = subprocess.run([str(exe)], capture_output=True, text=True)            # no arguments: usage, no device touched
    assert u.returncode == 2 and "usage" in u.stderr and "filter=bilinear|bicubic|lanczos" in u.stderr and "where=auto|before|after" in u.stderr
    assert "out=WxH" in u.stderr
    for bad in (["w.npz", "64", "64", "24", "60"],                            # no out=
                ["w.npz", "64", "64", "24", "60", "filter=bicubic"],
                ["w.npz", "64", "1", "24", "60", "out=128x128"],
                ["w.npz", "64", "64", "24", "60", "out=0x128"],
                ["w.npz", "64", "64", "24/0", "60", "out=128x128"],
                ["w.npz", "64", "64", "24", "x", "out=128x128"],
                ["w.npz", "64", "64", "24", "60", "out=128"],
                ["w.npz", "64", "64", "24", "60", "out=128x"],
                ["w.npz", "64", "64", "24", "60", "out=128x16385"],
                ["w.npz", "64", "64", "24", "60", "out=128x128", "filter=sharp"],
                ["w.npz", "64", "64", "24", "60", "out=128x128", "where=both"],
                ["w.npz", "1100", "64", "24", "60", "out=100x64"],             # 66 taps under the default Lanczos3
                ["w.npz", "64", "64", "24", "60", "out=128x128", "p12"],
                ["-", "64", "64", "24", "60", "out=128x128"]):                 # frames to interpolate and no weights
        u = subprocess.run([str(exe)] + bad, capture_output=True, text=True)
        assert u.returncode == 2 and "usage" in u.stderr, bad


def test_no_unsafe_packed_fp32_in_the_scale_library():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_pk_opsel.py"), LIB], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_kernels_use_no_scratch_and_stay_inside_the_lds_limit():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    ks = KR.kernels(LIB)
    assert len(ks) == 6, [k["name"] for k in ks]          # sample form x direct / staged read; both access forms, both passes and every plane in each
    for k in ks:
        assert "scale_kernel" in k["name"], k["name"]
        assert k.get("scratch", -1) == 0 and k.get("vgpr_spills", -1) == 0 and k.get("sgpr_spills", -1) == 0 and k.get("lds", 0) <= 65536, k


def test_binding_struct_sizes_and_version():
    import fldr_scale as K
    l = K.lib()
    text = open(HDR).read()
    assert l.fldr_scale_version() == K.SCALE_VERSION == int(re.search(r"#define FLDR_SCALE_VERSION (\d+)", text).group(1)) == 100
    for which, cls in enumerate((K.MapConfig, K.MapStruct, K.ScaleIO, K.ScaleConfig)):
        assert l.fldr_scale_sizeof(which) == ctypes.sizeof(cls)
    assert ctypes.sizeof(K.ScaleConfig) == ctypes.sizeof(K.RateConfig) + 32 and K.ScaleIO.scene.offset == ctypes.sizeof(K.IO)
    assert l.fldr_scale_sizeof(4) == K.E_ARG and l.fldr_scale_sizeof(-1) == K.E_ARG
    for macro, v in (("FLDR_SCALE_BILINEAR", K.BILINEAR), ("FLDR_SCALE_BICUBIC", K.BICUBIC), ("FLDR_SCALE_LANCZOS3", K.LANCZOS3),
                     ("FLDR_SCALE_LUMA", K.LUMA), ("FLDR_SCALE_CHROMA_H", K.CHROMA_H), ("FLDR_SCALE_CHROMA_V", K.CHROMA_V),
                     ("FLDR_SCALE_BEFORE", K.BEFORE), ("FLDR_SCALE_AFTER", K.AFTER), ("FLDR_SCALE_AUTO", K.AUTO),
                     ("FLDR_SCALE_READ_AUTO", K.READ_AUTO), ("FLDR_SCALE_READ_DIRECT", K.READ_DIRECT), ("FLDR_SCALE_READ_STAGED", K.READ_STAGED),
                     ("FLDR_SCALE_MAX_SIZE", K.MAX_SIZE), ("FLDR_SCALE_MAX_TAPS", K.MAX_TAPS)):
        assert int(re.search(r"#define %s\s+(\d+)" % macro, text).group(1)) == v, macro
    assert int(re.search(r"#define FLDR_SCALE_MAP_LIVE\s+(0x[0-9a-f]+)", text).group(1), 16) == K.MAP_LIVE
    assert (K.BILINEAR, K.BICUBIC, K.LANCZOS3, K.LUMA, K.CHROMA_H, K.CHROMA_V, K.BEFORE, K.AFTER, K.AUTO) == \
        (O.BILINEAR, O.BICUBIC, O.LANCZOS3, O.LUMA, O.CHROMA_H, O.CHROMA_V, O.BEFORE, O.AFTER, O.AUTO)


# ---- the tables ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("luma_in,luma_out", PAIRS)
def test_tables_against_the_float64_statement(luma_in, luma_out, filt):
    import fldr_scale as K
    n_want = O.taps_count(luma_in, luma_out, filt)
    if n_want > O.MAX_TAPS:
        assert K.taps_count(luma_in, luma_out, filt) == K.E_ARG
        return
    for kind in KINDS:
        n, left, coef = K.taps(luma_in, luma_out, filt, kind)
        nf, lf, x = O.taps_float(luma_in, luma_out, filt, kind)
        assert n == nf == n_want and left.tolist() == lf and coef.shape == (O.outputs(luma_out, kind), n)
        q = coef.astype(np.int64)
        assert (q.sum(axis=1) == 16384).all()
        assert np.abs(q).sum(axis=1).max() <= 32767
        # every tap within 1 of x_k; one tap of a row, a largest one, may carry the residual: a sum of n rounding errors of at most 1/2
        d = np.abs(q - x)
        over = d > 1
        assert (over.sum(axis=1) <= 1).all()
        for r in np.nonzero(over.any(axis=1))[0]:
            k = int(over[r].argmax())
            assert x[r, k] >= x[r].max() - 1 and d[r, k] <= 1 + n / 2, (kind, r, k)
        if luma_in == luma_out:
            assert ((q == 16384).sum(axis=1) == 1).all() and ((q != 0).sum(axis=1) == 1).all()
            assert (left + q.argmax(axis=1) == np.arange(len(left))).all()                    # ... and the one tap is the output's own index


def test_tap_counts_by_hand():
    import fldr_scale as K
    assert [K.taps_count(1080, 2160, f) for f in FILTERS] == [2, 4, 6]
    assert [K.taps_count(2160, 1080, f) for f in FILTERS] == [4, 8, 12]
    assert [K.taps_count(3, 2, f) for f in FILTERS] == [4, 6, 10]                             # ceil(1.5 a)
    assert K.taps_count(200, 19, K.LANCZOS3) == 64 and K.taps_count(31, 3, K.LANCZOS3) == 62     # ceil(3 x 200 / 19) = 32, ceil(31) = 31
    assert K.taps_count(1024, 32, K.BILINEAR) == 64 and K.taps_count(1025, 32, K.BILINEAR) == K.E_ARG


def test_chroma_column_centre_by_hand():
    """4:2:0 "left": chroma column o sits on luma column 2 o.  2x up, r = 1/2: c = o/2 - 1/8, so output 0 lies an eighth LEFT of source 0
    (a plain per-plane resize would put it a quarter left) and bilinear gives 1/8, 7/8 over sources -1, 0.  2x down, r = 2: c = 2 o + 1/4."""
    import fldr_scale as K
    for o in range(5):
        assert O.centre(4, 8, O.CHROMA_H, o) == Fraction(o, 2) - Fraction(1, 8)
        assert O.centre(8, 4, O.CHROMA_H, o) == 2 * o + Fraction(1, 4)
        assert O.centre(4, 8, O.CHROMA_V, o) == O.centre(4, 8, O.LUMA, o) == Fraction(2 * o + 1, 4) - Fraction(1, 2)
    n, left, coef = K.taps(4, 8, K.BILINEAR, K.CHROMA_H)
    assert n == 2 and left.tolist() == [-1, 0, 0, 1] and coef.tolist() == [[2048, 14336], [10240, 6144]] * 2      # 1/8 7/8; 5/8 3/8
    n, left, coef = K.taps(8, 4, K.BILINEAR, K.CHROMA_H)
    assert n == 4 and left.tolist() == [-1, 1] and coef.tolist() == [[3072, 7168, 5120, 1024]] * 2      # (3/8 7/8 5/8 1/8) / 2
    n, left, coef = K.taps(8, 4, K.BILINEAR, K.LUMA)
    assert left.tolist() == [-1, 1, 3, 5] and coef.tolist() == [[2048, 6144, 6144, 2048]] * 4           # c = 2 o + 1/2: symmetric


def test_limits():
    import fldr_scale as K
    for f in FILTERS:
        for a, b in ((0, 8), (8, 0), (16385, 8), (8, 16385), (-1, 8)):
            assert K.taps_count(a, b, f) == K.E_ARG, (a, b)
        assert K.taps_count(16384, 16384, f) == 2 * (f + 1) and K.taps_count(1, 16384, f) == 2 * (f + 1)
    assert K.taps_count(8, 8, 3) == K.E_ARG and K.taps_count(8, 8, -1) == K.E_ARG
    assert K.taps_count(1100, 100, K.LANCZOS3) == K.E_ARG                     # 2 ceil(33) = 66
    assert K.taps_count(1066, 100, K.LANCZOS3) == 64 and K.taps_count(1067, 100, K.LANCZOS3) == K.E_ARG       # "shrinks by at most 10.66"
    l = K.lib()
    left, coef = np.zeros(8, np.int32), np.zeros((8, 64), np.int16)
    ok = lambda *a: l.fldr_scale_taps(*a)
    assert ok(8, 8, 0, 0, left.ctypes.data, coef.ctypes.data) == 0
    assert ok(8, 8, 0, 3, left.ctypes.data, coef.ctypes.data) == K.E_ARG and ok(8, 8, 0, -1, left.ctypes.data, coef.ctypes.data) == K.E_ARG
    assert ok(8, 8, 0, 0, None, coef.ctypes.data) == K.E_ARG and ok(8, 8, 0, 0, left.ctypes.data, None) == K.E_ARG
    assert ok(1100, 100, 2, 0, left.ctypes.data, coef.ctypes.data) == K.E_ARG and ok(0, 8, 0, 0, left.ctypes.data, coef.ctypes.data) == K.E_ARG


def test_table_builder_alone_under_the_host_sanitizers(tmp_path):
    """scale/scale_taps.h is host-only: a stand-alone program with its own main, built with -fsanitize=undefined,address, walks sizes 1 and
    16384, both tap limits and every kind and filter, and checks the row sums."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "scale_taps_main"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                        "-Wno-unused-function", "-I" + INC, "-I" + os.path.join(PKG, "scale"), "-o", str(exe), os.path.join(ROOT, "tests", "scale_taps_main.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    u = subprocess.run([str(exe)], capture_output=True, text=True)
    assert u.returncode == 0 and "tables ok" in u.stdout, u.stdout + u.stderr


# ---- argument errors without a device -----------------------------------------------------------------------------------------------------
H0, W0, H1, W1 = 64, 48, 96, 80


def _host(V, layout, depth, H, W, count):
    """`count` frames whose planes all point into one zeroed, 256-byte aligned host buffer, each frame in a part of its own."""
    b = 2 if depth == 10 else 1
    part = (H + 1) * (W + 1) * 2 * b
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


def _fake_map(K, V, layout, depth, where=None, in_size=(H0, W0), out_size=(H1, W1)):
    """A fldr_scale_map as the create fills it, but with host memory for tables: good for every check that comes before a launch."""
    m = K.MapStruct()
    m.cfg = K.map_config(in_size, out_size, V.Format(layout, depth=depth), K.BICUBIC, K.AUTO if where is None else where)
    m.where = O.where(K.AUTO if where is None else where, in_size, out_size)
    m.taps_x = m.taps_y = 4
    for j in range(2):
        m.tile_w[j], m.tile_h[j] = 128 if depth == 10 else 256, 16
    m.lds_bytes = 4096
    keep = np.zeros(1 << 16, np.uint8)
    m.tables, m.live = keep.ctypes.data, K.MAP_LIVE
    m._keep = keep
    return m


def test_map_create_argument_errors_before_any_device_call():
    """A valid configuration ends at the device — 0 where there is one, E_DEVICE where there is none —, and that comes last: every
    argument error below is returned with an otherwise valid configuration, and the earlier ones also with a later error present."""
    import fldr_scale as K
    import fldr_rate as R
    import fldr_video as V

    def create(mutate=lambda c: None, in_size=(H0, W0), out_size=(H1, W1), filter=K.BICUBIC, where=K.AUTO, device=0, read=K.READ_AUTO):
        cfg = K.map_config(in_size, out_size, V.Format("nv12"), filter, where, device, read)
        mutate(cfg)
        m = K.MapStruct()
        m.live = 7                                                             # ... and an error leaves the struct zeroed
        rc = K.map_create_raw(cfg, m)
        if rc == 0:
            K.lib().fldr_scale_map_destroy(ctypes.byref(m))
        assert m.live == 0 and not m.tables
        return rc
    bad_format = lambda c: setattr(c.format, "layout", 2)
    too_many = dict(in_size=(H0, 1100), out_size=(H1, 100), filter=K.LANCZOS3)
    assert create() in (0, R.E_DEVICE)
    assert create(bad_format) == V.E_FORMAT and create(**too_many) == K.E_ARG
    assert K.map_create_raw(None, K.MapStruct()) == K.E_ARG and K.map_create_raw(K.map_config((8, 8), (8, 8), V.Format()), None) == K.E_ARG
    for size in (0, 16385, -1):
        for which in range(4):
            sizes = [H0, W0, H1, W1]
            sizes[which] = size
            assert create(bad_format, in_size=sizes[:2], out_size=sizes[2:]) == K.E_ARG, (size, which)
    for f in (-1, 3):
        assert create(bad_format, filter=f) == K.E_ARG
    for w in (-1, 3):
        assert create(bad_format, where=w) == K.E_ARG
    assert create(bad_format, device=-1) == K.E_ARG
    for r in (-1, 3):
        assert create(bad_format, read=r) == K.E_ARG
    for i in range(3):
        assert create(lambda c: (bad_format(c), c.reserved.__setitem__(i, 1))) == K.E_ARG
    for field, val in (("layout", 2), ("matrix", 2), ("range", -1), ("depth", 9), ("depth", 12)):
        assert create(lambda c: setattr(c.format, field, val)) == V.E_FORMAT, field
    assert create(lambda c: setattr(c.format, "depth", 9), **too_many) == V.E_FORMAT     # the format before the tap limit
    assert create(in_size=(1100, W0), out_size=(100, W1), filter=K.LANCZOS3) == K.E_ARG   # the limit of the vertical axis
    # a staged read whose rows do not fit is an argument error, after the format; the other two reads go on to the device
    wide = dict(in_size=(H0, 8192), out_size=(H1, 256), filter=K.BILINEAR)
    assert create(read=K.READ_STAGED, **wide) == K.E_ARG and create(lambda c: setattr(c.format, "depth", 9), read=K.READ_STAGED, **wide) == V.E_FORMAT
    assert create(read=K.READ_DIRECT, **wide) in (0, R.E_DEVICE) and create(**wide) in (0, R.E_DEVICE) and create(read=K.READ_STAGED) in (0, R.E_DEVICE)
    assert create(device=1 << 20) == R.E_DEVICE
    K.lib().fldr_scale_map_destroy(None)
    K.lib().fldr_scale_map_destroy(ctypes.byref(K.MapStruct()))


@pytest.mark.parametrize("layout", ["nv12", "i420"])
@pytest.mark.parametrize("depth", [8, 10])
def test_frame_argument_errors_before_any_device_call(layout, depth):
    import fldr_scale as K
    import fldr_video as V
    b = 2 if depth == 10 else 1
    m = _fake_map(K, V, layout, depth)
    bufs = []

    def call(mutate=lambda src, dst: None, use=(True, True), the_map=m):
        ib, ibase, (src,) = _host(V, layout, depth, H0, W0, 1)
        ob, obase, (dst,) = _host(V, layout, depth, H1, W1, 1)
        bufs.extend((ib, ob))
        mutate(src, dst)
        return K.frame_raw(the_map, src if use[0] else None, dst if use[1] else None, None)
    no_plane = lambda src, dst: dst.plane.__setitem__(1, None)
    # the map first: null, zeroed, destroyed
    assert call(the_map=None) == K.E_STATE and call(no_plane, use=(False, True), the_map=None) == K.E_STATE
    dead = _fake_map(K, V, layout, depth)
    dead.live = 0
    assert call(the_map=dead) == K.E_STATE
    dead = _fake_map(K, V, layout, depth)
    dead.tables = None
    assert call(the_map=dead) == K.E_STATE
    # then the frames null, seen before a missing plane
    assert call(no_plane, use=(False, True)) == K.E_ARG and call(lambda s, d: s.plane.__setitem__(0, None), use=(True, False)) == K.E_ARG
    # then planes, then pitches, of in, then of out
    shapes_in, shapes_out = V.plane_shapes(layout, H0, W0), V.plane_shapes(layout, H1, W1)
    for q in range(len(shapes_in)):
        assert call(lambda s, d: s.plane.__setitem__(q, None)) == V.E_PLANE
        assert call(lambda s, d: d.plane.__setitem__(q, None)) == V.E_PLANE
        assert call(lambda s, d: s.pitch.__setitem__(q, shapes_in[q][1] * b - b)) == V.E_PITCH
        assert call(lambda s, d: d.pitch.__setitem__(q, shapes_out[q][1] * b - b)) == V.E_PITCH
        assert call(lambda s, d: d.pitch.__setitem__(q, shapes_in[q][1] * b)) == V.E_PITCH        # a pitch that fits the IN width is short for out
        if depth == 10:
            assert call(lambda s, d: s.plane.__setitem__(q, s.plane[q] + 1)) == V.E_PLANE
            assert call(lambda s, d: d.pitch.__setitem__(q, shapes_out[q][1] * b + 1)) == V.E_PITCH
    assert call(lambda s, d: (s.pitch.__setitem__(0, 2), s.plane.__setitem__(1, None))) == V.E_PLANE          # in: planes before pitches
    assert call(lambda s, d: (s.pitch.__setitem__(0, 2), d.plane.__setitem__(1, None))) == V.E_PITCH          # in before out
    # last: out overlapping in — the whole frame, the last byte of a plane of the SOURCE size
    assert call(lambda s, d: d.plane.__setitem__(0, s.plane[0])) == K.E_ARG
    assert call(lambda s, d: d.plane.__setitem__(1, s.plane[0] + H0 * W0 * b - b)) == K.E_ARG
    assert call(lambda s, d: s.plane.__setitem__(1, d.plane[0] + ((H1 - 1) * W1 + W1 - 1) * b)) == K.E_ARG
    assert not any(x.any() for x in bufs)


def _io(K, V, layout, depth, m, n_t=2):
    ib, ibase, ins = _host(V, layout, depth, m.cfg.in_H, m.cfg.in_W, 2)
    ob, obase, outs_ = _host(V, layout, depth, m.cfg.out_H, m.cfg.out_W, n_t)
    io = K.ScaleIO()
    io.v.H, io.v.W = m.cfg.in_H, m.cfg.in_W
    io.v.in_format = V.Format(layout, depth=depth)
    io.v.out_format = V.Format(layout, depth=depth)
    io.v.in_[0], io.v.in_[1] = ins
    outs = (V.Frame * n_t)(*outs_)
    io.v.n_t, io.v.t, io.v.out = n_t, ibase, ctypes.cast(outs, ctypes.POINTER(V.Frame))
    io.scene = 1
    io._keep = (ib, ob, outs)
    return io, (ib, ob), outs


@pytest.mark.parametrize("layout,depth", [("nv12", 8), ("i420", 10)])
@pytest.mark.parametrize("where", [O.BEFORE, O.AFTER])
def test_forward_argument_errors_before_any_device_call(layout, depth, where):
    """Without a model every otherwise valid call ends at the null model (E_ARG), which comes after the formats and frames: a bad frame
    that is reported shows that everything before it passed."""
    import fldr_scale as K
    import fldr_rate as R
    import fldr_video as V
    l = K.lib()
    m = _fake_map(K, V, layout, depth, where)
    ws = np.zeros(4096 + 256, np.uint8)
    wsp = (ws.ctypes.data + 255) // 256 * 256

    def call(mutate=lambda io, outs: None, the_map=m):
        io, bufs, outs = _io(K, V, layout, depth, m)
        mutate(io, outs)
        rc = l.fldr_scale_forward(None, ctypes.byref(the_map) if the_map is not None else None, ctypes.byref(io), ctypes.c_void_p(wsp), 1 << 40, None)
        assert not any(b.any() for b in bufs) and not ws.any()
        return rc
    bad_frame = lambda io, outs: outs[1].pitch.__setitem__(0, 2)              # the last thing checked before the model
    assert l.fldr_scale_forward(None, ctypes.byref(m), None, None, 0, None) == K.E_ARG
    assert call() == K.E_ARG and call(bad_frame) == V.E_PITCH
    assert call(bad_frame, the_map=None) == K.E_STATE and call(bad_frame, the_map=K.MapStruct()) == K.E_STATE
    both = lambda f: (lambda io, outs: (bad_frame(io, outs), f(io)))
    for field, val in (("H", H1), ("W", W1), ("H", 0), ("n_t", 0), ("n_t", -1), ("n_t", 65), ("t", None)):
        assert call(both(lambda io: setattr(io.v, field, val))) == K.E_ARG, (field, val)
    assert call(both(lambda io: setattr(io.v, "out", ctypes.POINTER(V.Frame)()))) == K.E_ARG
    for s in (-1, 2):
        assert call(both(lambda io: setattr(io, "scene", s))) == K.E_ARG
    for i in range(4):
        assert call(both(lambda io: io.reserved.__setitem__(i, 1))) == K.E_ARG
    assert call(both(lambda io: setattr(io.scene_params, "sad_permille", 1001))) == K.E_ARG
    assert call(both(lambda io: io.scene_params.reserved.__setitem__(1, 1))) == K.E_ARG
    # the formats: each checked, then compared with each other and the map's
    assert call(both(lambda io: setattr(io.v.in_format, "layout", 2))) == V.E_FORMAT
    assert call(both(lambda io: setattr(io.v.out_format, "depth", 9))) == V.E_FORMAT
    assert call(both(lambda io: setattr(io.v.out_format, "depth", 18 - depth))) == R.E_FORMAT
    assert call(both(lambda io: (setattr(io.v.in_format, "layout", 1 - io.v.in_format.layout), setattr(io.v.out_format, "layout", io.v.in_format.layout)))) == R.E_FORMAT
    # planes, then pitches, of in[0], in[1], then of every out[k]
    assert call(lambda io, o: io.v.in_[1].plane.__setitem__(1, None)) == V.E_PLANE
    assert call(lambda io, o: io.v.in_[0].pitch.__setitem__(0, 2)) == V.E_PITCH
    assert call(lambda io, o: o[1].plane.__setitem__(0, None)) == V.E_PLANE
    assert call(lambda io, o: (io.v.in_[0].pitch.__setitem__(0, 2), o[1].plane.__setitem__(1, None))) == V.E_PITCH      # the inputs before the outputs
    fmt = V.Format(layout, depth=depth)
    fr = V.Frame()
    assert l.fldr_scale_workspace_bytes(None, None, 1) == K.E_STATE and l.fldr_scale_workspace_bytes(None, ctypes.byref(K.MapStruct()), 1) == K.E_STATE
    assert l.fldr_scale_workspace_bytes(None, ctypes.byref(m), 0) == K.E_ARG and l.fldr_scale_workspace_bytes(None, ctypes.byref(m), 65) == K.E_ARG
    assert l.fldr_scale_workspace_bytes(None, ctypes.byref(m), 1) < 0
    assert l.fldr_scale_temp_frame(None, ctypes.byref(m), None, 1, 0, None, ctypes.byref(fr)) == K.E_ARG
    assert l.fldr_scale_temp_frame(None, ctypes.byref(m), ctypes.byref(fmt), 1, 0, None, None) == K.E_ARG
    assert l.fldr_scale_temp_frame(None, None, ctypes.byref(fmt), 1, 0, None, ctypes.byref(fr)) == K.E_STATE


def _create(l, h, model=None, **kw):
    import fldr_scale as K
    import fldr_video as V
    cfg = K.make_config((64, 64), (96, 128), V.Format("i420"), 24, 60)
    for k, v in kw.items():
        if k == "mutate":
            v(cfg)
        elif k in ("out_H", "out_W", "filter", "where"):
            setattr(cfg, k, v)
        else:
            setattr(cfg.rate, k, v)
    before = bytes(cfg)
    rc = l.fldr_scale_create(model, ctypes.byref(cfg), ctypes.byref(h))
    assert bytes(cfg) == before and not h.value                              # an error writes nothing
    return rc


def test_stream_argument_errors_before_any_device_call():
    import fldr_scale as K
    import fldr_rate as R
    import fldr_video as V
    l = K.lib()
    h = ctypes.c_void_p()
    create = lambda **kw: _create(l, h, **kw)
    ratio_bad = dict(in_num=1, in_den=1, out_num=65, out_den=1)              # 65 outputs per pushed frame
    taps_bad = dict(W=1100, out_W=100, filter=K.LANCZOS3)                    # the last of this library's own checks
    assert create() == K.E_ARG                                               # valid (24 -> 60: B = 5), no model
    assert create(**taps_bad) == K.E_ARG and create(in_num=25, out_num=25, **taps_bad) == K.E_ARG
    assert create(**ratio_bad) == R.E_RATIO
    assert create(in_num=1, in_den=1, out_num=64, out_den=1) == K.E_ARG
    # fldr_rate_create's checks with its codes, in its order — the ratio of the rates included — before any word of this library
    assert create(H=1) == R.E_ARG and create(device=-1) == R.E_ARG and create(scene=2) == R.E_ARG
    assert create(mutate=lambda c: c.rate.reserved.__setitem__(2, 1)) == R.E_ARG
    assert create(mutate=lambda c: setattr(c.rate.scene_params, "sad_permille", 1001)) == R.E_ARG
    assert create(mutate=lambda c: setattr(c.rate.format, "layout", 3)) == V.E_FORMAT
    for term in ("in_num", "in_den", "out_num", "out_den"):
        assert create(**{term: 0}) == R.E_RATIO and create(**{term: -24}) == R.E_RATIO, term
    assert create(mutate=lambda c: setattr(c.rate.format, "layout", 3), filter=3) == V.E_FORMAT
    assert create(in_num=0, filter=3) == R.E_RATIO and create(in_num=0, out_H=0) == R.E_RATIO
    assert create(in_num=2 ** 25 + 1, in_den=1, out_num=2 ** 24, out_den=1, filter=3) == R.E_RATIO
    for field, bad in (("out_H", 0), ("filter", 3), ("where", 3)):
        assert create(**dict(ratio_bad, **{field: bad})) == R.E_RATIO, (field, bad)
    # then this library's: the sizes, filter, where, the reserved words, the tap limit — seen here with B == 1, where a valid
    # configuration goes on to the device and so cannot be what returns E_ARG
    same = dict(in_num=25, out_num=25)
    for field, bad in (("H", 16385), ("W", 16385), ("out_H", 0), ("out_H", 16385), ("out_W", 0), ("out_W", -5), ("filter", 3), ("filter", -1),
                       ("where", 3), ("where", -1)):
        assert create(**dict(same, **{field: bad})) == K.E_ARG, (field, bad)
    for i in range(4):
        assert create(mutate=lambda c: c.reserved.__setitem__(i, 1), **same) == K.E_ARG
    assert create(H=1100, out_H=100, filter=K.LANCZOS3, **same) == K.E_ARG
    # a NULL model is an argument error exactly where a frame is interpolated (B != 1)
    assert create(in_num=25, out_num=50) == K.E_ARG and create(in_num=60, out_num=25) == K.E_ARG
    assert l.fldr_scale_create(None, None, ctypes.byref(h)) == K.E_ARG
    n = ctypes.c_int()
    assert l.fldr_scale_push(None, None, None, ctypes.byref(n), None) == K.E_ARG
    assert l.fldr_scale_flush(None, None, ctypes.byref(n)) == K.E_ARG
    assert l.fldr_scale_reset(None) == K.E_ARG
    assert l.fldr_scale_max_out(None) == K.E_ARG
    l.fldr_scale_destroy(None)


# ---- the oracle alone ----------------------------------------------------------------------------------------------------------------------
def _tables(in_size, out_size, filt):
    import fldr_scale as K
    return K.tables(in_size, out_size, filt)


@pytest.mark.parametrize("layout,depth", [("nv12", 8), ("i420", 8), ("nv12", 10), ("i420", 10)])
def test_oracle_flat_planes_stay_flat_and_identity_is_the_identity(layout, depth):
    import fldr_video as V
    mx = 1023 if depth == 10 else 255
    dt = np.uint16 if depth == 10 else np.uint8
    sh = 6 if (layout, depth) == ("nv12", 10) else 0
    for (iH, iW), (oH, oW) in (((9, 7), (5, 16)), ((6, 10), (13, 4))):
        for filt in FILTERS:
            t = _tables((iH, iW), (oH, oW), filt)
            for v in (0, 1, mx // 2, mx - 1, mx):
                flat = tuple(np.full(s, v << sh, dt) for s in V.plane_shapes(layout, iH, iW))
                out = O.scale(flat, layout, depth, (oH, oW), t)
                assert [o.shape for o in out] == V.plane_shapes(layout, oH, oW)
                assert all((o == (v << sh)).all() for o in out), (filt, v)
    g = np.random.default_rng(5)
    f = tuple(g.integers(0, 65536 if depth == 10 else 256, s).astype(dt) for s in V.plane_shapes(layout, 9, 11))
    for filt in FILTERS:
        out = O.scale(f, layout, depth, (9, 11), _tables((9, 11), (9, 11), filt))
        want = O.canonicalised(f, layout, depth)
        assert all(np.array_equal(a, b) for a, b in zip(out, want))
        if depth == 10:
            assert not any(np.array_equal(a, b) for a, b in zip(out, f))          # the dirty bits were dropped ...
            assert all(np.array_equal(O.value(a, layout, depth), O.value(b, layout, depth)) for a, b in zip(out, f))      # ... and nothing else


def test_oracle_hand_worked_rows():
    """Bicubic 4 -> 8 on [0, 255, 0, 255]: Catmull-Rom at 1/4 and 3/4 is (-9, 111, 29, -3) / 128, i.e. q = -1152, 14208, 3712, -384.
    Output 1 (c = 1/4, sources -1 .. 2 = 0, 0, 255, 0): 3712 x 255 = 946560, m = (946560 + 128) >> 8 = 3698, o = (3698 x 16384 + 2^19) >> 20
    = 58.  Output 0 (c = -1/4, sources 0, 0, 0, 255): -1152 x 255 = -293760, m = -1147, o = floor(-17.4) = -18, clamped to 0.
    Bilinear 4 -> 2 on [10, 20, 30, 50]: q = (1, 3, 3, 1) / 8; output 0 from 10, 10, 20, 30 is 16.25 -> 16, output 1 from 20, 30, 50, 50 is
    38.75 -> 39."""
    zero_c = np.zeros((1, 4), np.uint8)
    t = _tables((1, 4), (1, 8), O.BICUBIC)
    assert t["luma_x"][1][:2].tolist() == [[-384, 3712, 14208, -1152], [-1152, 14208, 3712, -384]] and t["luma_y"][1].tolist() == [[0, 16384, 0, 0]]
    row = O.scale((np.array([[0, 255, 0, 255]], np.uint8), zero_c), "nv12", 8, (1, 8), t)[0][0].tolist()
    assert row == [0, 58, 221, 215, 40, 34, 197, 255]
    assert (-1152 * 255 + 128) >> 8 == -1147 and (-1147 * 16384 + (1 << 19)) >> 20 == -18 and (3698 * 16384 + (1 << 19)) >> 20 == 58
    lo, hi = O.unclamped_range(np.array([[0, 255, 0, 255]], np.int64), t["luma_x"], t["luma_y"], 8)
    assert lo == -18 and hi > 255                                             # both clamps act on this row
    t = _tables((1, 4), (1, 2), O.BILINEAR)
    assert t["luma_x"][1].tolist() == [[2048, 6144, 6144, 2048]] * 2 and t["luma_x"][0].tolist() == [-1, 1]
    assert O.scale((np.array([[10, 20, 30, 50]], np.uint8), zero_c), "nv12", 8, (1, 2), t)[0][0].tolist() == [16, 39]
    # the same row as 10-bit words: P010 carries it in the high bits and ignores dirty low ones, yuv420p10le ignores dirty high ones
    p010 = np.array([[(40 << 6) | 63, (80 << 6) | 1, 120 << 6, (200 << 6) | 32]], np.uint16)
    low10 = np.array([[40 | 0xfc00, 80 | 0x8000, 120, 200 | 0x0400]], np.uint16)
    zc = np.zeros((1, 4), np.uint16)
    assert O.scale((p010, zc), "nv12", 10, (1, 2), t)[0][0].tolist() == [65 << 6, 155 << 6]        # 65 and 155 exactly
    assert O.scale((low10, zc, zc[:, :2]), "i420", 10, (1, 2), t)[0][0].tolist() == [65, 155]
