"""CPU checks of the conform API (include/fldr_conform.h, libfldr_conform.so): the library's symbol table and link, the header as plain C99 /
C++, the C example, the code-generation guards, the binding's struct mirrors, the coefficient table against tests/conform_oracle.py and
against the route through R'G'B', the int32 bound, the oracle against a float64 statement of the conversion and on hand-worked cases, the
argument checks of the kernel entry, the view and the stream — which happen before any device call, so they run without a GPU —, and the
table builder as a stand-alone program under the host sanitizers."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import conform_oracle as O
from lib_checks import declared as _declared, syms as _syms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fldr-vfi_amd")
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "fldr_conform.h")
LIB = os.path.join(PKG, "libfldr_conform.so")
EXAMPLE = os.path.join(ROOT, "examples", "fldr_conform.c")
NAMES = ("version", "error_string", "sizeof", "coefs", "view", "frame", "create", "max_out", "push", "flush", "reset", "destroy")
ALLOWED_LIBS = ("fldr_conform", "fldr_rate", "fldr_video", "fldr_model")


def _fmt(f):
    """A fldr_video.Format of an oracle format (layout, matrix, range, depth)."""
    import fldr_video as V
    return V.Format(*f)


# ---- the library ------------------------------------------------------------------------------------------------------------------------
def test_library_exports_exactly_the_header():
    declared = _declared(HDR, "FLDR_CONFORM_API")
    assert len(NAMES) == 12 and declared == set("fldr_conform_" + n for n in NAMES), sorted(declared)
    assert _syms(LIB, ["--defined-only"]) == declared
    import fldr_conform
    assert set(fldr_conform.EXPORTS) == declared


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
    assert not used & {"fldr_rate_create", "fldr_rate_push", "fldr_rate_flush"}          # the stream is this library's own: it holds two formats


def test_header_and_library_name_no_library_but_rate_video_and_model():
    text = open(HDR).read().lower()
    raw = open(LIB, "rb").read().lower()
    for name in os.listdir(INC):
        other = re.fullmatch(r"(fldr_[a-z0-9]+)(_test_hooks)?\.h", name).group(1)
        if other not in ALLOWED_LIBS and other != "fldr_hip":
            assert other not in text and other.encode() not in raw, other
        if name != "fldr_conform.h":
            assert "fldr_conform" not in open(os.path.join(INC, name)).read().lower(), name
    for name in os.listdir(PKG):
        if re.fullmatch(r"libfldr_\w+\.so", name) and name != "libfldr_conform.so":
            assert b"fldr_conform" not in open(os.path.join(PKG, name), "rb").read(), name


@pytest.mark.parametrize("compiler", [["gcc", "-std=c99", "-x", "c"], ["g++", "-std=c++11", "-x", "c++"]])
def test_header_is_plain_c99_and_cxx(compiler, tmp_path):
    assert shutil.which(compiler[0]), compiler[0] + " not installed"
    src = tmp_path / "h.c"
    src.write_text('#include <stddef.h>\n#include "fldr_conform.h"\nint main(void) { fldr_conform_config c; fldr_conform_stream_config s;\n'
                   '  c.dither = FLDR_CONFORM_DITHER_ORDERED; s.dst_x = 2;\n'
                   '  return fldr_conform_sizeof(0) == (int)sizeof(c) && c.dither == 1 && s.dst_x == 2 && FLDR_CONFORM_DITHER_NONE == 0 &&\n'
                   '         FLDR_CONFORM_MAX_SIZE == 16384 && FLDR_CONFORM_KYY == 0 && FLDR_CONFORM_KVV == 6 &&\n'
                   '         offsetof(fldr_conform_stream_config, out_H) == sizeof(fldr_rate_config) ? 0 : 1; }\n')
    r = subprocess.run(compiler + ["-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I" + INC, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "hip" not in re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S).lower()


def test_header_defines_no_error_code_and_says_whose_it_returns():
    text = open(HDR).read()
    assert not re.findall(r"#define\s+FLDR_[A-Z0-9]+_E_[A-Z]+", text)
    for s in ("defines no code of its own", "FLDR_RATE_E_ARG", "FLDR_RATE_E_RATIO", "FLDR_RATE_E_DEVICE", "FLDR_VIDEO_E_FORMAT",
              "fldr_conform_error_string is fldr_rate_error_string"):
        assert s in text, s
    import fldr_conform as K
    import fldr_rate as R
    l = K.lib()
    for code in (R.E_ARG, R.E_STATE, R.E_RATIO, R.E_DEVICE, -101, -3, 0, -999):
        assert l.fldr_conform_error_string(code) == R.lib().fldr_rate_error_string(code)
    assert (K.E_ARG, K.E_STATE, K.E_RATIO, K.E_DEVICE) == (R.E_ARG, R.E_STATE, R.E_RATIO, R.E_DEVICE)


def test_header_states_the_rule_the_limits_and_what_is_out_of_scope():
    text = open(HDR).read()
    for s in ("myu = 2(1-KbA)(KbB - KgB KbA/KgA)", "mvu = -myu / (2(1-KrB))", "r(v) = floor(v * 16384 + 0.5)", "16384, -1893, -3407, 16689, 1878, 1230, 16799",
              "U' = cc_d + ((KUU (U - cc_s) + KUV (V - cc_s) + RC) >> 14)", "Y' = yo_d + ((8 KYY (Y - yo_s) + KYU cu + KYV cv + RY) >> 17)",
              "RY = (2 b + 1) << 10 and RC = (2 b + 1) << 7", "by definition and not by evaluation", "1.82e8", "[dst/2, dst/2 + ceil(in/2))",
              "FLDR_CONFORM_MAX_SIZE = 16384", "BT.2020 is not in fldr_video_format", "no transfer-function or primaries conversion",
              "the fill is black only", "the clamp is to [0, mx], not to the nominal range", 'chroma siting is "left" only',
              "4:2:2, 4:4:4, packed and RGB formats are out of scope", "the stream is synchronous", "Checked in this order", "Validation order"):
        assert s in text, s


def test_example_builds_with_cc(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    exe = tmp_path / "fldr_conform"
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + INC, "-o", str(exe), EXAMPLE, "-L" + PKG,
                        "-l:libfldr_conform.so", "-l:libfldr_rate.so", "-l:libfldr_video.so", "-l:libfldr_model.so", "-Wl,-rpath," + PKG],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    src = open(EXAMPLE).read()
    assert "hip" not in re.sub(r"/\*.*?\*/", "", src, flags=re.S).lower()
    u = subprocess.run([str(exe)], capture_output=True, text=True)            # no arguments: usage, no device touched
    assert u.returncode == 2 and "usage" in u.stderr
    for word in ("out=WxH", "at=X,Y", "to=bt601|bt709", "tofull|tolimited", "to8|to10", "dither"):
        assert word in u.stderr, word
    for bad in (["w.npz", "64", "1", "25", "25"],
                ["w.npz", "64", "64", "25/0", "25"],
                ["w.npz", "64", "64", "25", "x"],
                ["w.npz", "64", "64", "25", "25", "out=128"],
                ["w.npz", "64", "64", "25", "25", "out=128x"],
                ["w.npz", "64", "64", "25", "25", "out=0x128"],
                ["w.npz", "64", "64", "25", "25", "out=128x16385"],
                ["w.npz", "64", "64", "25", "25", "out=32x64"],                  # the picture does not fit
                ["w.npz", "64", "64", "25", "25", "out=128x64", "at=66,0"],      # ... nor at that place
                ["w.npz", "64", "64", "25", "25", "out=128x64", "at=3,0"],       # an odd place
                ["w.npz", "64", "64", "25", "25", "out=128x64", "at=-2,0"],
                ["w.npz", "64", "64", "25", "25", "out=128x64", "at=2"],
                ["w.npz", "64", "64", "25", "25", "at=0,2"],                     # no canvas to move on
                ["w.npz", "64", "64", "25", "25", "to=bt2020"],
                ["w.npz", "64", "64", "25", "25", "to12"],
                ["-", "64", "64", "24", "60", "to=bt709"]):                      # frames to interpolate and no weights
        u = subprocess.run([str(exe)] + bad, capture_output=True, text=True)
        assert u.returncode == 2 and "usage" in u.stderr, bad


def test_no_unsafe_packed_fp32_in_the_conform_library():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_pk_opsel.py"), LIB], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    ks = KR.kernels(LIB)
    assert len(ks) == 32, [k["name"] for k in ks]         # container in x container out x matrices equal / different; every plane in each
    for k in ks:
        assert "conform_kernel" in k["name"], k["name"]
        assert k.get("scratch", -1) == 0 and k.get("vgpr_spills", -1) == 0 and k.get("sgpr_spills", -1) == 0 and k.get("lds", -1) == 0, k


def test_binding_struct_sizes_and_version():
    import fldr_conform as K
    l = K.lib()
    text = open(HDR).read()
    assert l.fldr_conform_version() == K.CONFORM_VERSION == int(re.search(r"#define FLDR_CONFORM_VERSION (\d+)", text).group(1)) == 100
    for which, cls in enumerate((K.Config, K.StreamConfig)):
        assert l.fldr_conform_sizeof(which) == ctypes.sizeof(cls)
    assert ctypes.sizeof(K.StreamConfig) == ctypes.sizeof(K.RateConfig) + 8 + ctypes.sizeof(K.Format) + 28 and K.StreamConfig.out_H.offset == ctypes.sizeof(K.RateConfig)
    assert l.fldr_conform_sizeof(2) == K.E_ARG and l.fldr_conform_sizeof(-1) == K.E_ARG
    for macro, v in (("FLDR_CONFORM_DITHER_NONE", K.DITHER_NONE), ("FLDR_CONFORM_DITHER_ORDERED", K.DITHER_ORDERED), ("FLDR_CONFORM_MAX_SIZE", K.MAX_SIZE),
                     ("FLDR_CONFORM_KYY", K.KYY), ("FLDR_CONFORM_KYU", K.KYU), ("FLDR_CONFORM_KYV", K.KYV), ("FLDR_CONFORM_KUU", K.KUU),
                     ("FLDR_CONFORM_KUV", K.KUV), ("FLDR_CONFORM_KVU", K.KVU), ("FLDR_CONFORM_KVV", K.KVV)):
        assert int(re.search(r"#define %s\s+(\d+)" % macro, text).group(1)) == v, macro
    assert (K.DITHER_NONE, K.DITHER_ORDERED) == (O.DITHER_NONE, O.DITHER_ORDERED)
    internal = open(os.path.join(PKG, "conform", "conform_internal.h")).read()
    assert int(re.search(r"CONFORM_THREADS = (\d+)", internal).group(1)) == K.THREADS and int(re.search(r"RUN_BYTES = (\d+)", internal).group(1)) == K.RUN_BYTES


# ---- the table ------------------------------------------------------------------------------------------------------------------------------
def test_coefs_equal_the_oracle_for_all_256_format_pairs():
    import fldr_conform as K
    pairs = list(itertools.product(O.FORMATS, O.FORMATS))
    assert len(pairs) == 256
    for s, d in pairs:
        want = O.coefs(s[1:], d[1:])
        assert K.coefs(_fmt(s), _fmt(d)) == [want[n] for n in O.NAMES], (s, d)
    k = O.coefs(("bt601", "limited", 8), ("bt709", "limited", 8))
    assert [k[n] for n in O.NAMES] == [16384, -1893, -3407, 16689, 1878, 1230, 16799]
    import fldr_video as V
    assert K.coefs(V.Format("nv12", "bt601", "limited", 0), V.Format("nv12", "bt709", "limited", 8)) == [k[n] for n in O.NAMES]      # depth 0 is 8


def _rgb_matrix(name):
    """R'G'B' -> (Y, Cb, Cr), all normalised (Y 0 .. 1, C -0.5 .. 0.5)."""
    kr, kb = O.MATRICES[name]
    kg = 1.0 - kr - kb
    return np.array([[kr, kg, kb], [-kr / (2 * (1 - kb)), -kg / (2 * (1 - kb)), 0.5], [0.5, -kg / (2 * (1 - kr)), -kb / (2 * (1 - kr))]], np.float64)


def test_coefs_are_within_half_a_unit_of_the_route_through_rgb():
    """The OTHER route: YCbCr(A) -> R'G'B' -> YCbCr(B) composed numerically as 3 x 3 matrices, then scaled by the spans.  Each integer
    coefficient, over 16384, lies within 2^-15 of it (plus the 1e-12 the composition itself may be off)."""
    for s, d in itertools.product(O.COLOURS, O.COLOURS):
        T = _rgb_matrix(d[0]) @ np.linalg.inv(_rgb_matrix(s[0]))
        assert abs(T[0, 0] - 1) < 1e-12 and abs(T[1, 0]) < 1e-12 and abs(T[2, 0]) < 1e-12          # luma passes, and moves no chroma
        _, ys_s, _, cs_s, _ = O.side(s[1], s[2])
        _, ys_d, _, cs_d, _ = O.side(d[1], d[2])
        route = dict(KYY=T[0, 0] * ys_d / ys_s, KYU=T[0, 1] * ys_d / cs_s, KYV=T[0, 2] * ys_d / cs_s, KUU=T[1, 1] * cs_d / cs_s,
                     KUV=T[1, 2] * cs_d / cs_s, KVU=T[2, 1] * cs_d / cs_s, KVV=T[2, 2] * cs_d / cs_s)
        k, f = O.coefs(s, d), O.coefs_float(s, d)
        for n in O.NAMES:
            assert abs(k[n] / 16384.0 - route[n]) <= 2.0 ** -15 + 1e-12, (s, d, n, k[n], route[n])
            assert abs(f[n] - route[n]) < 1e-12, (s, d, n)


def test_equal_matrices_give_the_exact_unit_and_zero_entries():
    for s, d in itertools.product(O.COLOURS, O.COLOURS):
        if s[0] != d[0]:
            continue
        assert O.matrix_terms(s[0], d[0]) == (0.0, 0.0, 1.0, 0.0, 0.0, 1.0)
        k = O.coefs(s, d)
        assert k["KYU"] == k["KYV"] == k["KUV"] == k["KVU"] == 0 and k["KUU"] == k["KVV"], (s, d)
        if s[1:] == d[1:]:
            assert k["KYY"] == k["KUU"] == 16384


def test_every_intermediate_fits_int32_over_all_pairs():
    """The sums the kernel forms, rounding term and the folded destination offset included, from the operand maxima of each pair."""
    worst_y, worst_c = O.worst_sums()
    assert worst_y <= 1.82e8 and worst_c < 2 ** 31 and worst_y < 2 ** 31, (worst_y, worst_c)
    # ... and the oracle's own int64 sums on the extreme code values stay inside it
    for s, d in itertools.product(O.COLOURS, O.COLOURS):
        mx, yo_d = O.side(s[1], s[2])[4], O.side(d[1], d[2])[0]
        for y, u, v in itertools.product((0, mx), (0, mx), (0, mx)):
            sy, su, sv = O.sums(np.full((2, 2), y, np.int64), np.full((1, 1), u, np.int64), np.full((1, 1), v, np.int64), ("nv12",) + s, ("nv12",) + d)
            assert np.abs(sy).max() + (1 << 17) + (yo_d << 17) <= worst_y and max(np.abs(su).max(), np.abs(sv).max()) + (1 << 14) + (1 << 23) <= worst_c


# ---- the oracle against a float64 statement ----------------------------------------------------------------------------------------------------
def _safe_frame(src, H, W, kind, seed):
    """A frame whose colours stay away from the ends of the nominal range (luma 10 % .. 90 % of its span, chroma within 20 % of its span
    around the centre), so that no conversion between the formats clamps it: seeded noise, or hard edges between two such colours."""
    layout, _, rng, depth = src
    yo, ys, cc, cs, _ = O.side(rng, depth)
    g = np.random.default_rng(seed)
    ch, cw = (H + 1) // 2, (W + 1) // 2
    lo, hi, amp = yo + ys // 10, yo + ys * 9 // 10, cs // 5
    if kind == "noise":
        Y, U, V = g.integers(lo, hi + 1, (H, W)), g.integers(cc - amp, cc + amp + 1, (ch, cw)), g.integers(cc - amp, cc + amp + 1, (ch, cw))
    else:
        yy, xx = np.mgrid[0:H, 0:W]
        m = (xx >= W // 3) ^ (yy >= H // 2)                                   # a vertical and a horizontal edge, on odd and even sites
        Y = np.where(m, hi, lo)
        mc = m[::2, ::2]
        U, V = np.where(mc, cc + amp, cc - amp), np.where(mc, cc - amp, cc + amp)
    return O.join(Y.astype(np.int64), U.astype(np.int64), V.astype(np.int64), layout, depth)


@pytest.mark.parametrize("kind", ["noise", "edges"])
def test_oracle_against_the_float64_statement(kind):
    """|integer rule - float64 statement| <= 1/2 (the one rounding) + the coefficient quantisation: every coefficient is within 2^-15 of
    its real value, and multiplies an operand of at most ymax = max|Y - yo_s|, cmax = max|C - cc_s| (the upsampled chroma over 8 is a
    weighted mean of such operands) — 2^-15 (ymax + 2 cmax) for luma, 2^-15 2 cmax for chroma — plus 1e-9 for the float sums."""
    total = clamped_total = 0
    for n, (s, d) in enumerate(itertools.product(O.COLOURS, O.COLOURS)):
        src, dst = (O.LAYOUTS[n & 1],) + s, (O.LAYOUTS[(n >> 1) & 1],) + d
        frame = _safe_frame(src, 9, 14, kind, n)
        clamped = []
        got = O.split(O.conform(frame, src, dst, clamped=clamped), dst[0], dst[3])
        want = O.conform_float(frame, src, dst)
        yo_s, _, cc_s, _, mx_s = O.side(s[1], s[2])
        mx_d = O.side(d[1], d[2])[4]
        ymax, cmax = max(yo_s, mx_s - yo_s), max(cc_s, mx_s - cc_s)
        bounds = (0.5 + 2.0 ** -15 * (ymax + 2 * cmax) + 1e-9, 0.5 + 2.0 ** -15 * 2 * cmax + 1e-9, 0.5 + 2.0 ** -15 * 2 * cmax + 1e-9)
        for p in range(3):
            inside = (want[p] >= 0) & (want[p] <= mx_d) & (got[p] > 0) & (got[p] < mx_d)       # the clamped samples are excluded, and counted
            err = np.abs(got[p] - want[p])[inside]
            assert err.size and err.max() <= bounds[p], (src, dst, p, err.max(), bounds[p])
            total += got[p].size
            clamped_total += int((~inside).sum())
        assert clamped[0] == 0, (src, dst)
    assert clamped_total * 100 <= total, (clamped_total, total)                 # at most 1 % excluded


# ---- hand-worked cases ------------------------------------------------------------------------------------------------------------------------
def _flat(layout, depth, y, u, v, H=4, W=6):
    ch, cw = (H + 1) // 2, (W + 1) // 2
    return O.join(np.full((H, W), y, np.int64), np.full((ch, cw), u, np.int64), np.full((ch, cw), v, np.int64), layout, depth)


def test_hand_worked_grey_and_range_cases():
    for y8, y10 in ((16, 64), (128, 512), (235, 940)):
        out = O.split(O.conform(_flat("nv12", 8, y8, 128, 128), ("nv12", "bt601", "limited", 8), ("i420", "bt601", "limited", 10)), "i420", 10)
        assert (out[0] == y10).all() and (out[1] == 512).all() and (out[2] == 512).all()
    out = O.split(O.conform(_flat("i420", 8, 255, 128, 128), ("i420", "bt709", "full", 8), ("i420", "bt709", "limited", 8)), "i420", 8)
    assert (out[0] == 235).all() and (out[1] == 128).all()
    out = O.split(O.conform(_flat("i420", 8, 0, 255, 0), ("i420", "bt709", "full", 8), ("i420", "bt709", "limited", 8)), "i420", 8)
    assert (out[0] == 16).all() and (out[1] == 240).all() and (out[2] == 16).all()           # 128 + round(127 x 224 / 255) = 240, 128 - 112


def test_hand_worked_saturated_red_601_to_709():
    """BT.601 limited red is (81, 90, 240).  By the table 16384, -1893, -3407, 16689, 1878, 1230, 16799 with cu = 8 (90 - 128) = -304 and
    cv = 8 (240 - 128) = 896:
      Y' = 16 + ((8 x 16384 x 65 + 1893 x 304 - 3407 x 896 + 65536) >> 17) = 16 + (6108016 >> 17) = 16 + 46 = 62
      U' = 128 + ((16689 x -38 + 1878 x 112 + 8192) >> 14) = 128 + (-415654 >> 14) = 128 - 26 = 102
      V' = 128 + ((1230 x -38 + 16799 x 112 + 8192) >> 14) = 128 + (1842940 >> 14) = 128 + 112 = 240: BT.709's red, (63, 102, 240), to a code."""
    assert 8 * 16384 * 65 + 1893 * 304 - 3407 * 896 + 65536 == 6108016 and 6108016 >> 17 == 46
    assert 16689 * -38 + 1878 * 112 + 8192 == -415654 and -415654 >> 14 == -26
    assert 1230 * -38 + 16799 * 112 + 8192 == 1842940 and 1842940 >> 14 == 112
    out = O.split(O.conform(_flat("nv12", 8, 81, 90, 240), ("nv12", "bt601", "limited", 8), ("nv12", "bt709", "limited", 8)), "nv12", 8)
    assert (out[0] == 62).all() and (out[1] == 102).all() and (out[2] == 240).all()


@pytest.mark.parametrize("fmt", O.FORMATS, ids=lambda f: "-".join(str(v) for v in f))
def test_equal_formats_give_the_identity_for_every_code(fmt):
    layout, _, _, depth = fmt
    n = 1 << depth
    codes = np.arange(64 * 64, dtype=np.int64).reshape(64, 64) % n            # every code of every plane: 4096 luma, 1024 of each chroma
    ramp = np.arange(1024, dtype=np.int64).reshape(32, 32) % n
    frame = O.join(codes, ramp, (n - 1) - ramp, layout, depth)
    vals = O.split(frame, layout, depth)
    assert all(len(np.unique(p)) == n for p in vals)
    for dither in (O.DITHER_NONE, O.DITHER_ORDERED):
        out = O.conform(frame, fmt, fmt, dither=dither)
        assert all(np.array_equal(a, b) for a, b in zip(out, frame)), dither


def test_dither_mean_over_a_block_is_the_exact_value():
    """10 -> 8 bits of a constant field: the 64 rounding terms of an 8 x 8 block are (2 b + 1) / 128 for b = 0 .. 63, evenly spread over
    one code, so the mean of the block equals the exact (unrounded) value of the integer sum within 1/128 < 1/64 code."""
    src, dst = ("i420", "bt709", "limited", 10), ("i420", "bt709", "limited", 8)
    k = O.coefs(src[1:], dst[1:])
    for y, u, v in ((64, 512, 512), (301, 400, 700), (502, 513, 511), (939, 64, 960), (777, 601, 333)):
        out = O.split(O.conform(_flat("i420", 10, y, u, v, 16, 16), src, dst, dither=O.DITHER_ORDERED), "i420", 8)
        plain = O.split(O.conform(_flat("i420", 10, y, u, v, 16, 16), src, dst), "i420", 8)
        exact = (16 + 8 * k["KYY"] * (y - 64) / 2.0 ** 17, 128 + k["KUU"] * (u - 512) / 2.0 ** 14, 128 + k["KVV"] * (v - 512) / 2.0 ** 14)
        for p in range(3):
            blocks = out[p][:8, :8], out[p][8:16, 8:16] if p == 0 else out[p][:8, :8]
            for b in blocks:
                assert abs(b.mean() - exact[p]) <= 1.0 / 64, (y, u, v, p, b.mean(), exact[p])
            assert abs(plain[p][0, 0] - exact[p]) <= 0.5
        assert len(np.unique(out[0])) == 2 or float(exact[0]).is_integer()      # the dither does move single samples


def test_placement_in_the_oracle():
    src, dst = ("nv12", "bt601", "limited", 8), ("i420", "bt709", "full", 10)
    g = np.random.default_rng(1)
    frame = (g.integers(0, 256, (5, 7)).astype(np.uint8), g.integers(0, 256, (3, 8)).astype(np.uint8))
    alone = O.conform(frame, src, dst)
    out = O.conform(frame, src, dst, (12, 16), (4, 6))
    assert [p.shape for p in out] == [(12, 16), (6, 8), (6, 8)]
    assert np.array_equal(out[0][6:11, 4:11], alone[0]) and np.array_equal(out[1][3:6, 2:6], alone[1]) and np.array_equal(out[2][3:6, 2:6], alone[2])
    border = np.ones((12, 16), bool)
    border[6:11, 4:11] = False
    assert (out[0][border] == 0).all()                                         # full range: luma black is 0
    cb = np.ones((6, 8), bool)
    cb[3:6, 2:6] = False
    assert (out[1][cb] == 512).all() and (out[2][cb] == 512).all()
    lim = O.conform(frame, src, ("nv12", "bt709", "limited", 10), (12, 16), (4, 6))
    assert (lim[0][border] == 64 << 6).all() and (lim[1][np.repeat(cb, 2, axis=1)] == 512 << 6).all()


# ---- argument errors without a device -----------------------------------------------------------------------------------------------------
H0, W0, H1, W1 = 10, 14, 16, 24


def _host(V, fmt, H, W):
    """One frame whose planes all point into one zeroed, 256-byte aligned host buffer."""
    b = 2 if fmt.bits == 10 else 1
    buf = np.zeros((H + 1) * (W + 1) * 2 * b + 512, np.uint8)
    off = (buf.ctypes.data + 255) // 256 * 256
    f = V.Frame()
    for p, (r, c) in enumerate(V.plane_shapes(fmt, H, W)):
        f.plane[p], f.pitch[p] = off, c * b
        off += r * c * b
    return buf, f


@pytest.mark.parametrize("src,dst", [(("nv12", "bt601", "limited", 8), ("i420", "bt709", "limited", 10)),
                                     (("i420", "bt709", "full", 10), ("nv12", "bt709", "limited", 8))])
def test_frame_argument_errors_before_any_device_call(src, dst):
    """Every call below carries an error, so none reaches the launch; the earlier checks are also made with a later error present."""
    import fldr_conform as K
    import fldr_video as V
    fi, fo = _fmt(src), _fmt(dst)
    bi, bo = (2 if fi.bits == 10 else 1), (2 if fo.bits == 10 else 1)
    bufs = []

    def call(mutate=lambda c, s, d: None, use=(True, True, True), **kw):
        args = dict(in_size=(H0, W0), out_size=(H1, W1), at=(4, 2), dither=False)
        args.update(kw)
        cfg = K.config(args["in_size"], fi, args["out_size"], fo, args["at"], args["dither"])
        ib, s = _host(V, fi, max(1, min(args["in_size"][0], 64)), max(1, min(args["in_size"][1], 64)))
        ob, d = _host(V, fo, max(1, min(args["out_size"][0], 64)), max(1, min(args["out_size"][1], 64)))
        bufs.extend((ib, ob))
        mutate(cfg, s, d)
        return K.frame_raw(cfg if use[0] else None, s if use[1] else None, d if use[2] else None, None)
    no_plane = lambda c, s, d: d.plane.__setitem__(1, None)                   # a later error, present in the calls that test an earlier one
    overlap = lambda c, s, d: d.plane.__setitem__(0, s.plane[0])              # the last check of all
    assert call(overlap) == K.E_ARG
    for use in ((False, True, True), (True, False, True), (True, True, False)):
        assert call(no_plane, use=use) == K.E_ARG
    for size in (0, -1, 16385):
        for which in range(4):
            sizes = [H0, W0, H1, W1]
            sizes[which] = size
            assert call(no_plane, in_size=sizes[:2], out_size=sizes[2:], at=(0, 0)) == K.E_ARG, (size, which)
    for at in ((1, 0), (0, 1), (3, 3), (-2, 0), (0, -2), (-1, -1)):             # odd or negative
        assert call(no_plane, at=at) == K.E_ARG, at
    for at in ((W1 - W0 + 2, 0), (0, H1 - H0 + 2), (12, 2), (4, 8)):            # W0 + 12 > W1; H0 + 8 > H1
        assert call(no_plane, at=at) == K.E_ARG, at
    assert call(no_plane, in_size=(H1 + 2, W0), at=(0, 0)) == K.E_ARG and call(no_plane, in_size=(H0, W1 + 1), at=(0, 0)) == K.E_ARG
    for dz in (-1, 2):
        assert call(no_plane, dither=dz) == K.E_ARG
    for i in range(3):
        assert call(lambda c, s, d: (no_plane(c, s, d), c.reserved.__setitem__(i, 1))) == K.E_ARG
    # the formats, after the words and before the frames
    for side_ in ("in_format", "out_format"):
        for field, val in (("layout", 2), ("matrix", 2), ("range", -1), ("depth", 9), ("depth", 12)):
            assert call(lambda c, s, d: (no_plane(c, s, d), setattr(getattr(c, side_), field, val))) == V.E_FORMAT, (side_, field)
    assert call(lambda c, s, d: (setattr(c.in_format, "layout", 2), c.reserved.__setitem__(0, 1))) == K.E_ARG
    # planes, then pitches, of in, then of out
    shapes_in, shapes_out = V.plane_shapes(fi, H0, W0), V.plane_shapes(fo, H1, W1)
    for q in range(len(shapes_in)):
        assert call(lambda c, s, d: s.plane.__setitem__(q, None)) == V.E_PLANE
        assert call(lambda c, s, d: s.pitch.__setitem__(q, shapes_in[q][1] * bi - bi)) == V.E_PITCH
        if bi == 2:
            assert call(lambda c, s, d: s.plane.__setitem__(q, s.plane[q] + 1)) == V.E_PLANE
    for q in range(len(shapes_out)):
        assert call(lambda c, s, d: d.plane.__setitem__(q, None)) == V.E_PLANE
        assert call(lambda c, s, d: d.pitch.__setitem__(q, shapes_out[q][1] * bo - bo)) == V.E_PITCH
        if bo == 2:
            assert call(lambda c, s, d: d.pitch.__setitem__(q, shapes_out[q][1] * bo + 1)) == V.E_PITCH
    assert call(lambda c, s, d: (s.pitch.__setitem__(0, 0), s.plane.__setitem__(1, None))) == V.E_PLANE          # in: planes before pitches
    assert call(lambda c, s, d: (s.pitch.__setitem__(0, 0), d.plane.__setitem__(1, None))) == V.E_PITCH          # in before out
    # last: out overlapping in — the last row of a plane on each side (an even address, as 16-bit samples ask)
    assert call(lambda c, s, d: d.plane.__setitem__(1, s.plane[0] + (H0 - 1) * W0 * bi)) == K.E_ARG
    assert call(lambda c, s, d: s.plane.__setitem__(1, d.plane[0] + ((H1 - 1) * W1 + W1 - 2) * bo)) == K.E_ARG
    assert not any(x.any() for x in bufs)


def test_view_argument_errors_and_addresses():
    import fldr_conform as K
    import fldr_video as V
    for f in (("nv12", "bt601", "limited", 8), ("i420", "bt601", "limited", 8), ("nv12", "bt709", "full", 10), ("i420", "bt709", "full", 10)):
        fmt = _fmt(f)
        b = 2 if fmt.bits == 10 else 1
        buf, fr = _host(V, fmt, 20, 30)
        out = V.Frame()
        assert K.view_raw(fr, fmt, 6, 4, out) == 0
        assert out.plane[0] == fr.plane[0] + 4 * fr.pitch[0] + 6 * b and list(out.pitch)[:2] == list(fr.pitch)[:2]
        if f[0] == "nv12":
            assert out.plane[1] == fr.plane[1] + 2 * fr.pitch[1] + 6 * b and not out.plane[2]
        else:
            assert out.plane[1] == fr.plane[1] + 2 * fr.pitch[1] + 3 * b and out.plane[2] == fr.plane[2] + 2 * fr.pitch[2] + 3 * b
        assert K.view_raw(fr, fmt, 0, 0, out) == 0 and [out.plane[p] for p in range(3)] == [fr.plane[p] for p in range(3)]
        for x, y in ((1, 0), (0, 1), (3, 5), (-2, 0), (0, -2)):                 # an odd or negative origin
            assert K.view_raw(fr, fmt, x, y, out) == K.E_ARG, (x, y)
        assert K.view_raw(None, fmt, 0, 0, out) == K.E_ARG and K.view_raw(fr, None, 0, 0, out) == K.E_ARG and K.view_raw(fr, fmt, 0, 0, None) == K.E_ARG
        bad = fmt.copy()
        bad.layout = 2
        assert K.view_raw(fr, bad, 0, 0, out) == V.E_FORMAT and K.view_raw(fr, bad, 1, 0, out) == K.E_ARG
        gone = V.Frame.from_buffer_copy(bytes(fr))
        gone.plane[1] = None
        assert K.view_raw(gone, fmt, 0, 0, out) == V.E_PLANE
        # the binding's view of numpy planes is the same window as the oracle's slices
        g = np.random.default_rng(3)
        planes = tuple(g.integers(0, 200, s).astype(np.uint16 if b == 2 else np.uint8) for s in V.plane_shapes(fmt, 20, 30))
        for got, want in zip(K.view(planes, fmt, 6, 4, (9, 13)), O.view(planes, f[0], 6, 4, (9, 13))):
            assert got.shape == want.shape and np.array_equal(got, want)
    assert K.coefs_raw(None, _fmt(O.FORMATS[0]), np.zeros(7, np.int32)) == K.E_ARG and K.coefs_raw(_fmt(O.FORMATS[0]), _fmt(O.FORMATS[0]), None) == K.E_ARG
    bad = _fmt(O.FORMATS[0])
    bad.matrix = 2
    assert K.coefs_raw(bad, _fmt(O.FORMATS[0]), np.zeros(7, np.int32)) == V.E_FORMAT and K.coefs_raw(_fmt(O.FORMATS[0]), bad, np.zeros(7, np.int32)) == V.E_FORMAT


def _create(l, h, model=None, **kw):
    import fldr_conform as K
    import fldr_video as V
    cfg = K.stream_config((64, 64), V.Format("i420", "bt601"), (96, 128), V.Format("i420", "bt709", depth=10), 24, 60, at=(32, 16))
    for k, v in kw.items():
        if k == "mutate":
            v(cfg)
        elif k in ("out_H", "out_W", "dst_x", "dst_y", "dither"):
            setattr(cfg, k, v)
        else:
            setattr(cfg.rate, k, v)
    before = bytes(cfg)
    rc = l.fldr_conform_create(model, ctypes.byref(cfg), ctypes.byref(h))
    assert bytes(cfg) == before and not h.value                              # an error writes nothing
    return rc


def test_stream_argument_errors_before_any_device_call():
    import fldr_conform as K
    import fldr_rate as R
    import fldr_video as V
    l = K.lib()
    h = ctypes.c_void_p()
    create = lambda **kw: _create(l, h, **kw)
    ratio_bad = dict(in_num=1, in_den=1, out_num=65, out_den=1)              # 65 outputs per pushed frame
    assert create() == K.E_ARG                                               # valid (24 -> 60: B = 5), no model
    assert create(**ratio_bad) == R.E_RATIO
    # fldr_rate_create's checks with its codes, in its order — the ratio of the rates included — before any word of this library
    assert create(H=1) == R.E_ARG and create(device=-1) == R.E_ARG and create(scene=2) == R.E_ARG
    assert create(mutate=lambda c: c.rate.reserved.__setitem__(2, 1)) == R.E_ARG
    assert create(mutate=lambda c: setattr(c.rate.scene_params, "sad_permille", 1001)) == R.E_ARG
    assert create(mutate=lambda c: setattr(c.rate.format, "layout", 3)) == V.E_FORMAT
    for term in ("in_num", "in_den", "out_num", "out_den"):
        assert create(**{term: 0}) == R.E_RATIO and create(**{term: -24}) == R.E_RATIO, term
    assert create(mutate=lambda c: setattr(c.rate.format, "layout", 3), dither=3) == V.E_FORMAT
    assert create(in_num=0, dither=3) == R.E_RATIO and create(in_num=0, out_H=0) == R.E_RATIO
    for field, bad in (("out_H", 0), ("dst_x", 1), ("dither", 2)):
        assert create(**dict(ratio_bad, **{field: bad})) == R.E_RATIO, (field, bad)
    # then this library's own words — seen here with B == 1 and a bad out_format behind them, so that neither a valid configuration going
    # on to the device nor the null model can be what returns E_ARG
    same = dict(in_num=25, out_num=25)
    bad_out = lambda c: setattr(c.out_format, "depth", 9)
    assert create(mutate=bad_out, **same) == V.E_FORMAT
    for field, bad in (("H", 16385), ("W", 16385), ("out_H", 0), ("out_H", 16385), ("out_W", 0), ("out_W", -5), ("out_H", 64 + 14), ("out_W", 64 + 30),
                       ("dst_x", 1), ("dst_x", -2), ("dst_y", 3), ("dst_y", -2), ("dst_x", 66), ("dst_y", 34), ("dither", 2), ("dither", -1)):
        assert create(mutate=bad_out, **dict(same, **{field: bad})) == K.E_ARG, (field, bad)
    for i in range(4):
        assert create(mutate=lambda c: (bad_out(c), c.reserved.__setitem__(i, 1)), **same) == K.E_ARG
    for field, val in (("layout", 2), ("matrix", 2), ("range", -1), ("depth", 12)):
        assert create(mutate=lambda c: setattr(c.out_format, field, val), **same) == V.E_FORMAT, field
    # a NULL model is an argument error exactly where a frame is interpolated (B != 1), after the formats
    assert create(in_num=25, out_num=50) == K.E_ARG and create(in_num=60, out_num=25) == K.E_ARG
    assert create(mutate=bad_out, in_num=25, out_num=50) == V.E_FORMAT
    assert l.fldr_conform_create(None, None, ctypes.byref(h)) == K.E_ARG
    n = ctypes.c_int()
    assert l.fldr_conform_push(None, None, None, ctypes.byref(n), None) == K.E_ARG
    assert l.fldr_conform_flush(None, None, ctypes.byref(n)) == K.E_ARG
    assert l.fldr_conform_reset(None) == K.E_ARG
    assert l.fldr_conform_max_out(None) == K.E_ARG
    l.fldr_conform_destroy(None)


def test_table_builder_alone_under_the_host_sanitizers(tmp_path):
    """conform/conform_coefs.h is host-only: a stand-alone program with its own main, built with -fsanitize=address,undefined, builds the
    table of every pair of (matrix, range, depth) and checks the exact entries, the worked table and the int32 bound."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "conform_coefs_main"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                        "-Wno-unused-function", "-I" + INC, "-I" + os.path.join(PKG, "conform"), "-o", str(exe),
                        os.path.join(ROOT, "tests", "conform_coefs_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    u = subprocess.run([str(exe)], capture_output=True, text=True)
    assert u.returncode == 0 and "coefs ok: 144 tables" in u.stdout, u.stdout + u.stderr
