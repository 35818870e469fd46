"""CPU checks of the 10-bit video path (include/fldr_video.h `depth`, libfldr_video.so): the format and frame checks happen before any
device call, the depth-generic oracle (tests/yuv_hd_oracle.py) is tests/yuv_oracle.py at depth 8 and derives both tables of
yuv_color.h, the int32 accumulators still fit, known colours, the 4:4:4 round trip, the hand-worked tap weights, the containers' unused
bits, the unchanged struct sizes, the headers and the example."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import yuv_hd_oracle as HD
import yuv_oracle as O
from lib_checks import disassemble as _disassemble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fldr-vfi_amd")
INC = os.path.join(ROOT, "include")
LIB = os.path.join(PKG, "libfldr_video.so")
COLOR_H = os.path.join(PKG, "video", "yuv_color.h")
FORMATS = [(m, r) for m in HD.MATRICES for r in HD.RANGES]


# ---- argument checks without a device ---------------------------------------------------------------------------------------------
def _io(V, H=64, W=64, layout="nv12", in_depth=10, out_depth=10):
    buf = np.zeros(H * W * 8 + 64, np.uint8)
    base = (buf.ctypes.data + 15) // 16 * 16
    io = V.IO()
    io.H, io.W = H, W
    io.in_format, io.out_format = V.Format(layout, depth=in_depth), V.Format(layout, depth=out_depth)
    shapes = V.plane_shapes(layout, H, W)
    for f in range(2):
        for p, (r, c) in enumerate(shapes):
            io.in_[f].plane[p], io.in_[f].pitch[p] = base, c * (2 if in_depth == 10 else 1)
    outs = (V.Frame * 1)()
    for p, (r, c) in enumerate(shapes):
        outs[0].plane[p], outs[0].pitch[p] = base, c * (2 if out_depth == 10 else 1)
    io.n_t, io.t, io.out = 1, base, ctypes.cast(outs, ctypes.POINTER(V.Frame))
    io._keep = (buf, outs)
    return io


@pytest.mark.parametrize("layout", ["nv12", "i420"])
def test_depth_is_checked_before_any_device_call(layout):
    """The acceptance test: depth 10 in either format passes the format check (a null model then gives E_ARG; a library without the
    feature gives E_FORMAT for the non-zero word)."""
    import fldr_video as V
    l = V.lib()
    call = lambda io: l.fldr_video_forward(None, ctypes.byref(io), None, 0, None)
    for di, do in ((10, 10), (10, 8), (8, 10), (10, 0), (0, 10)):
        assert call(_io(V, layout=layout, in_depth=di, out_depth=do)) == V.E_ARG, (di, do)
    for bad in (9, 12, 16, -1):
        io = _io(V, layout=layout); io.in_format.depth = bad
        assert call(io) == V.E_FORMAT, bad
        io = _io(V, layout=layout); io.out_format.depth = bad
        assert call(io) == V.E_FORMAT, bad
    for word in (1, 2, 3, 4):                                                   # the four words that stay reserved
        io = _io(V, layout=layout); io.in_format.reserved[word] = 1
        assert call(io) == V.E_FORMAT, word
    nplanes = 2 if layout == "nv12" else 3
    for p in range(nplanes):
        io = _io(V, layout=layout); io.in_[1].pitch[p] += 1                     # odd pitch
        assert call(io) == V.E_PITCH, p
        io = _io(V, layout=layout); io.out[0].pitch[p] += 3
        assert call(io) == V.E_PITCH, p
        io = _io(V, layout=layout); io.in_[0].plane[p] += 1                     # odd plane address
        assert call(io) == V.E_PLANE, p
        io = _io(V, layout=layout); io.out[0].plane[p] += 1
        assert call(io) == V.E_PLANE, p
    io = _io(V, layout=layout); io.in_[0].pitch[0] = 64                         # an 8-bit-sized pitch (W bytes) at depth 10
    assert call(io) == V.E_PITCH
    io = _io(V, layout=layout); io.out[0].pitch[1] = 64 if layout == "nv12" else 32
    assert call(io) == V.E_PITCH
    # at depth 8 odd pitches and addresses stay legal
    io = _io(V, layout=layout, in_depth=8, out_depth=8); io.in_[0].pitch[0] += 1; io.in_[0].plane[0] += 1
    assert call(io) == V.E_ARG
    # sessions: the same format check
    h = ctypes.c_void_p()
    cfg = V.SessionConfig()
    cfg.H, cfg.W, cfg.n_t = 64, 64, 1
    cfg.in_format, cfg.out_format = V.Format(layout, depth=10), V.Format(layout, depth=10)
    assert l.fldr_video_session_create(None, ctypes.byref(cfg), ctypes.byref(h)) == V.E_ARG
    cfg.out_format.depth = 12
    assert l.fldr_video_session_create(None, ctypes.byref(cfg), ctypes.byref(h)) == V.E_FORMAT


def test_struct_sizes_and_versions_are_pinned():
    import fldr_model as M
    import fldr_video as V
    # sizeof(fldr_video_format), fldr_video_frame, fldr_video_io, fldr_video_session_config before `depth` existed
    assert [V.lib().fldr_video_sizeof(i) for i in range(4)] == [32, 48, 192, 104]
    assert [M.lib().fldr_model_sizeof(i) for i in range(3)] == [56, 32, 160]
    assert V.VIDEO_VERSION == 101 and V.lib().fldr_video_version() == 101
    hdr = open(os.path.join(INC, "fldr_video.h")).read()
    assert re.search(r"int32_t\s+depth;", hdr) and re.search(r"int32_t\s+reserved\[4\];", hdr)
    f = V.Format("i420", "bt601", "full", depth=10)
    assert (f.depth, f.reserved[0], f.bits) == (10, 10, 10) and len(f.reserved) == 5 and V.Format.reserved.offset == 12
    assert V.Format().depth == 8 and V.plane_dtype(f, numpy=True) == np.uint16 and V.plane_dtype(V.Format(), numpy=True) == np.uint8


@pytest.mark.parametrize("compiler", [["gcc", "-std=c99", "-x", "c"], ["g++", "-std=c++11", "-x", "c++"]])
def test_header_compiles_and_depth_sits_on_the_first_reserved_word(compiler, tmp_path):
    if not shutil.which(compiler[0]):
        pytest.skip(compiler[0] + " not installed")
    src = tmp_path / "h.c"
    src.write_text('#include <stddef.h>\n#include "fldr_video.h"\n'
                   'typedef char depth_offset[offsetof(fldr_video_format, depth) == 12 ? 1 : -1];\n'
                   'typedef char format_size[sizeof(fldr_video_format) == 32 ? 1 : -1];\n'
                   'int main(void) { fldr_video_format f; f.depth = 10; return f.depth == 10 ? 0 : 1; }\n')
    r = subprocess.run(compiler + ["-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I" + INC, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_example_builds_with_cc_and_knows_p10(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if not cc:
        pytest.skip("no C compiler")
    exe = tmp_path / "fldr_slowmo"
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + INC, "-o", str(exe),
                        os.path.join(ROOT, "examples", "fldr_slowmo.c"), "-L" + PKG, "-l:libfldr_video.so", "-l:libfldr_model.so",
                        "-Wl,-rpath," + PKG], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    u = subprocess.run([str(exe)], capture_output=True, text=True)                 # no arguments: usage, no device touched
    assert u.returncode == 2 and "p10" in u.stderr
    u = subprocess.run([str(exe), "w.npz", "64", "64", "2", "p11"], capture_output=True, text=True)   # an unknown word: usage
    assert u.returncode == 2


def _no_stale_half_packing(lib):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    n, seen = 0, False
    for txt in _disassemble(lib):
        # both kernels in both sample types: Ih / It open the mangled template arguments <unsigned char, ...> / <unsigned short, ...>
        seen = seen or all(k + t in txt for k in ("yuv420_to_planar_pair_kernelI", "planar_to_yuv420_kernelI") for t in "ht")
        n += len(re.findall(r"\bv_ashr_pk_\w+|\bv_cvt_pk_[ui]16_\w+", txt))
    assert seen and n == 0
    ks = KR.kernels(lib)
    assert sum("yuv420" in k["name"] for k in ks) == 16                        # 2 kernels x 2 sample types x 2 layouts x 2 forms
    for k in ks:
        assert k["scratch"] == 0 and k["vgpr_spills"] == 0, k


def test_no_stale_half_packing_in_the_video_library():
    """The 16-bit packing invites v_ashr_pk_* / v_cvt_pk_u16_* / v_cvt_pk_i16_* (video_kernels.hip, pack2h): none may be in the library,
    and the 10-bit kernels are in it."""
    _no_stale_half_packing(LIB)


# ---- the colour definition --------------------------------------------------------------------------------------------------------
def _table(name):
    body = open(COLOR_H).read().split(name + "[2][2] = {", 1)[1]
    rows = re.findall(r"\{([-0-9, ]+)\}", body)[:4]
    return {(("bt601", "bt709")[i // 2], ("limited", "full")[i % 2]): dict(zip(HD.NAMES, (int(v) for v in row.split(","))))
            for i, row in enumerate(rows)}


def test_both_tables_are_derived_from_kr_kb():
    for name, depth in (("YUV_COEFFS", 8), ("YUV_COEFFS_10", 10)):
        t = _table(name)
        assert len(t) == 4
        for (mat, rng), row in t.items():
            assert row == HD.constants(mat, rng, depth), (name, mat, rng)
            sy, _ = HD.scales(rng, depth)
            assert row["KYR"] + row["KYG"] + row["KYB"] == int(np.floor(sy * 65536 + 0.5))
            assert row["KUR"] + row["KUG"] == -row["KUB"] and row["KVG"] + row["KVB"] == -row["KVR"]
            assert HD.constants(mat, rng, 8) == O.constants(mat, rng)
    assert HD.constants("bt709", "limited", 10)["YOFF"] == 64 and abs(HD.scales("limited", 10)[0] - 876 / 1023) < 1e-15


@pytest.mark.parametrize("mat,rng", FORMATS)
@pytest.mark.parametrize("H,W", [(64, 96), (37, 53)])
def test_depth_8_is_the_8_bit_oracle_byte_for_byte(mat, rng, H, W):
    g = np.random.default_rng(H * W)
    bgr = g.integers(0, 256, (3, H, W)).astype(np.uint8)
    a, b = HD.bgr_to_yuv420(bgr, mat, rng, 8), O.bgr_to_yuv420(bgr, mat, rng)
    for x, y in zip(a, b):
        assert x.dtype == np.uint8 and np.array_equal(x, y)
    ch, cw = HD.chroma_size(H, W)
    Y, U, V = g.integers(0, 256, (H, W)).astype(np.uint8), g.integers(0, 256, (ch, cw)).astype(np.uint8), g.integers(0, 256, (ch, cw)).astype(np.uint8)
    assert np.array_equal(HD.yuv420_to_bgr(Y, U, V, mat, rng, 8), O.yuv420_to_bgr(Y, U, V, mat, rng))
    v = g.integers(0, 256, (3, 1000))
    for x, y in zip(HD.rgb_to_yuv444(*v, mat, rng, 8), O.rgb_to_yuv444(*v, mat, rng)):
        assert np.array_equal(x, y)
    for x, y in zip(HD.yuv444_to_rgb(*v, mat, rng, 8), O.yuv444_to_rgb(*v, mat, rng)):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("mat,rng", FORMATS)
@pytest.mark.parametrize("depth", [8, 10])
def test_int32_accumulators_are_bounded_by_their_coefficients(mat, rng, depth):
    """Every int32 accumulator of the four kernels is bounded by the sum of |coefficient| x largest |input| (inputs 0 .. 2^d - 1, the
    centred chroma sums in -8 mid .. 8 (max - mid)), and that bound is below 2^31."""
    k = HD.constants(mat, rng, depth)
    mx, mid = (1 << depth) - 1, 128 << (depth - 8)
    ymax = max(mx - k["YOFF"], k["YOFF"]) * 8 * k["KY"]
    cmax = 8 * max(mid, mx - mid)
    up = [ymax + k["KRV"] * cmax + (1 << 18), ymax + (k["KGU"] + k["KGV"]) * cmax + (1 << 18), ymax + k["KBU"] * cmax + (1 << 18)]
    down = []
    for a, b, c in ((k["KYR"], k["KYG"], k["KYB"]), (k["KUR"], k["KUG"], k["KUB"]), (k["KVR"], k["KVG"], k["KVB"])):
        down.append(8 * (abs(a) + abs(b) + abs(c)) * mx + (1 << 18))                  # eight taps of one plane sum, then the rounding term
    bound = max(up + down)
    assert bound < 2 ** 31, (bound, up, down)
    if depth == 10 and (mat, rng) == ("bt709", "limited"):
        assert up[2] == max(up) and 1.15e9 < up[2] < 1.17e9                           # blue: the tightest, as the header says


@pytest.mark.parametrize("mat,rng", FORMATS)
def test_known_colours_at_depth_10(mat, rng):
    lim = rng == "limited"
    Y, U, V = HD.rgb_to_yuv444([0, 1023, 512, 300], [0, 1023, 512, 300], [0, 1023, 512, 300], mat, rng, 10)
    assert list(Y[:2]) == ([64, 940] if lim else [0, 1023])
    assert list(U) == [512] * 4 and list(V) == [512] * 4                            # grey has no chroma
    y, u, v = HD.bgr_to_yuv420(np.zeros((3, 4, 4), np.uint16), mat, rng, 10)
    assert (int(y[0, 0]), int(u[0, 0]), int(v[0, 0])) == ((64, 512, 512) if lim else (0, 512, 512))
    y, u, v = HD.bgr_to_yuv420(np.full((3, 4, 4), 1023, np.uint16), mat, rng, 10)
    assert (int(y[0, 0]), int(u[0, 0]), int(v[0, 0])) == ((940, 512, 512) if lim else (1023, 512, 512))
    kr, kb = HD.MATRICES[mat]
    sy, sc = (876 / 1023, 896 / 1023) if lim else (1.0, 1.0)
    yoff = 64 if lim else 0
    for rgb in ((1023, 0, 0), (0, 1023, 0), (0, 0, 1023), (0, 1023, 1023), (1023, 0, 1023), (1023, 1023, 0)):
        bgr = np.stack([np.full((4, 4), c, np.uint16) for c in rgb[::-1]])
        y, u, v = HD.bgr_to_yuv420(bgr, mat, rng, 10)
        r, g, b = rgb
        luma = kr * r + (1 - kr - kb) * g + kb * b
        ey = luma * sy + yoff
        eu = min(max(512 + sc * (b - luma) / (2 * (1 - kb)), 0), 1023)
        ev = min(max(512 + sc * (r - luma) / (2 * (1 - kr)), 0), 1023)
        assert np.all(np.abs(y.astype(float) - ey) <= 1) and np.all(np.abs(u.astype(float) - eu) <= 1) and \
            np.all(np.abs(v.astype(float) - ev) <= 1), (rgb, y[0, 0], ey, u[0, 0], eu, v[0, 0], ev)
        assert y.dtype == np.uint16


@pytest.mark.parametrize("mat,rng", FORMATS)
def test_round_trip_444_at_depth_10(mat, rng):
    """The cube's six faces and a seeded million of inner triples (all 2^30 are too many): within test_round_trip_444's bound in codes,
    2 for limited range and 1 for full."""
    v = np.arange(1024, dtype=np.int64)
    A, B = np.meshgrid(v, v, indexing="ij")
    A, B = A.ravel(), B.ravel()
    trip = []
    for fixed in (0, 1023):
        F = np.full_like(A, fixed)
        trip += [(F, A, B), (A, F, B), (A, B, F)]
    g = np.random.default_rng(10)
    trip.append(tuple(g.integers(0, 1024, 1000000) for _ in range(3)))
    err = 0
    for R, G, Bv in trip:
        R2, G2, B2 = HD.yuv444_to_rgb(*HD.rgb_to_yuv444(R, G, Bv, mat, rng, 10), mat, rng, 10)
        err = max(err, int(np.abs(R2 - R).max()), int(np.abs(G2 - G).max()), int(np.abs(B2 - Bv).max()))
    print("4:4:4 round trip at depth 10, %s %s: max error %d codes" % (mat, rng, err))
    assert err <= (2 if rng == "limited" else 1), err


def test_weights_on_a_hand_worked_3x3_frame_at_depth_10():
    """test_weights_on_a_hand_worked_3x3_frame with 10-bit values: the same siting and weights, centre 512."""
    mat, rng = "bt709", "full"
    k = HD.constants(mat, rng, 10)
    U = np.array([[400, 640], [160, 880]], np.uint16)
    Vp = np.full((2, 2), 512, np.uint16)
    Y = np.full((3, 3), 512, np.uint16)
    bgr = HD.yuv420_to_bgr(Y, U, Vp, mat, rng, 10)
    hw = {0: {0: 2}, 1: {0: 1, 1: 1}, 2: {1: 2}}
    vw = {0: {0: 4}, 1: {0: 3, 1: 1}, 2: {0: 1, 1: 3}}
    for yy in range(3):
        for xx in range(3):
            su = sum(wv * wh * int(U[r, c]) for r, wv in vw[yy].items() for c, wh in hw[xx].items())
            cu = su - 8 * 512
            b = min(max((512 * 8 * k["KY"] + k["KBU"] * cu + (1 << 18)) >> 19, 0), 1023)
            assert bgr[0, yy, xx] == b, (xx, yy)
    g = np.random.default_rng(0)
    bgr = g.integers(0, 1024, (3, 3, 3)).astype(np.uint16)
    _, u, v = HD.bgr_to_yuv420(bgr, mat, rng, 10)
    B, G, R = (bgr[c].astype(np.int64) for c in range(3))
    up = k["KUR"] * R + k["KUG"] * G + k["KUB"] * B
    cols = {0: {0: 3, 1: 1}, 1: {1: 1, 2: 3}}
    rows = {0: {0: 1, 1: 1}, 1: {2: 2}}
    for j in range(2):
        for i in range(2):
            s = sum(wr * wc * int(up[r, c]) for r, wr in rows[j].items() for c, wc in cols[i].items())
            assert u[j, i] == min(max(((s + (1 << 18)) >> 19) + 512, 0), 1023), (i, j)
    assert u.shape == v.shape == (2, 2)


@pytest.mark.parametrize("layout", ["nv12", "i420"])
def test_unused_container_bits_do_not_reach_the_colour(layout):
    """P010 with random low six bits and yuv420p10le with random high six bits decode to the BGR of the clean words."""
    g = np.random.default_rng(3)
    H, W = 37, 53
    ch, cw = HD.chroma_size(H, W)
    Y, U, V = (g.integers(0, 1024, s).astype(np.uint16) for s in ((H, W), (ch, cw), (ch, cw)))
    clean = HD.pack_planes(Y, U, V, layout, 10)
    dirty = HD.pack_planes(Y, U, V, layout, 10, dirt=g)
    assert any(not np.array_equal(c, d) for c, d in zip(clean, dirty))
    for planes in (clean, dirty):
        y, u, v = HD.unpack_planes(planes, layout, 10)
        assert np.array_equal(y, Y) and np.array_equal(u, U) and np.array_equal(v, V)
    want = HD.yuv420_to_bgr(Y, U, V, "bt709", "limited", 10)
    assert np.array_equal(HD.yuv420_to_bgr(*HD.unpack_planes(dirty, layout, 10), "bt709", "limited", 10), want)
    if layout == "nv12":
        assert all(int((p & 63).max()) == 0 for p in clean) and int(clean[0].max()) <= 1023 << 6


# ---- the test build and the float64 definition at depth 10 --------------------------------------------------------------------------------
def test_no_stale_half_packing_in_the_video_test_library():
    """The same listing check on libfldr_video_test.so: it is the binary tests/test_gpu_video_convert.py executes."""
    _no_stale_half_packing(os.path.join(PKG, "libfldr_video_test.so"))


@pytest.mark.parametrize("mat,rng", FORMATS)
def test_depth_10_is_within_the_derived_bound_of_the_float_definition(mat, rng):
    """The integer oracle at depth 10 against the float64 definition written from the standard (tests/yuv_float_ref.py): pure triples (the
    cube's six faces and a seeded million, as the round-trip test takes them) through the 4:4:4 forms, and full 4:2:0 noise frames in both
    directions.  Bound, derived from the table: 0.5 + sum over the expression's coefficients of 2^-17 x the largest |operand| = 0.5151
    (limited) / 0.5156 (full) to RGB, 0.5234 to YUV.  Measured maxima over the four formats: 4:4:4 0.5122 to RGB (BT.709 limited), 0.5140
    to YUV (BT.601 limited); 4:2:0 noise 0.5092 to RGB, 0.5104 to YUV."""
    import yuv_float_ref as F
    k = HD.constants(mat, rng, 10)
    up_bound, down_bound = 0.5 + F.coefficient_bound(k, 10, "to_rgb"), 0.5 + F.coefficient_bound(k, 10, "to_yuv")
    assert 0.5 < up_bound < 0.516 and 0.5 < down_bound < 0.524
    v = np.arange(1024, dtype=np.int64)
    A, B = (a.ravel() for a in np.meshgrid(v, v, indexing="ij"))
    trip = []
    for fixed in (0, 1023):
        Fx = np.full_like(A, fixed)
        trip += [(Fx, A, B), (A, Fx, B), (A, B, Fx)]
    g = np.random.default_rng(10)
    trip.append(tuple(g.integers(0, 1024, 1000000) for _ in range(3)))
    eu = ed = 0.0
    for a, b, c in trip:
        eu = max(eu, max(float(np.abs(i - F.clip(f, 10)).max()) for i, f in zip(HD.yuv444_to_rgb(a, b, c, mat, rng, 10), F.ycbcr_to_rgb(a, b, c, mat, rng, 10))))
        ed = max(ed, max(float(np.abs(i - F.clip(f, 10)).max()) for i, f in zip(HD.rgb_to_yuv444(a, b, c, mat, rng, 10), F.rgb_to_ycbcr(a, b, c, mat, rng, 10))))
    nu = nd = 0.0
    for H, W in ((203, 301), (64, 96), (2, 2), (3, 5)):
        g = np.random.default_rng(H * W + 10)
        ch, cw = HD.chroma_size(H, W)
        Y, U, V = (g.integers(0, 1024, s).astype(np.uint16) for s in ((H, W), (ch, cw), (ch, cw)))
        nu = max(nu, float(np.abs(HD.yuv420_to_bgr(Y, U, V, mat, rng, 10) - F.yuv420_to_bgr(Y, U, V, mat, rng, 10)).max()))
        bgr = g.integers(0, 1024, (3, H, W)).astype(np.uint16)
        nd = max(nd, max(float(np.abs(i - f).max()) for i, f in zip(HD.bgr_to_yuv420(bgr, mat, rng, 10), F.bgr_to_yuv420(bgr, mat, rng, 10))))
    print("10-bit, %s %s: max |integer - float| 4:4:4 %.4f to RGB, %.4f to YUV; 4:2:0 noise %.4f to RGB, %.4f to YUV; bounds %.4f, %.4f" % (
        mat, rng, eu, ed, nu, nd, up_bound, down_bound))
    assert max(eu, nu) <= up_bound and max(ed, nd) <= down_bound, (eu, nu, up_bound, ed, nd, down_bound)
