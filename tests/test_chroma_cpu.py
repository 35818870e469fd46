"""CPU checks of the 4:2:2 / 4:4:4 API (include/fldr_chroma.h, libfldr_chroma.so): the library's symbol table and link, the header as plain
C99 / C++, the C example, the binding's struct mirrors, the argument checks (decided before any device call, so they run without a GPU),
the listing of the kernels, and the colour definition of tests/yuv_chroma_oracle.py: against a float64 statement, against the 4:2:0
oracle, its round trip and its int32 headroom."""
import ctypes
import glob
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import yuv_chroma_oracle as C
import yuv_float_ref as F
import yuv_hd_oracle as HD
from lib_checks import declared as _declared, disassemble as _disassemble, syms as _syms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fldr-vfi_amd")
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "fldr_chroma.h")
LIB = os.path.join(PKG, "libfldr_chroma.so")
EXAMPLE_C = os.path.join(ROOT, "examples", "fldr_slowmo_pro.c")
FORMATS = [(m, r) for m in C.MATRICES for r in C.RANGES]


# ---- the library ----------------------------------------------------------------------------------------------------------------
def test_library_exports_exactly_the_header():
    declared = _declared(HDR, "FLDR_CHROMA_API")
    assert len(declared) == 11, sorted(declared)
    assert _syms(LIB, ["--defined-only"]) == declared
    import fldr_chroma
    assert set(fldr_chroma.EXPORTS) == declared and len(fldr_chroma.EXPORTS) == 11


def test_library_links_only_the_model_api():
    dyn = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    needed = re.findall(r"NEEDED.*\[(libfldr_[a-z_]+\.so)\]", dyn)
    assert needed == ["libfldr_model.so"], dyn
    assert re.search(r"R(UN)?PATH.*\$ORIGIN", dyn), dyn
    used = set(n for n in _syms(LIB, ["--undefined-only"]) if n.startswith("fldr_"))
    assert used and used <= _declared(os.path.join(INC, "fldr_model.h"), "FLDR_MODEL_API"), sorted(used)
    assert "fldr_model_forward" in used


@pytest.mark.parametrize("compiler", [["gcc", "-std=c99", "-x", "c"], ["g++", "-std=c++11", "-x", "c++"]])
def test_header_is_plain_c99_and_cxx(compiler, tmp_path):
    assert shutil.which(compiler[0]), compiler[0] + " not installed"
    src = tmp_path / "h.c"
    src.write_text('#include "fldr_chroma.h"\nint main(void) { return fldr_chroma_sizeof(0) > 0 ? 0 : 1; }\n')
    r = subprocess.run(compiler + ["-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I" + INC, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "hip" not in re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S).lower()


def test_nothing_else_mentions_the_library():
    for h in glob.glob(os.path.join(INC, "*.h")):
        if h != HDR:
            assert "fldr_chroma" not in open(h).read().lower(), h
    libs = [l for l in glob.glob(os.path.join(PKG, "libfldr_*.so")) if l != LIB]
    assert len(libs) >= 9, libs
    for l in libs:
        assert not [n for n in _syms(l, []) if "fldr_chroma" in n], l
        assert b"fldr_chroma" not in open(l, "rb").read(), l


def test_binding_struct_sizes_version_and_codes():
    import fldr_chroma as V
    l = V.lib()
    assert l.fldr_chroma_version() == V.CHROMA_VERSION
    text = open(HDR).read()
    assert int(re.search(r"#define FLDR_CHROMA_VERSION (\d+)", text).group(1)) == V.CHROMA_VERSION
    for which, cls in enumerate((V.Format, V.Frame, V.IO, V.SessionConfig)):
        assert l.fldr_chroma_sizeof(which) == ctypes.sizeof(cls)
    assert ctypes.sizeof(V.Format) == 32 and ctypes.sizeof(V.Frame) == 48
    assert l.fldr_chroma_sizeof(4) == V.E_ARG
    for name, v in (("E_ARG", V.E_ARG), ("E_FORMAT", V.E_FORMAT), ("E_PITCH", V.E_PITCH), ("E_PLANE", V.E_PLANE),
                    ("E_WORKSPACE", V.E_WORKSPACE), ("E_DEVICE", V.E_DEVICE)):
        assert re.search(r"#define FLDR_CHROMA_%s\s+\((-?\d+)\)" % name, text).group(1) == str(v)
        assert v <= -700                                                       # below every other library's range
        assert l.fldr_chroma_error_string(v).decode().startswith("fldr_chroma")
    assert l.fldr_chroma_error_string(-3).decode().startswith("fldr_model")   # model codes pass through
    for table, prefix in ((V.SAMPLINGS, ""), (V.LAYOUTS, ""), (V.MATRICES, ""), (V.RANGES, "")):
        for name, v in table.items():
            assert re.search(r"FLDR_CHROMA_%s = %d\b" % (name.upper(), v), text), name
    body = open(os.path.join(PKG, "chroma", "chroma_internal.h")).read()
    assert int(re.search(r"RUN8 = (\d+)", body).group(1)) == V.RUN[8] and int(re.search(r"RUN16 = (\d+)", body).group(1)) == V.RUN[10]


def test_example_builds_with_cc_prints_usage_and_rejects_bad_arguments(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    exe = tmp_path / "fldr_slowmo_pro"
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + INC, "-o", str(exe), EXAMPLE_C, "-L" + PKG,
                        "-l:libfldr_chroma.so", "-l:libfldr_model.so", "-Wl,-rpath," + PKG], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "hip" not in re.sub(r"/\*.*?\*/", "", open(EXAMPLE_C).read(), flags=re.S).lower()
    u = subprocess.run([str(exe)], capture_output=True, text=True)            # no arguments: usage, no device touched
    assert u.returncode == 2 and "usage" in u.stderr
    for bad in (["w.npz", "64", "64", "2"], ["w.npz", "64", "64", "2", "yuv420p"], ["w.npz", "64", "64", "1", "yuv422p"],
                ["w.npz", "1", "64", "2", "yuv422p"], ["w.npz", "64", "64", "2", "uyvy422", "bt2020"],
                ["w.npz", "64", "64", "2", "yuv444p", "bt601", "full", "more"]):
        u = subprocess.run([str(exe)] + bad, capture_output=True, text=True)
        assert u.returncode == 2 and "usage" in u.stderr, bad


# ---- argument errors without a device ---------------------------------------------------------------------------------------------
def _io(V, fmt=None, H=64, W=64):
    fmt = fmt or V.Format()
    buf = np.zeros(H * W * 8, np.uint8)
    io = V.IO()
    io.H, io.W = H, W
    io.in_format, io.out_format = fmt.copy(), fmt.copy()
    b = 2 if fmt.bits == 10 else 1
    shapes = V.plane_shapes(fmt, H, W)
    for f in range(2):
        for p, (r, c) in enumerate(shapes):
            io.in_[f].plane[p], io.in_[f].pitch[p] = buf.ctypes.data, c * b
    outs = (V.Frame * 1)()
    for p, (r, c) in enumerate(shapes):
        outs[0].plane[p], outs[0].pitch[p] = buf.ctypes.data, c * b
    io.n_t, io.t, io.out = 1, buf.ctypes.data, ctypes.cast(outs, ctypes.POINTER(V.Frame))
    io._keep = (buf, outs)
    return io


def _all_formats(V):
    return [V.Format(s, l, depth=d) for s, l, d in C.containers()]


def test_every_container_is_accepted_and_every_bad_field_is_a_format_error():
    import fldr_chroma as V
    l = V.lib()
    call = lambda io: l.fldr_chroma_forward(None, ctypes.byref(io), None, 0, None)
    assert len(_all_formats(V)) == 10
    for fmt in _all_formats(V):
        assert call(_io(V, fmt)) == V.E_ARG                                   # valid io, no model
        for side in ("in_format", "out_format"):
            for field, val in (("sampling", 2), ("sampling", -1), ("layout", 4), ("layout", -1), ("matrix", 2), ("range", 2), ("depth", 12),
                               ("depth", 16), ("depth", 9)):
                io = _io(V, fmt); setattr(getattr(io, side), field, val)
                assert call(io) == V.E_FORMAT, (side, field, val)
            for w in range(3):
                io = _io(V, fmt); getattr(io, side).reserved[w] = 1
                assert call(io) == V.E_FORMAT
    io = _io(V); io.in_format.depth = 0                                        # 0 is an alias of 8
    assert call(io) == V.E_ARG
    for layout in ("uyvy", "yuyv"):
        io = _io(V, V.Format("422", layout)); io.in_format.depth = 10          # a packed layout at depth 10
        assert call(io) == V.E_FORMAT
        io = _io(V, V.Format("422", layout)); io.out_format.sampling = 1       # a packed layout at 4:4:4
        assert call(io) == V.E_FORMAT
    # the converters refuse the same formats, before looking at anything else they would touch
    fr, bad = V.Frame(), V.Format("444", "uyvy")
    buf = np.zeros(64, np.uint8)
    fr.plane[0], fr.pitch[0] = buf.ctypes.data, 64
    assert l.fldr_chroma_to_planar(ctypes.byref(fr), 1, ctypes.byref(bad), ctypes.c_void_p(buf.ctypes.data), 4, 4, None) == V.E_FORMAT
    assert l.fldr_chroma_from_planar(ctypes.c_void_p(buf.ctypes.data), ctypes.byref(bad), ctypes.byref(fr), 4, 4, None) == V.E_FORMAT


def test_pitch_plane_and_argument_errors_before_any_device_call():
    import fldr_chroma as V
    l = V.lib()
    call = lambda io: l.fldr_chroma_forward(None, ctypes.byref(io), None, 0, None)
    for fmt in _all_formats(V):
        b = 2 if fmt.bits == 10 else 1
        shapes = V.plane_shapes(fmt, 64, 63)                                   # W = 63: chroma rows are ceil(W/2) = 32 samples at 4:2:2
        for p, (r, c) in enumerate(shapes):
            io = _io(V, fmt, W=63); io.in_[1].pitch[p] = c * b - 1
            assert call(io) == V.E_PITCH, p
            io = _io(V, fmt, W=63); io.out[0].pitch[p] = c * b - b
            assert call(io) == V.E_PITCH, p
            io = _io(V, fmt, W=63); io.in_[0].plane[p] = None
            assert call(io) == V.E_PLANE, p
            io = _io(V, fmt, W=63); io.out[0].plane[p] = None
            assert call(io) == V.E_PLANE, p
            if b == 2:                                                         # 16-bit words: odd pitches and odd addresses
                io = _io(V, fmt, W=63); io.in_[0].pitch[p] = c * b + 3
                assert call(io) == V.E_PITCH, p
                io = _io(V, fmt, W=63); io.out[0].plane[p] = io.out[0].plane[p] + 1
                assert call(io) == V.E_PLANE, p
            else:
                io = _io(V, fmt, W=63); io.in_[0].pitch[p] = c * b + 3; io.in_[0].plane[p] = io.in_[0].plane[p] + 1
                assert call(io) == V.E_ARG, p                                  # fine at depth 8: only the model is missing
        for p in range(len(shapes), 3):                                        # planes the layout does not have are not looked at
            io = _io(V, fmt, W=63); io.in_[0].plane[p] = None; io.in_[0].pitch[p] = 0
            assert call(io) == V.E_ARG
        io = _io(V, fmt); io.n_t = 0
        assert call(io) == V.E_ARG
        io = _io(V, fmt); io.t = None
        assert call(io) == V.E_ARG
        io = _io(V, fmt); io.W = 1
        assert call(io) == V.E_ARG
    assert l.fldr_chroma_forward(None, None, None, 0, None) == V.E_ARG
    assert l.fldr_chroma_workspace_bytes(None, 64, 64, 1) == V.E_ARG
    # the packed row is 4 ceil(W/2) bytes: W = 63 -> 128
    assert V.plane_shapes(V.Format("422", "uyvy"), 64, 63) == [(64, 128)]
    # the converters alone
    fmt = V.Format("422", "semiplanar", depth=10)
    buf = np.zeros(4096, np.uint8)
    fr = V.Frame()
    for p in range(2):
        fr.plane[p], fr.pitch[p] = buf.ctypes.data, 16
    to = lambda fr_, planar, H=4, W=8, n=1: l.fldr_chroma_to_planar(ctypes.byref(fr_), n, ctypes.byref(fmt), planar, H, W, None)
    frm = lambda fr_, planar, H=4, W=8: l.fldr_chroma_from_planar(planar, ctypes.byref(fmt), ctypes.byref(fr_), H, W, None)
    ok = ctypes.c_void_p(buf.ctypes.data)
    assert to(fr, None) == V.E_ARG and frm(fr, None) == V.E_ARG
    assert to(fr, ok, H=0) == V.E_ARG and frm(fr, ok, W=0) == V.E_ARG and to(fr, ok, n=0) == V.E_ARG
    assert to(fr, ctypes.c_void_p(buf.ctypes.data + 1)) == V.E_ARG            # uint16 planar frames at an odd address
    fr.pitch[1] = 14
    assert to(fr, ok) == V.E_PITCH and frm(fr, ok) == V.E_PITCH
    fr.pitch[1] = 16; fr.plane[0] = buf.ctypes.data + 1
    assert to(fr, ok) == V.E_PLANE and frm(fr, ok) == V.E_PLANE


def test_session_argument_errors_before_any_device_call():
    import fldr_chroma as V
    l = V.lib()
    h = ctypes.c_void_p()
    cfg = V.SessionConfig()
    cfg.H, cfg.W, cfg.n_t = 64, 64, 1
    cfg.in_format, cfg.out_format = V.Format("422", "planar", depth=10), V.Format("444", "planar")
    create = lambda: l.fldr_chroma_session_create(None, ctypes.byref(cfg), ctypes.byref(h))
    assert create() == V.E_ARG
    cfg.reserved[1] = 1
    assert create() == V.E_FORMAT
    cfg.reserved[1] = 0
    cfg.out_format.layout = 2                                                  # uyvy at 4:4:4
    assert create() == V.E_FORMAT
    cfg.out_format.layout = 0
    cfg.n_t = 0
    assert create() == V.E_ARG
    assert l.fldr_chroma_session_push(None, None, None, None) == V.E_ARG and l.fldr_chroma_session_reset(None) == V.E_ARG
    l.fldr_chroma_session_destroy(None)


# ---- the listing ----------------------------------------------------------------------------------------------------------------
def test_kernels_use_no_scratch_no_lds_and_leave_four_waves_per_simd():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    ks = KR.kernels(LIB)
    names = [k["name"] for k in ks]
    # one input and one output kernel per sample width (h / t in the mangled name), each in 6 / 4 (sampling, layout) pairs and two forms
    for stem, n8, n16 in (("chroma_to_planar_kernelI", 12, 8), ("chroma_from_planar_kernelI", 12, 8)):
        assert sum(stem + "h" in n for n in names) == n8 and sum(stem + "t" in n for n in names) == n16, names
    assert len(ks) == 40
    for k in ks:
        assert k["scratch"] == 0 and k["vgpr_spills"] == 0 and k["sgpr_spills"] == 0 and k["lds"] == 0, k
        assert k["vgpr"] + k["agpr"] <= 128, k                                 # 512 / 128: four waves per SIMD


def test_listing_has_the_wide_accesses_and_no_stale_half_packing():
    """v_ashr_pk_* / v_cvt_pk_[ui]16_* leave upper bits stale on gfx950 (video_kernels.hip, pack4): none may be in the library; the wide
    forms show as 8- and 16-byte loads and stores."""
    texts = _disassemble(LIB)
    assert texts and any("chroma_to_planar_kernel" in t and "chroma_from_planar_kernel" in t for t in texts)
    n = sum(len(re.findall(r"\bv_ashr_pk_\w+|\bv_cvt_pk_[ui]16_\w+", t)) for t in texts)
    assert n == 0
    for ins in ("global_load_dwordx2", "global_load_dwordx4", "global_store_dwordx2", "global_store_dwordx4", "v_perm_b32"):
        assert any(ins in t for t in texts), ins


def test_no_unsafe_packed_fp32_in_the_library():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_pk_opsel.py"), LIB], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


# ---- the colour definition --------------------------------------------------------------------------------------------------------
def _up_h(Cp, W):
    """A 4:2:2 chroma plane [H, ceil(W/2)] -> [H, W] float64, from the definition: chroma sample i sits on luma column 2 i, so an even
    luma column takes its sample and an odd one the mean of its two neighbours (linear interpolation; the row's last sample repeats)."""
    Cp = np.asarray(Cp, np.float64)
    cw = Cp.shape[1]
    out = np.empty((Cp.shape[0], W))
    for x in range(W):
        pos = x / 2.0
        i0 = int(np.floor(pos))
        f = pos - i0
        out[:, x] = (1.0 - f) * Cp[:, min(i0, cw - 1)] + f * Cp[:, min(i0 + 1, cw - 1)]
    return out


def _down_h(P):
    """A full-resolution plane [H, W] -> [H, ceil(W/2)] float64, from the definition: (1, 2, 1) / 4 around luma column 2 i, the row's
    edge samples repeating."""
    P = np.asarray(P, np.float64)
    W = P.shape[1]
    out = np.empty((P.shape[0], (W + 1) // 2))
    for i in range(out.shape[1]):
        out[:, i] = 0.25 * P[:, max(2 * i - 1, 0)] + 0.5 * P[:, 2 * i] + 0.25 * P[:, min(2 * i + 1, W - 1)]
    return out


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("mat,rng", FORMATS)
def test_oracle_is_within_the_derived_bound_of_the_float_definition(mat, rng, depth):
    """The integer oracle against the float64 definition (tests/yuv_float_ref.py's matrices, the horizontal resampling above) on noise
    frames, both samplings, both directions.  Bound, derived as tests/test_video10_cpu.py derives its own: the rounding's half code plus,
    per output expression, the sum over its 16-bit coefficients of 2^-17 x the largest |operand| (coefficient_bound); the taps add nothing,
    their weights are exact in binary.  That is 0.5 + 0.0039 (depth 8) / 0.0156 (depth 10) to RGB at most, 0.5 + 0.0058 / 0.0234 to YUV.
    Measured maxima over the four colour formats: depth 8 0.5010 to RGB, 0.5014 to YUV; depth 10 0.5080 to RGB, 0.5116 to YUV."""
    k = C.constants(mat, rng, depth)
    up_bound, down_bound = 0.5 + F.coefficient_bound(k, depth, "to_rgb"), 0.5 + F.coefficient_bound(k, depth, "to_yuv")
    assert 0.5 < up_bound < 0.516 and 0.5 < down_bound < 0.524
    mx = (1 << depth) - 1
    eu = ed = 0.0
    for sampling in C.SAMPLINGS:
        for H, W in ((37, 301), (8, 96), (1, 1), (2, 2), (3, 5)):
            g = np.random.default_rng(H * W + depth)
            cw = C.chroma_width(sampling, W)
            Y, U, V = (g.integers(0, mx + 1, s).astype(C.dtype_of(depth)) for s in ((H, W), (H, cw), (H, cw)))
            Uf, Vf = (U.astype(np.float64), V.astype(np.float64)) if sampling == "444" else (_up_h(U, W), _up_h(V, W))
            R, G, B = F.ycbcr_to_rgb(Y.astype(np.float64), Uf, Vf, mat, rng, depth)
            ref = np.stack([F.clip(B, depth), F.clip(G, depth), F.clip(R, depth)])
            eu = max(eu, float(np.abs(C.yuv_to_bgr(Y, U, V, sampling, mat, rng, depth) - ref).max()))
            bgr = g.integers(0, mx + 1, (3, H, W)).astype(C.dtype_of(depth))
            Yf, Cb, Cr = F.rgb_to_ycbcr(bgr[2].astype(np.float64), bgr[1].astype(np.float64), bgr[0].astype(np.float64), mat, rng, depth)
            if sampling == "422":
                Cb, Cr = _down_h(Cb), _down_h(Cr)
            for i, f in zip(C.bgr_to_yuv(bgr, sampling, mat, rng, depth), (Yf, Cb, Cr)):
                ed = max(ed, float(np.abs(i - F.clip(f, depth)).max()))
    print("depth %d, %s %s: max |integer - float| %.4f to RGB (bound %.4f), %.4f to YUV (bound %.4f)" % (depth, mat, rng, eu, up_bound, ed, down_bound))
    assert eu <= up_bound and ed <= down_bound, (eu, up_bound, ed, down_bound)


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("mat,rng", FORMATS)
def test_oracle_is_the_420_oracle_when_row_pairs_are_equal(mat, rng, depth):
    """Exact ties to tests/yuv_hd_oracle.py: with every 4:2:0 chroma row serving two luma rows the vertical taps (1, 3) / (3, 1) land on
    equal rows only if neighbouring chroma rows are equal too, so all chroma rows are equal here; and a BGR frame whose rows 2j, 2j + 1 are
    equal down-converts at 4:2:0 to the 4:2:2 conversion's row 2j."""
    mx = (1 << depth) - 1
    for H, W in ((6, 7), (5, 16), (2, 2), (9, 33)):
        g = np.random.default_rng(H * W)
        ch, cw = HD.chroma_size(H, W)
        Y = g.integers(0, mx + 1, (H, W)).astype(C.dtype_of(depth))
        U, V = (np.repeat(g.integers(0, mx + 1, (1, cw)), ch, axis=0).astype(C.dtype_of(depth)) for _ in range(2))
        U2, V2 = (np.repeat(P, 2, axis=0)[:H] for P in (U, V))               # the 4:2:2 planes: U, V repeated by rows
        assert np.array_equal(HD.yuv420_to_bgr(Y, U, V, mat, rng, depth), C.yuv_to_bgr(Y, U2, V2, "422", mat, rng, depth))
        rows = g.integers(0, mx + 1, (3, ch, W)).astype(C.dtype_of(depth))
        bgr = np.repeat(rows, 2, axis=1)[:, :H]
        y0, u0, v0 = HD.bgr_to_yuv420(bgr, mat, rng, depth)
        y2, u2, v2 = C.bgr_to_yuv(bgr, "422", mat, rng, depth)
        assert np.array_equal(y0, y2) and np.array_equal(u0, u2[0::2]) and np.array_equal(v0, v2[0::2])


@pytest.mark.parametrize("mat,rng", FORMATS)
def test_444_planes_are_the_hd_oracles_and_round_trip(mat, rng):
    """The 4:4:4 forms are yuv444_to_rgb / rgb_to_yuv444 unchanged; RGB -> YUV -> RGB is off by at most 2 codes (limited) / 1 (full), as
    documented for 4:2:0, over every 8-bit triple and, at depth 10, the cube's faces and a seeded million."""
    v = np.arange(256, dtype=np.int64)
    R, G, B = (a.reshape(256, -1) for a in np.meshgrid(v, v, v, indexing="ij"))
    bgr = np.stack([B, G, R]).astype(np.uint8)
    Y, U, V = C.bgr_to_yuv(bgr, "444", mat, rng)
    for a, b in zip((Y, U, V), HD.rgb_to_yuv444(R, G, B, mat, rng)):
        assert np.array_equal(a, b)
    back = C.yuv_to_bgr(Y, U, V, "444", mat, rng)
    for a, b in zip(back[::-1], HD.yuv444_to_rgb(Y, U, V, mat, rng)):
        assert np.array_equal(a, b)
    tol = 2 if rng == "limited" else 1
    assert np.abs(back.astype(int) - bgr.astype(int)).max() <= tol
    g = np.random.default_rng(44)
    A, Bq = (a.reshape(1024, -1) for a in np.meshgrid(np.arange(1024), np.arange(1024), indexing="ij"))
    trips = [np.stack([g.integers(0, 1024, (1000, 1000)) for _ in range(3)])]
    for fixed in (0, 1023):
        Fx = np.full_like(A, fixed)
        trips += [np.stack([Fx, A, Bq]), np.stack([A, Fx, Bq]), np.stack([A, Bq, Fx])]
    for t in trips:
        t = t.astype(np.uint16)
        back = C.yuv_to_bgr(*C.bgr_to_yuv(t, "444", mat, rng, 10), "444", mat, rng, 10)
        assert np.abs(back.astype(int) - t.astype(int)).max() <= tol


@pytest.mark.parametrize("mat,rng", FORMATS)
def test_int32_headroom_at_depth_10(mat, rng):
    """Every accumulator of both kernels at the extreme triples of depth 10 (each operand at 0, the offsets and 1023; the chroma sums at
    their extremes: all taps equal, the weights sum to 8 as at 4:2:0) stays inside int32, below the 1.16e9 INTEGRATION.md documents."""
    k = C.constants(mat, rng, 10)
    ext = np.array([0, 64, 512, 940, 960, 1023], dtype=np.int64)
    A, B_, Cc = np.meshgrid(ext, ext, ext, indexing="ij")
    yv = (A - k["YOFF"]) * 8 * k["KY"]
    cu, cv = 4 * (B_ + B_) - 8 * 512, 4 * (Cc + Cc) - 8 * 512
    m = 0
    for acc in (yv, yv + k["KRV"] * cv + (1 << 18), yv - k["KGU"] * cu, yv - k["KGU"] * cu - k["KGV"] * cv + (1 << 18),
                yv + k["KBU"] * cu + (1 << 18), k["KRV"] * cv, k["KBU"] * cu, k["KGU"] * cu, k["KGV"] * cv):
        m = max(m, int(np.abs(acc).max()))
    for kr, kg, kb in ((k["KYR"], k["KYG"], k["KYB"]), (k["KUR"], k["KUG"], k["KUB"]), (k["KVR"], k["KVG"], k["KVB"])):
        p = kr * A + kg * B_ + kb * Cc
        s = 2 * (p + 2 * p + p)
        m = max(m, int(np.abs(s + (1 << 18)).max()), int(np.abs(kr * A + kg * B_).max()), int(np.abs(p).max()), int(np.abs(4 * p).max()))
    assert m < 2 ** 31 - 1 and m <= 1.16e9, m


def test_pack_and_unpack_are_inverse_and_dirt_stays_out_of_the_values():
    g = np.random.default_rng(3)
    for s, l, d in C.containers():
        for H, W in ((3, 7), (2, 8), (1, 1)):
            mx = (1 << d) - 1
            cw = C.chroma_width(s, W)
            Y, U, V = (g.integers(0, mx + 1, sh).astype(C.dtype_of(d)) for sh in ((H, W), (H, cw), (H, cw)))
            clean, dirty = C.pack(Y, U, V, s, l, d), C.pack(Y, U, V, s, l, d, dirt=g)
            for planes in (clean, dirty):
                for a, b in zip(C.unpack(planes, s, l, W, d), (Y, U, V)):
                    assert np.array_equal(a, b), (s, l, d)
            if l in ("uyvy", "yuyv"):
                assert clean[0].shape == (H, 4 * ((W + 1) // 2))
                if W % 2:
                    assert np.array_equal(clean[0][:, -2 if l == "yuyv" else -1], Y[:, -1])    # the spare luma byte: a copy of the last
