"""CPU checks of the linear-light API (include/fldr_light.h, libfldr_light.so): the built-in tables against the float64 curves of
tests/light_oracle.py, the oracle itself on hand-worked samples, the library's symbol table and link, the header as plain C99 / C++,
the C example, the code-generation guards, the binding's struct mirror, and the argument checks — which happen before any device
call, so they run without a GPU."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import light_oracle as LO
import shutter_oracle as SO
from lib_checks import declared as _declared, disassemble as _disassemble, syms as _syms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fldr-vfi_amd")
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "fldr_light.h")
LIB = os.path.join(PKG, "libfldr_light.so")


# ---- the tables -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("transfer", LO.TRANSFERS)
def test_builtin_tables_follow_the_curves(transfer, depth):
    """Strictly increasing from 0 to at most S; within 1 of the oracle's rounded value wherever the + 1 floor is not active — where the
    oracle's own rounded values are already increasing.  libm enters nowhere else, and +-1 is its allowance."""
    import fldr_light as L
    lin = L.table(transfer, depth).astype(np.int64)
    n = 1 << depth
    assert lin.shape == (n,) and lin[0] == 0 and lin[-1] <= LO.S
    assert (np.diff(lin) > 0).all()
    want = LO.rounded(transfer, depth)
    ref = LO.table(transfer, depth)                                 # the whole rule, floor included
    free = ref == want                                              # the floor is not active: the curve alone carries the table
    free[0] = False
    assert free.sum() > n // 2, "the check would look at too little of the table"
    assert np.abs(lin - want)[free].max() <= 1, (transfer, depth)
    assert lin[-1] >= LO.S - 1                                      # light 1 at the top code
    if transfer == "pq" and depth == 10:                            # what the header says about this table
        assert 12 <= (ref != want).sum() <= 60 and (lin[:20] == np.arange(20)).all()        # the floor carries the first few dozen codes
    assert (L.table(transfer, 0) == L.table(transfer, 8)).all()     # depth 0 is 8


def test_table_argument_errors():
    import fldr_light as L
    l = L.lib()
    buf = (ctypes.c_uint32 * 1024)()
    assert l.fldr_light_table(0, 8, None) == L.E_ARG
    assert l.fldr_light_table(3, 8, buf) == L.E_ARG and l.fldr_light_table(-1, 8, buf) == L.E_ARG      # TABLE has no built-in table
    assert l.fldr_light_table(0, 9, buf) == L.E_ARG and l.fldr_light_table(0, 12, buf) == L.E_ARG


# ---- the oracle on hand-worked samples --------------------------------------------------------------------------------------------------
def test_oracle_white_crossing_black_for_half_the_window():
    """GAMMA24 at depth 8, equal weights on codes 0 and 255: 255 x 0.5^(1/2.4) = 191.04 -> 191; the code-value average gives 128."""
    lin = LO.table("gamma24", 8)
    codes = [np.zeros((3, 1, 1), np.uint8), np.full((3, 1, 1), 255, np.uint8)]
    got = LO.resolve_codes(LO.accumulate_codes(codes, [1, 1], lin), 2, lin)
    assert got.tolist() == [[[191]]] * 3
    assert abs(255 * 0.5 ** (1 / 2.4) - 191.04) < 0.01
    assert SO.mix([(codes[0][0],), (codes[1][0],)], [1, 1], "i420", 8)[0].tolist() == [[128]]
    lin10 = LO.table("gamma24", 10)
    c10 = [np.zeros((3, 1, 1), np.uint16), np.full((3, 1, 1), 1023, np.uint16)]
    assert LO.resolve_codes(LO.accumulate_codes(c10, [1, 1], lin10), 2, lin10).tolist() == [[[766]]] * 3     # 1023 x 0.5^(1/2.4) = 766.4


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("transfer", LO.TRANSFERS)
def test_oracle_one_frame_resolves_to_its_own_codes(transfer, depth):
    lin = LO.table(transfer, depth)
    codes = np.arange(1 << depth).reshape(1, 1, -1)
    for w in (1, 7, 255):
        assert np.array_equal(LO.resolve_codes(LO.accumulate_codes([codes], [w], lin), w, lin), codes), w


def test_oracle_a_tie_goes_up():
    lin = np.array([0, 10, 20, 31], np.int64)                       # mid = 10, 30, 51
    assert LO.mid_of(lin).tolist() == [10, 30, 51]
    r = lambda acc, total: int(LO.resolve_codes(np.array([acc]), total, lin)[0])
    assert r(5, 1) == 1                                             # 2 q = 10 = mid[1]: halfway between entries 0 and 1, up
    assert r(4, 1) == 0
    assert r(15, 1) == 2 and r(14, 1) == 1
    assert r(25, 1) == 2 and r(26, 1) == 3                          # mid[3] = 51 is odd: 2 q = 50 stays below, 52 is above
    assert r(29, 2) == 2                                            # q = (58 + 2) // 4 = 15: a half rounds up, then the tie goes up
    assert r(27, 2) == 1                                            # q = 14


def test_oracle_converter_marks_lone_input_frames():
    outs = LO.outputs(12, 120, 24, 1, 1, cuts=(6,))                 # frames 0 .. 4; 5 alone; 10, 11
    assert [(len(o["points"]), o["unchanged"]) for o in outs] == [(5, None), (1, 5), (2, None)]
    outs = LO.outputs(4, 60, 24, (1, 2), 4, cuts=(1,))
    assert outs[0]["points"] == [(0, 0, None), (0, 1, 0)] and outs[0]["unchanged"] is None


# ---- the library ------------------------------------------------------------------------------------------------------------------------
def test_library_exports_exactly_the_header():
    declared = _declared(HDR, "FLDR_LIGHT_API")
    assert len(declared) == 19, sorted(declared)
    assert _syms(LIB, ["--defined-only"]) == declared
    import fldr_light
    assert set(fldr_light.EXPORTS) == declared


def test_library_links_only_the_shutter_rate_video_and_model_apis():
    dyn = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    for name in ("shutter", "rate", "video"):
        assert re.search(r"NEEDED.*\[libfldr_%s\.so\]" % name, dyn), dyn
    assert not re.search(r"NEEDED.*\[libfldr_hip\.so\]", dyn), dyn
    assert re.search(r"R(UN)?PATH.*\$ORIGIN", dyn), dyn
    used = set(n for n in _syms(LIB, ["--undefined-only"]) if n.startswith("fldr_"))
    allowed = set()
    for h, macro in (("fldr_shutter.h", "FLDR_SHUTTER_API"), ("fldr_rate.h", "FLDR_RATE_API"), ("fldr_video.h", "FLDR_VIDEO_API"),
                     ("fldr_model.h", "FLDR_MODEL_API")):
        allowed |= _declared(os.path.join(INC, h), macro)
    assert used and used <= allowed, sorted(used)
    assert {"fldr_video_forward", "fldr_scene_measure", "fldr_shutter_error_string"} <= used


def test_the_libraries_below_keep_their_exports():
    """The shutter library shares its converter with this one and must come out with the same face; no lower header or library knows
    of fldr_light."""
    assert _syms(os.path.join(PKG, "libfldr_shutter.so"), ["--defined-only"]) == _declared(os.path.join(INC, "fldr_shutter.h"), "FLDR_SHUTTER_API")
    for name in ("fldr_hip.h", "fldr_model.h", "fldr_video.h", "fldr_rate.h", "fldr_shutter.h"):
        assert "fldr_light" not in open(os.path.join(INC, name)).read(), name
    for name in ("libfldr_hip.so", "libfldr_model.so", "libfldr_video.so", "libfldr_rate.so", "libfldr_shutter.so"):
        assert not [n for n in _syms(os.path.join(PKG, name), []) if "fldr_light" in n], name


@pytest.mark.parametrize("compiler", [["gcc", "-std=c99", "-x", "c"], ["g++", "-std=c++11", "-x", "c++"]])
def test_header_is_plain_c99_and_cxx(compiler, tmp_path):
    if not shutil.which(compiler[0]):
        pytest.skip(compiler[0] + " not installed")
    src = tmp_path / "h.c"
    src.write_text('#include "fldr_light.h"\nint main(void) { return fldr_light_sizeof(0) > 0 && FLDR_LIGHT_MAX_TOTAL == 255 ? 0 : 1; }\n')
    r = subprocess.run(compiler + ["-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I" + INC, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "hip/" not in open(HDR).read()


def test_example_builds_with_cc(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if not cc:
        pytest.skip("no C compiler")
    exe = tmp_path / "fldr_cine_linear"
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + INC, "-o", str(exe),
                        os.path.join(ROOT, "examples", "fldr_cine_linear.c"), "-L" + PKG, "-l:libfldr_light.so", "-l:libfldr_shutter.so",
                        "-l:libfldr_rate.so", "-l:libfldr_video.so", "-l:libfldr_model.so", "-Wl,-rpath," + PKG], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    src = open(os.path.join(ROOT, "examples", "fldr_cine_linear.c")).read()
    assert "hip" not in re.sub(r"/\*.*?\*/", "", src, flags=re.S).lower()
    for transfer in ("gamma", "pq", "hlg"):
        assert '"%s"' % transfer in src
    for args in ([], ["w.npz", "64", "64", "120/0", "24"], ["w.npz", "64", "64", "120", "24", "angle=0"], ["w.npz", "64", "64", "120", "24", "sub=65"],
                 ["w.npz", "64", "64", "120", "24", "srgb"]):
        u = subprocess.run([str(exe)] + args, capture_output=True, text=True)             # usage, no device touched
        assert u.returncode == 2 and "usage" in u.stderr, args


def test_no_unsafe_packed_fp32_in_the_light_library():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_pk_opsel.py"), LIB], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_kernels_read_and_write_wide_and_search_in_lds():
    txt = "\n".join(_disassemble(LIB))
    for name in ("light_accumulate_kernel", "light_resolve_kernel", "light_mix_kernel"):
        assert name in txt
    assert len(re.findall(r"\bv_pk_(add|mul|fma)_f32\b", txt)) == 0                     # no packed fp32
    assert re.search(r"\bglobal_load_dwordx4\b", txt) and re.search(r"\bglobal_store_dwordx4\b", txt)
    assert not re.search(r"\bscratch_(load|store)_", txt)
    assert re.search(r"\bds_read_b32\b", txt) or re.search(r"\bds_load_b32\b", txt)     # the tables are read from LDS


def test_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    ks = KR.kernels(LIB)
    mine = [k for k in ks if "light_" in k["name"]]
    assert len(mine) == 10, [k["name"] for k in ks]       # accumulate, mix x (2 depths x wide / per-sample), resolve x 2 depths
    assert len(ks) == 10 + 16, [k["name"] for k in ks]    # and the video library's converters, compiled in
    for k in ks:
        assert k.get("scratch", -1) == 0 and k.get("vgpr_spills", -1) == 0 and k.get("sgpr_spills", -1) == 0, k
    for k in mine:
        assert k["vgpr"] <= 128, k                         # at least four waves per SIMD
        assert 1024 <= k["lds"] <= 8192, k                 # one or both tables: 1 KB each at depth 8, 4 KB at depth 10


def test_binding_struct_sizes_and_version():
    import fldr_light as L
    import fldr_shutter as T
    l = L.lib()
    text = open(HDR).read()
    assert l.fldr_light_version() == L.LIGHT_VERSION == int(re.search(r"#define FLDR_LIGHT_VERSION (\d+)", text).group(1)) == 100
    assert l.fldr_light_sizeof(0) == ctypes.sizeof(L.LightConfig) == (ctypes.sizeof(T.ShutterConfig) + 7) // 8 * 8 + 8
    assert l.fldr_light_sizeof(1) == L.E_ARG
    for name, v in (("E_ARG", L.E_ARG), ("E_CURVE", L.E_CURVE), ("E_TABLE", L.E_TABLE), ("E_ACC", L.E_ACC), ("E_WEIGHT", L.E_WEIGHT),
                    ("E_RATIO", L.E_RATIO), ("E_DEVICE", L.E_DEVICE), ("E_FORMAT", L.E_FORMAT)):
        assert re.search(r"#define FLDR_LIGHT_%s\s+\((-?\d+)\)" % name, text).group(1) == str(v)
        assert v <= -400                                                       # apart from the ranges of the libraries below
        assert l.fldr_light_error_string(v).decode().startswith("fldr_light")
    assert int(re.search(r"#define FLDR_LIGHT_MAX_TOTAL\s+(\d+)", text).group(1)) == L.MAX_TOTAL == 255
    assert int(re.search(r"#define FLDR_LIGHT_SCALE\s+(\d+)", text).group(1)) == L.SCALE == LO.S
    assert L.MAX_TOTAL * L.SCALE < 2 ** 32
    for code, prefix in ((-303, "fldr_shutter"), (-203, "fldr_rate"), (-101, "fldr_video"), (-3, "fldr_model")):
        assert l.fldr_light_error_string(code).decode().startswith(prefix)      # lower layers' codes pass through
    assert l.fldr_light_error_string(0).decode() == "success"
    for name in re.findall(r"FLDR_LIGHT_(GAMMA24|PQ|HLG|TABLE)\s*=\s*(\d)", text):
        assert L.TRANSFERS[name[0].lower()] == int(name[1])


def test_acc_and_scratch_bytes():
    import fldr_light as L
    import fldr_video as V
    al = lambda v: (v + 255) // 256 * 256
    for H, W in ((2, 2), (3, 5), (1080, 1920), (2159, 3837)):
        assert L.acc_bytes(H, W) == al(12 * H * W)
        for depth in (8, 10):
            b = 2 if depth == 10 else 1
            # the planar pair, one planar frame, the accumulator a long mix runs through
            assert L.scratch_bytes(H, W, V.Format("nv12", depth=depth)) == al(6 * H * W * b) + al(3 * H * W * b) + al(12 * H * W)
    l = L.lib()
    assert l.fldr_light_acc_bytes(0, 4) == L.E_ARG and l.fldr_light_acc_bytes(4, -1) == L.E_ARG
    assert l.fldr_light_scratch_bytes(4, 4, None) == L.E_ARG
    f = V.Format()
    f.depth = 12
    assert l.fldr_light_scratch_bytes(4, 4, ctypes.byref(f)) == V.E_FORMAT


# ---- argument errors without a device ---------------------------------------------------------------------------------------------------
def _host_frames(V, layout, depth, n, H=64, W=64):
    buf = np.zeros(H * W * 8 + 512, np.uint8)
    base = (buf.ctypes.data + 255) // 256 * 256
    b = 2 if depth == 10 else 1
    fr = (V.Frame * n)()
    for f in fr:
        for p, (r, c) in enumerate(V.plane_shapes(layout, H, W)):
            f.plane[p], f.pitch[p] = base, c * b
    return buf, base, fr


@pytest.mark.parametrize("layout", ["nv12", "i420"])
@pytest.mark.parametrize("depth", [8, 10])
def test_kernel_argument_errors_before_any_device_call(layout, depth):
    """accumulate, resolve and mix: every refusal tests/test_shutter_cpu.py tries, with host memory in place of device memory — nothing
    may touch it — and the new ones: a total above 255, a missing scratch, a null curve.  The curve is looked at last, so every other
    defect is reported without one; a call with a null curve and no other defect is the last refusal.  (A curve of the other depth needs
    a device to exist: tests/test_gpu_light.py.)"""
    import fldr_light as L
    import fldr_shutter as T
    import fldr_video as V
    l = L.lib()
    b = 2 if depth == 10 else 1
    shapes = V.plane_shapes(layout, 64, 64)
    buf, base, _ = _host_frames(V, layout, depth, 1)

    def run(which, damage=None, H=64, W=64, n=3, weights=(1, 2, 3), acc=base, total=6, fmt=True, frames=True, out=True, scratch=base):
        _, _, fr = _host_frames(V, layout, depth, max(n, 1))
        _, _, o = _host_frames(V, layout, depth, 1)
        f = V.Format(layout, depth=depth)
        if damage:
            damage(f, fr[max(n, 1) - 1], o[0])
        w = (ctypes.c_int32 * max(len(weights), 1))(*weights)
        fp = ctypes.byref(f) if fmt else None
        if which == "accumulate":
            rc = l.fldr_light_accumulate(H, W, fp, None, fr if frames else None, w, n, 1, acc, scratch, None)
        elif which == "resolve":
            rc = l.fldr_light_resolve(H, W, fp, None, acc, total, o if out else None, scratch, None)
        else:
            rc = l.fldr_light_mix(H, W, fp, None, fr if frames else None, w, n, o if out else None, scratch, None)
        assert rc != 0, "a test call without a defect"
        return rc
    for which in ("accumulate", "resolve", "mix"):
        assert run(which) == L.E_ARG                                                      # nothing wrong but the null curve
        assert run(which, H=0) == L.E_ARG and run(which, W=0) == L.E_ARG and run(which, H=-1) == L.E_ARG
        assert run(which, fmt=False) == L.E_ARG
        for field, val in (("layout", 2), ("matrix", 2), ("range", -1), ("depth", 9), ("depth", 12)):
            assert run(which, lambda f, fr, o: setattr(f, field, val)) == V.E_FORMAT, field
        assert run(which, lambda f, fr, o: f.reserved.__setitem__(4, 1)) == V.E_FORMAT
        side = (lambda fr, o: o) if which == "resolve" else (lambda fr, o: fr)           # the frame the call looks at first
        for q in range(len(shapes)):
            assert run(which, lambda f, fr, o: side(fr, o).plane.__setitem__(q, None)) == V.E_PLANE, q
            assert run(which, lambda f, fr, o: side(fr, o).pitch.__setitem__(q, shapes[q][1] * b - b)) == V.E_PITCH, q
            if depth == 10:
                assert run(which, lambda f, fr, o: side(fr, o).plane.__setitem__(q, base + 1)) == V.E_PLANE, q
                assert run(which, lambda f, fr, o: side(fr, o).pitch.__setitem__(q, shapes[q][1] * b + 1)) == V.E_PITCH, q
        for s in (None, base + 128, base + 16):
            assert run(which, scratch=s) == L.E_ACC, s
    for which in ("accumulate", "mix"):
        assert run(which, frames=False) == L.E_ARG and run(which, n=0) == L.E_ARG and run(which, n=-3) == L.E_ARG
        for bad in ((0, 1, 1), (1, 256, 1), (1, 1, -1)):
            assert run(which, weights=bad) == L.E_WEIGHT, bad
        assert run(which, weights=(100, 100, 56)) == L.E_WEIGHT                           # a total of 256
        assert run(which, weights=(100, 100, 55)) == L.E_ARG                              # 255 is allowed: on to the curve
    for which in ("resolve", "mix"):
        assert run(which, out=False) == L.E_ARG
    for q in range(len(shapes)):                                                          # the mix's output, behind valid sources
        assert run("mix", lambda f, fr, o: o.plane.__setitem__(q, None)) == V.E_PLANE
        assert run("mix", lambda f, fr, o: o.pitch.__setitem__(q, shapes[q][1] * b - b)) == V.E_PITCH
    assert run("mix", n=T.LAUNCH_FRAMES + 1, weights=(1,) * (T.LAUNCH_FRAMES + 1)) == L.E_ARG       # a mix takes what a forward can have
    for total in (0, -1, 256, 65535):
        assert run("resolve", total=total) == L.E_WEIGHT, total
    assert run("resolve", total=255) == L.E_ARG
    for which in ("accumulate", "resolve"):
        for acc in (None, base + 128, base + 16):
            assert run(which, acc=acc) == L.E_ACC, acc
    assert not buf.any()


def test_curve_create_argument_errors_before_any_device_call():
    import fldr_light as L
    l = L.lib()
    h = ctypes.c_void_p()
    ok = np.arange(256, dtype=np.uint32) * 65793                    # 255 * 65793 = S
    assert int(ok[-1]) == LO.S
    P = ctypes.POINTER(ctypes.c_uint32)

    def create(table, transfer=3, depth=8, device=0, out=True):
        rc = l.fldr_light_curve_create(transfer, depth, table.ctypes.data_as(P) if table is not None else None, device,
                                       ctypes.byref(h) if out else None)
        assert rc != 0 and (not out or h.value is None)             # without a device even a valid table ends at E_DEVICE
        return rc
    assert create(ok, out=False) == L.E_ARG
    assert create(ok, transfer=4) == L.E_ARG and create(ok, transfer=-1) == L.E_ARG
    assert create(ok, depth=9) == L.E_ARG and create(ok, device=-1) == L.E_ARG
    assert create(None) == L.E_ARG                                  # TABLE without a table
    flat = ok.copy(); flat[100] = flat[99]
    down = ok.copy(); down[7] = down[5]
    high = ok.copy(); high[255] = LO.S + 1
    for bad in (flat, down, high, np.zeros(256, np.uint32)):
        assert create(bad) == L.E_TABLE
    short = np.arange(1024, dtype=np.uint32)
    short[600] = short[599]
    assert create(short, depth=10) == L.E_TABLE
    l.fldr_light_curve_destroy(None)


def _io(V, H=64, W=64, layout="nv12", n_t=1):
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
    io.n_t, io.t, io.out = n_t, buf.ctypes.data, ctypes.cast(outs, ctypes.POINTER(V.Frame))
    io._keep = (buf, outs)
    return io


@pytest.mark.parametrize("layout", ["nv12", "i420"])
def test_forward_argument_errors_before_any_device_call(layout):
    import fldr_light as L
    import fldr_video as V
    l = L.lib()
    ones = (ctypes.c_int32 * 64)(*([1] * 64))

    def call(io, w0=1, w1=1, w=ones):
        return l.fldr_light_forward(None, ctypes.byref(io), None, w0, w1, w, None, 0, None)
    assert call(_io(V, layout=layout)) == L.E_ARG                           # valid io: the null curve
    assert l.fldr_light_forward(None, None, None, 1, 1, ones, None, 0, None) == L.E_ARG
    assert call(_io(V, layout=layout), w=None) == L.E_ARG
    cases = []
    for field, val in (("layout", 1 - V.LAYOUTS[layout]), ("matrix", 0), ("range", 1), ("depth", 10)):
        io = _io(V, layout=layout); setattr(io.out_format, field, val); cases.append((io, L.E_FORMAT))     # valid, but not the input's
    io = _io(V, layout=layout); io.in_format.depth = 0; cases.append((io, L.E_ARG))                         # 0 and 8 are one depth
    for field, val in (("layout", 2), ("matrix", 2), ("range", 2)):
        io = _io(V, layout=layout); setattr(io.in_format, field, val); setattr(io.out_format, field, val); cases.append((io, V.E_FORMAT))
    io = _io(V, layout=layout); io.in_[0].pitch[0] = 63; cases.append((io, V.E_PITCH))
    io = _io(V, layout=layout); io.out[0].pitch[1] = (32 if layout == "i420" else 64) - 1; cases.append((io, V.E_PITCH))
    io = _io(V, layout=layout); io.in_[1].plane[1] = None; cases.append((io, V.E_PLANE))
    io = _io(V, layout=layout); io.out[0].plane[0] = None; cases.append((io, V.E_PLANE))
    io = _io(V, layout=layout); io.n_t = 0; cases.append((io, V.E_ARG))
    io = _io(V, layout=layout); io.n_t = 65; cases.append((io, L.E_ARG))
    io = _io(V, layout=layout); io.t = None; cases.append((io, V.E_ARG))
    io = _io(V, layout=layout); io.W = 1; cases.append((io, V.E_ARG))
    for io, code in cases:
        assert call(io) == code
    assert call(_io(V, layout=layout), w0=-1) == L.E_WEIGHT and call(_io(V, layout=layout), w1=256) == L.E_WEIGHT
    assert call(_io(V, layout=layout, n_t=2), w=(ctypes.c_int32 * 2)(1, 0)) == L.E_WEIGHT
    assert call(_io(V, layout=layout), w0=200, w1=55) == L.E_WEIGHT         # 200 + 55 + 1: a total of 256
    assert call(_io(V, layout=layout), w0=200, w1=54) == L.E_ARG            # 255: on to the curve
    assert call(_io(V, layout=layout, n_t=64), w0=255, w1=0) == L.E_WEIGHT
    assert call(_io(V, layout=layout), w0=0, w1=0) == L.E_ARG               # allowed: the sub-frames alone
    assert l.fldr_light_workspace_bytes(None, 64, 64, 1) == V.E_ARG


def test_converter_argument_errors_before_any_device_call():
    """Every case tests/test_shutter_cpu.py tries on fldr_shutter_create, with this library's codes, and the window of more than 255
    points.  A null curve is the last refusal before the model."""
    import fldr_light as L
    import fldr_shutter as T
    import fldr_video as V
    l = L.lib()
    h = ctypes.c_void_p()

    def create(**kw):
        cfg = L.LightConfig()
        cfg.shutter = T.config(120, 24, (1, 2), 1, 64, 64, V.Format("i420"), 0, True)
        for k, v in kw.items():
            if k == "mutate":
                v(cfg.shutter)
            else:
                setattr(cfg.shutter, k, v)
        return l.fldr_light_create(None, ctypes.byref(cfg), ctypes.byref(h))
    assert create() == L.E_ARG                                               # valid, no curve (and no model)
    for term in ("in_num", "in_den", "out_num", "out_den", "shutter_num", "shutter_den"):
        assert create(**{term: 0}) == L.E_RATIO and create(**{term: -24}) == L.E_RATIO, term
    assert create(shutter_num=3, shutter_den=2) == L.E_RATIO
    assert create(shutter_num=2, shutter_den=2) == L.E_ARG
    assert create(in_num=24, out_num=60, sub=1) == L.E_RATIO and create(in_num=24, out_num=60, sub=4) == L.E_RATIO
    assert create(in_num=24, out_num=60, sub=5) == L.E_ARG
    assert create(in_num=60, out_num=24, shutter_num=1, shutter_den=4, sub=1) == L.E_RATIO
    assert create(in_num=60, out_num=24, shutter_num=1, shutter_den=4, sub=2) == L.E_ARG
    assert create(sub=0) == L.E_ARG and create(sub=65) == L.E_ARG and create(sub=64) == L.E_ARG      # 120 -> 24, s = 1/2, sub 64: 160 points
    assert create(in_num=1, out_num=63, shutter_num=1, shutter_den=1, sub=64) == L.E_ARG
    assert create(in_num=1, out_num=64, shutter_num=1, shutter_den=1, sub=64) == L.E_RATIO
    assert create(in_num=2 ** 25 + 1, out_num=2 ** 25) == L.E_RATIO
    assert create(shutter_num=2 ** 25 - 1, shutter_den=2 ** 25) == L.E_RATIO
    # windows of 255 and of 256 points: 255 / 1 and 256 / 1 input frames per output, the whole interval exposed
    assert create(in_num=255, out_num=1, shutter_num=1, shutter_den=1, sub=1) == L.E_ARG
    assert create(in_num=256, out_num=1, shutter_num=1, shutter_den=1, sub=1) == L.E_RATIO
    assert create(in_num=120, out_num=24, shutter_num=1, shutter_den=1, sub=51) == L.E_ARG           # 255
    assert create(in_num=120, out_num=24, shutter_num=1, shutter_den=1, sub=52) == L.E_RATIO         # 260: the shutter library takes it
    f, la = ctypes.c_int64(), ctypes.c_int64()
    assert T.lib().fldr_shutter_plan(ctypes.byref(T.config(120, 24, 1, 52)), 0, ctypes.byref(f), ctypes.byref(la)) == 0
    assert create(in_num=60000, in_den=1001, out_num=24000, out_den=1001) == L.E_ARG
    assert create(scene=2) == L.E_ARG and create(scene=-1) == L.E_ARG
    assert create(H=1) == L.E_ARG and create(device=-1) == L.E_ARG
    assert create(mutate=lambda c: c.reserved.__setitem__(2, 1)) == L.E_ARG
    assert create(mutate=lambda c: setattr(c.scene_params, "sad_permille", 1001)) == L.E_ARG
    assert create(mutate=lambda c: c.scene_params.reserved.__setitem__(0, 1)) == L.E_ARG
    assert create(mutate=lambda c: setattr(c.format, "layout", 3)) == V.E_FORMAT
    assert create(mutate=lambda c: setattr(c.format, "depth", 12)) == V.E_FORMAT
    assert l.fldr_light_create(None, None, ctypes.byref(h)) == L.E_ARG
    n = ctypes.c_int()
    assert l.fldr_light_push(None, None, None, None, ctypes.byref(n), None) == L.E_ARG
    assert l.fldr_light_flush(None, None, None, ctypes.byref(n)) == L.E_ARG
    assert l.fldr_light_reset(None) == L.E_ARG
    assert l.fldr_light_max_out(None) == L.E_ARG
    l.fldr_light_destroy(None)
