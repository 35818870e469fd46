"""CPU checks of the packed 10-bit API (include/fldr_pack10.h, libfldr_pack10.so): the library's symbol table and link, the header as
plain C99 / C++, the C example, the binding's struct mirrors, the argument checks (decided before any device call, so they run without a
GPU), the listing of the kernels, and the container statement of tests/yuv_pack10_oracle.py: the header's worked v210 example as literal
words, a walking field, pack / unpack as inverses, dirt, and the spare-slot rule."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import yuv_pack10_oracle as P
from lib_checks import declared as _declared, disassemble as _disassemble, syms as _syms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fldr-vfi_amd")
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "fldr_pack10.h")
LIB = os.path.join(PKG, "libfldr_pack10.so")
EXAMPLE_C = os.path.join(ROOT, "examples", "fldr_slowmo_sdi.c")


# ---- the library ----------------------------------------------------------------------------------------------------------------
def test_library_exports_exactly_the_header():
    declared = _declared(HDR, "FLDR_PACK10_API")
    assert len(declared) == 11, sorted(declared)
    assert _syms(LIB, ["--defined-only"]) == declared
    import fldr_pack10
    assert set(fldr_pack10.EXPORTS) == declared and len(fldr_pack10.EXPORTS) == 11


def test_library_links_only_the_model_api():
    dyn = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    needed = re.findall(r"NEEDED.*\[(libfldr_[a-z0-9_]+\.so)\]", dyn)
    assert needed == ["libfldr_model.so"], dyn
    assert re.search(r"R(UN)?PATH.*\$ORIGIN", dyn), dyn
    used = set(n for n in _syms(LIB, ["--undefined-only"]) if n.startswith("fldr_"))
    assert used and used <= _declared(os.path.join(INC, "fldr_model.h"), "FLDR_MODEL_API"), sorted(used)
    assert "fldr_model_forward" in used


@pytest.mark.parametrize("compiler", [["gcc", "-std=c99", "-x", "c"], ["g++", "-std=c++11", "-x", "c++"]])
def test_header_is_plain_c99_and_cxx(compiler, tmp_path):
    assert shutil.which(compiler[0]), compiler[0] + " not installed"
    src = tmp_path / "h.c"
    src.write_text('#include "fldr_pack10.h"\nint main(void) { return fldr_pack10_sizeof(0) > 0 && sizeof(fldr_pack10_format) == 32 ? 0 : 1; }\n')
    r = subprocess.run(compiler + ["-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I" + INC, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "hip" not in re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S).lower()


def test_binding_struct_sizes_version_and_codes():
    import fldr_pack10 as V
    l = V.lib()
    assert l.fldr_pack10_version() == V.PACK10_VERSION
    text = open(HDR).read()
    assert int(re.search(r"#define FLDR_PACK10_VERSION (\d+)", text).group(1)) == V.PACK10_VERSION
    for which, cls in enumerate((V.Format, V.Frame, V.IO, V.SessionConfig)):
        assert l.fldr_pack10_sizeof(which) == ctypes.sizeof(cls)
    assert ctypes.sizeof(V.Format) == 32 and ctypes.sizeof(V.Frame) == 48
    import fldr_chroma
    assert ctypes.sizeof(V.IO) == ctypes.sizeof(fldr_chroma.IO) and ctypes.sizeof(V.SessionConfig) == ctypes.sizeof(fldr_chroma.SessionConfig)
    assert l.fldr_pack10_sizeof(4) == V.E_ARG
    for name, v in (("E_ARG", V.E_ARG), ("E_FORMAT", V.E_FORMAT), ("E_PITCH", V.E_PITCH), ("E_PLANE", V.E_PLANE),
                    ("E_WORKSPACE", V.E_WORKSPACE), ("E_DEVICE", V.E_DEVICE)):
        assert re.search(r"#define FLDR_PACK10_%s\s+\((-?\d+)\)" % name, text).group(1) == str(v)
        assert v <= -800                                                       # below every other library's range
        assert l.fldr_pack10_error_string(v).decode().startswith("fldr_pack10")
    assert l.fldr_pack10_error_string(-3).decode().startswith("fldr_model")   # model codes pass through
    for table in (V.CONTAINERS, V.MATRICES, V.RANGES):
        for name, v in table.items():
            assert re.search(r"FLDR_PACK10_%s = %d\b" % (name.upper(), v), text), name
    assert tuple(V.CONTAINERS) == P.CONTAINERS
    body = open(os.path.join(PKG, "pack10", "pack10_internal.h")).read()
    assert int(re.search(r"RUN_V210 = (\d+)", body).group(1)) == V.RUN["v210"]
    assert int(re.search(r"RUN_WORDS = (\d+)", body).group(1)) == V.RUN["y210"] == V.RUN["y410"]
    for c in P.CONTAINERS:                                                     # the binding's geometry is the oracle's
        for W in range(1, 50):
            assert V.plane_shapes(V.Format(c), 3, W) == [(3, P.row_words(c, W))]
    assert V.v210_pitch(1920) == 5120 == P.v210_pitch(1920) and V.v210_pitch(1) == 128


def test_example_builds_with_cc_prints_usage_and_rejects_bad_arguments(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    exe = tmp_path / "fldr_slowmo_sdi"
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + INC, "-o", str(exe), EXAMPLE_C, "-L" + PKG,
                        "-l:libfldr_pack10.so", "-l:libfldr_model.so", "-Wl,-rpath," + PKG], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "hip" not in re.sub(r"/\*.*?\*/", "", open(EXAMPLE_C).read(), flags=re.S).lower()
    u = subprocess.run([str(exe)], capture_output=True, text=True)            # no arguments: usage, no device touched
    assert u.returncode == 2 and "usage" in u.stderr
    for bad in (["w.npz", "64", "64"], ["w.npz", "64", "64", "1"], ["w.npz", "1", "64", "2"], ["w.npz", "64", "64", "2", "yuv422p10le"],
                ["w.npz", "64", "64", "2", "bt709", "y210"], ["w.npz", "64", "64", "2", "v210", "bt2020"],
                ["w.npz", "64", "64", "2", "y410", "bt601", "full", "more"]):
        u = subprocess.run([str(exe)] + bad, capture_output=True, text=True)
        assert u.returncode == 2 and "usage" in u.stderr, bad


# ---- argument errors without a device ---------------------------------------------------------------------------------------------
def _io(V, fmt=None, H=64, W=64):
    fmt = fmt or V.Format()
    buf = np.zeros(H * W * 8 + 64, np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    io = V.IO()
    io.H, io.W = H, W
    io.in_format, io.out_format = fmt.copy(), fmt.copy()
    pitch = V.plane_shapes(fmt, H, W)[0][1] * np.dtype(V.plane_dtype(fmt, numpy=True)).itemsize
    for f in range(2):
        io.in_[f].plane[0], io.in_[f].pitch[0] = base, pitch
    outs = (V.Frame * 1)()
    outs[0].plane[0], outs[0].pitch[0] = base, pitch
    io.n_t, io.t, io.out = 1, base, ctypes.cast(outs, ctypes.POINTER(V.Frame))
    io._keep = (buf, outs)
    return io


def _all_formats(V):
    return [V.Format(c) for c in P.containers()]


def test_every_container_is_accepted_and_every_bad_field_is_a_format_error():
    import fldr_pack10 as V
    l = V.lib()
    call = lambda io: l.fldr_pack10_forward(None, ctypes.byref(io), None, 0, None)
    assert len(_all_formats(V)) == 3
    for fmt in _all_formats(V):
        assert call(_io(V, fmt)) == V.E_ARG                                   # valid io, no model
        for side in ("in_format", "out_format"):
            for field, val in (("container", 3), ("container", -1), ("matrix", 2), ("matrix", -1), ("range", 2), ("depth", 8), ("depth", 0),
                               ("depth", 12), ("depth", 16)):
                io = _io(V, fmt); setattr(getattr(io, side), field, val)
                assert call(io) == V.E_FORMAT, (side, field, val)
            for w in range(4):
                io = _io(V, fmt); getattr(io, side).reserved[w] = 1
                assert call(io) == V.E_FORMAT
        for other in _all_formats(V):                                          # the two sides are independent
            io = _io(V, fmt); io.out_format = other
            io.out[0].pitch[0] = _io(V, other).out[0].pitch[0]
            assert call(io) == V.E_ARG, (fmt.name, other.name)
    # the converters refuse the same formats, before looking at anything else they would touch
    fr, bad = V.Frame(), V.Format("v210", depth=8)
    buf = np.zeros(256, np.uint8)
    fr.plane[0], fr.pitch[0] = buf.ctypes.data, 64
    assert l.fldr_pack10_to_planar(ctypes.byref(fr), 1, ctypes.byref(bad), ctypes.c_void_p(buf.ctypes.data), 4, 4, None) == V.E_FORMAT
    assert l.fldr_pack10_from_planar(ctypes.c_void_p(buf.ctypes.data), ctypes.byref(bad), ctypes.byref(fr), 4, 4, None) == V.E_FORMAT


def test_pitch_plane_and_argument_errors_before_any_device_call():
    import fldr_pack10 as V
    l = V.lib()
    call = lambda io: l.fldr_pack10_forward(None, ctypes.byref(io), None, 0, None)
    W = 63                                                                     # v210: 11 groups = 176 bytes; Y210: 32 groups = 256; Y410: 252
    rows = {"v210": 16 * ((W + 5) // 6), "y210": 8 * ((W + 1) // 2), "y410": 4 * W}
    assert rows == {"v210": 176, "y210": 256, "y410": 252}
    for fmt in _all_formats(V):
        rb, unit = rows[fmt.name], (2 if fmt.name == "y210" else 4)
        assert _io(V, fmt, W=W).in_[0].pitch[0] == rb
        assert call(_io(V, fmt, W=W)) == V.E_ARG
        io = _io(V, fmt, W=W); io.in_[1].pitch[0] = rb - 4                    # shorter than the row (v210: 16 ceil(W/6) - 4)
        assert call(io) == V.E_PITCH
        io = _io(V, fmt, W=W); io.out[0].pitch[0] = rb - unit
        assert call(io) == V.E_PITCH
        io = _io(V, fmt, W=W); io.in_[0].pitch[0] = rb + 2                    # long enough, but not a multiple of 4
        assert call(io) == (V.E_ARG if unit == 2 else V.E_PITCH)
        io = _io(V, fmt, W=W); io.out[0].pitch[0] = rb + 2
        assert call(io) == (V.E_ARG if unit == 2 else V.E_PITCH)
        io = _io(V, fmt, W=W); io.in_[0].pitch[0] = rb + 3                    # odd: never
        assert call(io) == V.E_PITCH
        io = _io(V, fmt, W=W); io.in_[0].pitch[0] = rb + 4
        assert call(io) == V.E_ARG
        io = _io(V, fmt, W=W); io.in_[0].plane[0] = None
        assert call(io) == V.E_PLANE
        io = _io(V, fmt, W=W); io.out[0].plane[0] = None
        assert call(io) == V.E_PLANE
        for side in ("in", "out"):
            for off, want in ((1, V.E_PLANE), (2, V.E_ARG if unit == 2 else V.E_PLANE), (4, V.E_ARG)):
                io = _io(V, fmt, W=W)
                fr = io.in_[1] if side == "in" else io.out[0]
                fr.plane[0] = fr.plane[0] + off
                assert call(io) == want, (fmt.name, side, off)
        # two faults at once: the plane and then the pitch by the 16-bit word, then the plane and then the pitch by the unit of 4
        for side in ("in", "out"):
            def two(off, pitch):
                io = _io(V, fmt, W=W)
                fr = io.in_[1] if side == "in" else io.out[0]
                fr.plane[0] = fr.plane[0] + off if off is not None else None
                fr.pitch[0] = pitch
                return call(io)
            assert two(2, rb - 4) == V.E_PITCH, (fmt.name, side)              # an address = 2 mod 4 and a short pitch: the pitch
            assert two(2, rb - 2) == V.E_PITCH, (fmt.name, side)
            assert two(1, rb - 4) == V.E_PLANE, (fmt.name, side)              # an odd address comes before any pitch
            assert two(2, rb + 2) == (V.E_ARG if unit == 2 else V.E_PLANE), (fmt.name, side)   # both = 2 mod 4, the pitch covers the row
            assert two(4, rb + 2) == (V.E_ARG if unit == 2 else V.E_PITCH), (fmt.name, side)
            assert two(None, rb - 4) == V.E_PLANE, (fmt.name, side)           # a null plane and a bad pitch: the plane
            assert two(None, rb + 2) == V.E_PLANE, (fmt.name, side)
            assert two(None, rb + 3) == V.E_PLANE, (fmt.name, side)
        io = _io(V, fmt, W=W); io.in_[0].plane[1] = None; io.in_[0].plane[2] = None; io.in_[0].pitch[1] = io.in_[0].pitch[2] = 0
        assert call(io) == V.E_ARG                                             # only plane 0 is looked at
        io = _io(V, fmt); io.n_t = 0
        assert call(io) == V.E_ARG
        io = _io(V, fmt); io.t = None
        assert call(io) == V.E_ARG
        io = _io(V, fmt); io.W = 1
        assert call(io) == V.E_ARG
    assert l.fldr_pack10_forward(None, None, None, 0, None) == V.E_ARG
    assert l.fldr_pack10_workspace_bytes(None, 64, 64, 1) == V.E_ARG
    # the converters alone
    fmt = V.Format("v210")
    buf = np.zeros(4096 + 64, np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    fr = V.Frame()
    fr.plane[0], fr.pitch[0] = base, 32
    to = lambda fr_, planar, H=4, W=8, n=1: l.fldr_pack10_to_planar(ctypes.byref(fr_), n, ctypes.byref(fmt), planar, H, W, None)
    frm = lambda fr_, planar, H=4, W=8: l.fldr_pack10_from_planar(planar, ctypes.byref(fmt), ctypes.byref(fr_), H, W, None)
    ok = ctypes.c_void_p(base)
    assert to(fr, None) == V.E_ARG and frm(fr, None) == V.E_ARG
    assert to(fr, ok, H=0) == V.E_ARG and frm(fr, ok, W=0) == V.E_ARG and to(fr, ok, n=0) == V.E_ARG
    assert to(fr, ctypes.c_void_p(base + 1)) == V.E_ARG and frm(fr, ctypes.c_void_p(base + 1)) == V.E_ARG   # uint16 planar frames at an odd address
    fr.pitch[0] = 28                                                           # W = 8: two groups
    assert to(fr, ok) == V.E_PITCH and frm(fr, ok) == V.E_PITCH
    fr.pitch[0] = 34
    assert to(fr, ok) == V.E_PITCH and frm(fr, ok) == V.E_PITCH
    fr.pitch[0] = 32; fr.plane[0] = base + 2
    assert to(fr, ok) == V.E_PLANE and frm(fr, ok) == V.E_PLANE


def test_workspace_and_session_argument_errors_before_any_device_call():
    import fldr_pack10 as V
    l = V.lib()
    h = ctypes.c_void_p()
    cfg = V.SessionConfig()
    cfg.H, cfg.W, cfg.n_t = 64, 64, 1
    cfg.in_format, cfg.out_format = V.Format("v210"), V.Format("y410", "bt601", "full")
    create = lambda: l.fldr_pack10_session_create(None, ctypes.byref(cfg), ctypes.byref(h))
    assert create() == V.E_ARG
    cfg.reserved[1] = 1
    assert create() == V.E_FORMAT
    cfg.reserved[1] = 0
    cfg.out_format.depth = 8
    assert create() == V.E_FORMAT
    cfg.out_format.depth = 10
    cfg.in_format.container = 3
    assert create() == V.E_FORMAT
    cfg.in_format.container = 0
    cfg.n_t = 0
    assert create() == V.E_ARG
    assert l.fldr_pack10_session_create(None, None, ctypes.byref(h)) == V.E_ARG
    assert l.fldr_pack10_session_push(None, None, None, None) == V.E_ARG and l.fldr_pack10_session_reset(None) == V.E_ARG
    l.fldr_pack10_session_destroy(None)
    assert l.fldr_pack10_workspace_bytes(None, 64, 64, 1) == V.E_ARG
    assert l.fldr_pack10_error_string(V.E_WORKSPACE).decode().startswith("fldr_pack10: workspace")


# ---- the listing ----------------------------------------------------------------------------------------------------------------
def test_kernels_use_no_scratch_no_lds_and_leave_four_waves_per_simd():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    ks = KR.kernels(LIB)
    names = [k["name"] for k in ks]
    # one input and one output kernel, each for three containers in two forms
    for stem in ("pack10_to_planar_kernel", "pack10_from_planar_kernel"):
        assert sum(stem in n for n in names) == 6, names
    assert len(ks) == 12
    for k in ks:
        assert k["scratch"] == 0 and k["vgpr_spills"] == 0 and k["sgpr_spills"] == 0 and k["lds"] == 0, k
        assert k["vgpr"] + k["agpr"] <= 128, k                                 # 512 / 128: four waves per SIMD


def test_listing_has_the_wide_accesses_and_no_stale_half_packing():
    """v_ashr_pk_* / v_cvt_pk_[ui]16_* leave upper bits stale on gfx950 (video/yuv_run_device.h): none may be in the library; the wide
    forms show as 16-byte loads and stores."""
    texts = _disassemble(LIB)
    assert texts and any("pack10_to_planar_kernel" in t and "pack10_from_planar_kernel" in t for t in texts)
    n = sum(len(re.findall(r"\bv_ashr_pk_\w+|\bv_cvt_pk_[ui]16_\w+", t)) for t in texts)
    assert n == 0
    for ins in ("global_load_dwordx4", "global_store_dwordx4"):
        assert any(ins in t for t in texts), ins


def test_no_unsafe_packed_fp32_in_the_library():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_pk_opsel.py"), LIB], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


# ---- the containers ---------------------------------------------------------------------------------------------------------------
# include/fldr_pack10.h's layout, by hand: U = 001 002 003, Y = 010 020 030 040 050 060, V = 100 200 300 (hex)
EX_Y, EX_U, EX_V = [0x010, 0x020, 0x030, 0x040, 0x050, 0x060], [0x001, 0x002, 0x003], [0x100, 0x200, 0x300]
EX_WORDS = [0x10004001, 0x03000820, 0x00310200, 0x060C0050]


def test_the_worked_v210_example_in_both_directions():
    Y, U, V = (np.array([a], np.uint16) for a in (EX_Y, EX_U, EX_V))
    words = P.pack(Y, U, V, "v210")[0]
    assert words.dtype == np.uint32 and words.tolist() == [EX_WORDS]
    for got, want in zip(P.unpack((np.array([EX_WORDS], np.uint32),), "v210", 6), (EX_Y, EX_U, EX_V)):
        assert got.tolist() == [want]
    assert words.tobytes()[:4] == bytes([0x01, 0x40, 0x00, 0x10])              # little-endian


def test_a_walking_field_lands_on_one_sample_of_the_right_plane_and_column():
    """Each of the 12 sample fields of a group set to 0x3ff alone: word w, field b holds what the header's table says.  The pad bits and
    the Y410 alpha bits decode to nothing."""
    table = {(0, 0): ("U", 0), (0, 1): ("Y", 0), (0, 2): ("V", 0), (1, 0): ("Y", 1), (1, 1): ("U", 1), (1, 2): ("Y", 2),
             (2, 0): ("V", 1), (2, 1): ("Y", 3), (2, 2): ("U", 2), (3, 0): ("Y", 4), (3, 1): ("V", 2), (3, 2): ("Y", 5)}
    seen = set()
    for group in (0, 1):                                                       # the second group: columns 6 .. 11, chroma 3 .. 5
        for (w, b), (plane, slot) in table.items():
            words = np.zeros((1, 8), np.uint32)
            words[0, 4 * group + w] = 0x3ff << (10 * b)
            Y, U, V = P.unpack((words,), "v210", 12)
            got = {"Y": Y, "U": U, "V": V}
            col = (6 if plane == "Y" else 3) * group + slot
            for name, arr in got.items():
                want = np.zeros_like(arr)
                if name == plane:
                    want[0, col] = 0x3ff
                assert np.array_equal(arr, want), (group, w, b, name)
            seen.add((plane, col))
    assert len(seen) == 24
    for w in range(4):                                                         # the 8 pad bits of a group
        for bit in (30, 31):
            words = np.zeros((1, 4), np.uint32)
            words[0, w] = 1 << bit
            assert not any(a.any() for a in P.unpack((words,), "v210", 6))
    for shift, plane in ((0, 1), (10, 0), (20, 2)):                            # Y410: U, Y, V; alpha is nothing
        got = P.unpack((np.array([[0x3ff << shift]], np.uint32),), "y410", 1)
        assert [int(a[0, 0]) for a in got] == [0x3ff if p == plane else 0 for p in range(3)]
    assert not any(a.any() for a in P.unpack((np.array([[0xc0000000]], np.uint32),), "y410", 1))
    got = P.unpack((np.array([[0xffc0, 0x003f, 0x0040, 0x8000]], np.uint16),), "y210", 2)      # Y0 U Y1 V, value high, low six bits nothing
    assert [a.tolist() for a in got] == [[[0x3ff, 1]], [[0]], [[0x200]]]


WIDTHS = list(range(1, 14)) + [47, 48, 49]


@pytest.mark.parametrize("c", P.CONTAINERS)
def test_pack_and_unpack_are_inverse_and_dirt_stays_out_of_the_values(c):
    g = np.random.default_rng(3)
    for W in WIDTHS:
        for H in (1, 3):
            cw = P.chroma_width(P.SAMPLING[c], W)
            Y, U, V = (g.integers(0, 1024, sh).astype(np.uint16) for sh in ((H, W), (H, cw), (H, cw)))
            clean, dirty = P.pack(Y, U, V, c), P.pack(Y, U, V, c, dirt=g)
            assert clean[0].shape == (H, P.row_words(c, W)) and clean[0].dtype == (np.uint16 if c == "y210" else np.uint32)
            assert not np.array_equal(clean[0], dirty[0])
            for planes in (clean, dirty):
                for a, b in zip(P.unpack(planes, c, W), (Y, U, V)):
                    assert a.dtype == np.uint16 and np.array_equal(a, b), (c, W)
            again = P.pack(*P.unpack(dirty, c, W), c)                          # a writer's frame of a reader's values: the clean one
            assert np.array_equal(again[0], clean[0])
    # every code value passes through
    ramp = np.arange(1024, dtype=np.uint16)[None, :]
    cr = np.ascontiguousarray(ramp[:, ::-1][:, :P.chroma_width(P.SAMPLING[c], 1024)])
    for a, b in zip(P.unpack(P.pack(ramp, cr, cr, c), c, 1024), (ramp, cr, cr)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("W", range(1, 14))
def test_the_spare_slot_rule_at_every_width(W):
    """A written v210 row is whole groups: spare luma slots repeat luma W - 1, spare chroma slots chroma sample ceil(W/2) - 1, pad bits are
    zero; a written odd-width Y210 row ends with a copy of its last luma word; Y410 alpha is 3."""
    g = np.random.default_rng(W)
    cw = (W + 1) // 2
    Y, U, V = (g.integers(0, 1024, sh).astype(np.uint16) for sh in ((2, W), (2, cw), (2, cw)))
    words = P.pack(Y, U, V, "v210")[0]
    ng = (W + 5) // 6
    assert words.shape == (2, 4 * ng) and not (words >> 30).any()
    Ye, Ue, Ve = P.unpack((words,), "v210", 6 * ng)                           # read as a full-width row: the spare slots as samples
    assert Ye.shape == (2, 6 * ng) and Ue.shape == (2, 3 * ng)
    assert np.array_equal(Ye[:, :W], Y) and (Ye[:, W:] == Y[:, W - 1:W]).all()
    assert np.array_equal(Ue[:, :cw], U) and (Ue[:, cw:] == U[:, cw - 1:cw]).all()
    assert np.array_equal(Ve[:, :cw], V) and (Ve[:, cw:] == V[:, cw - 1:cw]).all()
    y210 = P.pack(Y, U, V, "y210")[0]
    assert not (y210 & 0x3f).any()
    if W % 2:
        assert np.array_equal(y210[:, -2] >> 6, Y[:, -1]) and np.array_equal(y210[:, -4] >> 6, Y[:, -1])
    y410 = P.pack(Y, np.repeat(U, 2, axis=1)[:, :W], np.repeat(V, 2, axis=1)[:, :W], "y410")[0]
    assert ((y410 >> 30) == 3).all()
