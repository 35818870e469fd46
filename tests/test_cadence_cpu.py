"""CPU checks of the cadence API (include/fldr_cadence.h, libfldr_cadence.so): the library's symbol table and link, the header as plain
C99 / C++, the C example, the code-generation guards, the binding's struct mirrors, the argument checks of both layers — which happen
before any device call, so they run without a GPU —, the derived inner rate, the oracle (tests/cadence_oracle.py) alone on hand-worked
frames and key sequences, and the condition tests/test_gpu_cadence.py puts on its input streams."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import cadence_frames as CF
import cadence_oracle as C
from lib_checks import declared as _declared, disassemble as _disassemble, syms as _syms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fldr-vfi_amd")
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "fldr_cadence.h")
LIB = os.path.join(PKG, "libfldr_cadence.so")
EXAMPLE = os.path.join(ROOT, "examples", "fldr_film.c")


# ---- the library ------------------------------------------------------------------------------------------------------------------------
def test_library_exports_exactly_the_header():
    declared = _declared(HDR, "FLDR_CADENCE_API")
    assert len(declared) == 11, sorted(declared)
    assert _syms(LIB, ["--defined-only"]) == declared
    import fldr_cadence
    assert set(fldr_cadence.EXPORTS) == declared
    for name in ("version", "error_string", "sizeof", "create", "destroy", "max_out", "push", "flush", "reset", "inner_rate"):
        assert "fldr_cadence_" + name in declared, name
    assert "fldr_repeat_measure" in declared


def test_library_links_only_the_rate_video_and_model_apis():
    dyn = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    assert re.search(r"NEEDED.*\[libfldr_rate\.so\]", dyn) and re.search(r"NEEDED.*\[libfldr_video\.so\]", dyn), dyn
    for other in ("hip", "shutter", "light", "pipe"):
        assert not re.search(r"NEEDED.*\[libfldr_%s\.so\]" % other, dyn), dyn
    assert re.search(r"R(UN)?PATH.*\$ORIGIN", dyn), dyn
    used = set(n for n in _syms(LIB, ["--undefined-only"]) if n.startswith("fldr_"))
    allowed = (_declared(os.path.join(INC, "fldr_rate.h"), "FLDR_RATE_API") | _declared(os.path.join(INC, "fldr_video.h"), "FLDR_VIDEO_API") |
               _declared(os.path.join(INC, "fldr_model.h"), "FLDR_MODEL_API"))
    assert used and used <= allowed, sorted(used)
    assert {"fldr_rate_create", "fldr_rate_push", "fldr_rate_flush", "fldr_rate_reset", "fldr_rate_destroy"} <= used


def test_the_libraries_below_know_nothing_of_the_cadence_api():
    for name in os.listdir(INC):
        if name != "fldr_cadence.h":
            text = open(os.path.join(INC, name)).read().lower()
            assert "fldr_cadence" not in text and "fldr_repeat" not in text, name
    for name in ("libfldr_hip.so", "libfldr_model.so", "libfldr_video.so", "libfldr_rate.so", "libfldr_shutter.so", "libfldr_light.so",
                 "libfldr_pipe.so"):
        assert not [n for n in _syms(os.path.join(PKG, name), []) if "fldr_cadence" in n or "fldr_repeat" in n], name


@pytest.mark.parametrize("compiler", [["gcc", "-std=c99", "-x", "c"], ["g++", "-std=c++11", "-x", "c++"]])
def test_header_is_plain_c99_and_cxx(compiler, tmp_path):
    if not shutil.which(compiler[0]):
        pytest.skip(compiler[0] + " not installed")
    src = tmp_path / "h.c"
    src.write_text('#include "fldr_cadence.h"\nint main(void) { fldr_cadence_config c; fldr_cadence_report r; c.cycle = FLDR_CADENCE_MAX_CYCLE;\n'
                   '  r.n_frames = 0;\n'
                   '  return fldr_cadence_sizeof(2) == (int)sizeof(c) && c.cycle == 16 && r.n_frames == 0 && FLDR_CADENCE_E_ARG == -600 &&\n'
                   '         FLDR_REPEAT_STATE_BYTES == 4096 && sizeof(fldr_repeat_result) == 32 ? 0 : 1; }\n')
    r = subprocess.run(compiler + ["-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I" + INC, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "hip/" not in open(HDR).read()


def test_header_says_where_the_default_comes_from():
    text = open(HDR).read()
    assert "synthetic content only" in text and "not on footage" in text
    assert C.default() == 2048 == 2 * 32 * 32                               # a mean difference of two codes over a full tile


def test_example_builds_with_cc(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if not cc:
        pytest.skip("no C compiler")
    exe = tmp_path / "fldr_film"
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + INC, "-o", str(exe), EXAMPLE, "-L" + PKG,
                        "-l:libfldr_cadence.so", "-l:libfldr_rate.so", "-l:libfldr_video.so", "-l:libfldr_model.so", "-Wl,-rpath," + PKG],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    src = open(EXAMPLE).read()
    assert "hip" not in re.sub(r"/\*.*?\*/", "", src, flags=re.S).lower()
    u = subprocess.run([str(exe)], capture_output=True, text=True)            # no arguments: usage, no device touched
    assert u.returncode == 2 and "usage" in u.stderr and "cycle=" in u.stderr
    for bad in (["w.npz", "64", "64", "60", "120", "cycle=5"],                # no drop=
                ["w.npz", "64", "64", "60", "120", "cycle=5", "drop=5"],      # drop not below cycle
                ["w.npz", "64", "64", "60", "120", "cycle=17", "drop=1"],
                ["w.npz", "64", "64", "60/0", "120", "cycle=5", "drop=3"]):
        u = subprocess.run([str(exe)] + bad, capture_output=True, text=True)
        assert u.returncode == 2 and "usage" in u.stderr, bad


def test_no_unsafe_packed_fp32_in_the_cadence_library():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_pk_opsel.py"), LIB], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_kernels_use_the_sad_instructions_integer_atomics_and_no_float():
    txt = "\n".join(_disassemble(LIB))
    assert "repeat_tiles_kernel" in txt and "repeat_result_kernel" in txt and "repeat_zero_kernel" in txt
    assert len(re.findall(r"\bv_ashr_pk_[ui]8_i32\b", txt)) == 0
    assert re.search(r"\bv_sad_u8\b", txt) and re.search(r"\bv_sad_u16\b", txt)
    assert re.search(r"\bglobal_atomic_umax_x2\b", txt) and re.search(r"\bglobal_atomic_add_x2\b", txt)   # the 64-bit key and sum
    assert re.search(r"\bglobal_load_dwordx4\b", txt)                         # 16 bytes per lane
    # no float anywhere: no conversion, no float arithmetic (an integer division would bring v_cvt_f32_u32 and v_rcp with it)
    assert not re.search(r"\bv_(cvt_f|rcp|add_f|mul_f|fma_f|mac_f|pk_\w+_f)", txt)


def test_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    ks = KR.kernels(LIB)
    assert len(ks) == 8, [k["name"] for k in ks]          # zero, result, tiles x (3 sample forms x wide / per-sample)
    for k in ks:
        assert k.get("scratch", -1) == 0 and k.get("vgpr_spills", -1) == 0 and k.get("sgpr_spills", -1) == 0, k


def test_binding_struct_sizes_and_version():
    import fldr_cadence as K
    l = K.lib()
    text = open(HDR).read()
    assert l.fldr_cadence_version() == K.CADENCE_VERSION == int(re.search(r"#define FLDR_CADENCE_VERSION (\d+)", text).group(1)) == 100
    for which, cls in enumerate((K.RepeatParams, K.RepeatResult, K.CadenceConfig, K.Report)):
        assert l.fldr_cadence_sizeof(which) == ctypes.sizeof(cls)
    assert ctypes.sizeof(K.RepeatResult) == 32 and ctypes.sizeof(K.RepeatParams) == 16
    assert ctypes.sizeof(K.Report) == 32 + 16 * 32
    assert l.fldr_cadence_sizeof(4) == K.E_ARG
    for name, v in (("E_ARG", K.E_ARG), ("E_STATE", K.E_STATE), ("E_DEVICE", K.E_DEVICE)):
        assert re.search(r"#define FLDR_CADENCE_%s\s+\((-?\d+)\)" % name, text).group(1) == str(v)
        assert v <= -600
        assert l.fldr_cadence_error_string(v).decode().startswith("fldr_cadence")
    for macro, v in (("FLDR_REPEAT_STATE_BYTES", K.REPEAT_STATE_BYTES), ("FLDR_CADENCE_MAX_CYCLE", K.MAX_CYCLE), ("FLDR_REPEAT_TILE", K.TILE),
                     ("FLDR_REPEAT_TILE_SAD_MAX", K.TILE_SAD_MAX), ("FLDR_REPEAT_TILE_SAD_DEFAULT", K.TILE_SAD_DEFAULT)):
        assert int(re.search(r"#define %s\s+(\d+)" % macro, text).group(1)) == v, macro
    assert K.TILE_SAD_MAX == 32 * 32 * 255 and K.MAX_CYCLE == 16
    assert l.fldr_cadence_error_string(-203).decode().startswith("fldr_rate")     # rate codes pass through,
    assert l.fldr_cadence_error_string(-101).decode().startswith("fldr_video")    # video codes through it,
    assert l.fldr_cadence_error_string(-3).decode().startswith("fldr_model")      # and model codes through that


# ---- argument errors without a device ---------------------------------------------------------------------------------------------------
def _frames(V, layout, depth, H=64, W=64):
    buf = np.zeros(H * W * 8 + 512, np.uint8)
    base = (buf.ctypes.data + 255) // 256 * 256
    b = 2 if depth == 10 else 1
    fr = []
    for _ in range(2):
        f = V.Frame()
        for p, (r, c) in enumerate(V.plane_shapes(layout, H, W)):
            f.plane[p], f.pitch[p] = base, c * b
        fr.append(f)
    return buf, base, fr


@pytest.mark.parametrize("layout", ["nv12", "i420"])
@pytest.mark.parametrize("depth", [8, 10])
def test_measure_argument_errors_before_any_device_call(layout, depth):
    import fldr_cadence as K
    import fldr_video as V
    H = W = 64
    b = 2 if depth == 10 else 1
    buf, base, _ = _frames(V, layout, depth)
    shapes = V.plane_shapes(layout, H, W)

    def call(mutate=lambda fr, fmt: None, params=None, state=base, H=H, W=W):
        _, _, fr = _frames(V, layout, depth)
        for f in fr:
            for p in range(len(shapes)):
                f.plane[p] = base
        fmt = V.Format(layout, depth=depth)
        mutate(fr[1], fmt)
        return K.repeat_measure_raw(H, W, fmt, fr, params, state, None)
    assert call(state=None) == K.E_STATE
    assert call(state=base + 128) == K.E_STATE and call(state=base + 16) == K.E_STATE
    assert call(H=0) == K.E_ARG and call(W=0) == K.E_ARG and call(H=-1) == K.E_ARG
    assert call(H=1, W=2 ** 31 - 1) == K.E_ARG and call(H=2 ** 31 - 1, W=1) == K.E_ARG     # rounding up to whole tiles would leave 32 bits
    assert K.repeat_measure_raw(H, W, None, _frames(V, layout, depth)[2], None, base, None) == K.E_ARG
    assert K.repeat_measure_raw(H, W, V.Format(layout, depth=depth), None, None, base, None) == K.E_ARG
    for bad in (-1, 261121, 2 ** 31 - 1):
        assert call(params=K.RepeatParams(bad)) == K.E_ARG, bad
    for q in range(3):
        p = K.RepeatParams()
        p.reserved[q] = 1
        assert call(params=p) == K.E_ARG
    # the stated order: size, threshold, format, planes, pitches, state
    assert call(lambda fr, fmt: setattr(fmt, "layout", 2), params=K.RepeatParams(-1), H=0) == K.E_ARG
    assert call(lambda fr, fmt: setattr(fmt, "layout", 2), params=K.RepeatParams(-1)) == K.E_ARG
    assert call(lambda fr, fmt: (setattr(fmt, "layout", 2), fr.plane.__setitem__(0, None)), state=None) == V.E_FORMAT
    assert call(lambda fr, fmt: (fr.plane.__setitem__(0, None), fr.pitch.__setitem__(0, 1)), state=None) == V.E_PLANE
    assert call(lambda fr, fmt: fr.pitch.__setitem__(0, 2), state=None) == V.E_PITCH
    for field, val in (("layout", 2), ("matrix", 2), ("range", -1), ("depth", 9), ("depth", 12)):
        assert call(lambda fr, fmt: setattr(fmt, field, val)) == V.E_FORMAT, field
    assert call(lambda fr, fmt: fmt.reserved.__setitem__(3, 1)) == V.E_FORMAT
    for q in range(len(shapes)):                                           # every plane of the format is checked, though only plane 0 is read
        assert call(lambda fr, fmt: fr.plane.__setitem__(q, None)) == V.E_PLANE, q
        assert call(lambda fr, fmt: fr.pitch.__setitem__(q, shapes[q][1] * b - b)) == V.E_PITCH, q
        if depth == 10:
            assert call(lambda fr, fmt: fr.plane.__setitem__(q, base + 1)) == V.E_PLANE, q
            assert call(lambda fr, fmt: fr.pitch.__setitem__(q, shapes[q][1] * b + 1)) == V.E_PITCH, q
    assert not buf.any()


def _create(l, h, **kw):
    import fldr_cadence as K
    import fldr_video as V
    cfg = K.make_config(64, 64, V.Format("i420"), 60, 120, 5, 3)
    for k, v in kw.items():
        if k == "mutate":
            v(cfg)
        elif hasattr(cfg, k) and k not in ("rate",):
            setattr(cfg, k, v)
        else:
            setattr(cfg.rate, k, v)
    return l.fldr_cadence_create(None, ctypes.byref(cfg), ctypes.byref(h))


def test_stream_argument_errors_before_any_device_call():
    import fldr_cadence as K
    import fldr_rate as R
    import fldr_video as V
    l = K.lib()
    h = ctypes.c_void_p()
    create = lambda **kw: _create(l, h, **kw)
    assert create() == K.E_ARG                                               # valid, no model: this library's code
    # fldr_rate_create's checks with its codes ...
    assert create(H=1) == R.E_ARG and create(device=-1) == R.E_ARG and create(scene=2) == R.E_ARG
    assert create(mutate=lambda c: c.rate.reserved.__setitem__(2, 1)) == R.E_ARG
    assert create(mutate=lambda c: setattr(c.rate.scene_params, "sad_permille", 1001)) == R.E_ARG
    assert create(mutate=lambda c: setattr(c.rate.format, "layout", 3)) == V.E_FORMAT
    for term in ("in_num", "in_den", "out_num", "out_den"):
        assert create(**{term: 0}) == R.E_RATIO and create(**{term: -24}) == R.E_RATIO, term
    # ... and in its order, before this library's
    assert create(H=1, cycle=0) == R.E_ARG
    assert create(mutate=lambda c: setattr(c.rate.format, "layout", 3), cycle=0) == V.E_FORMAT
    assert create(in_num=0, cycle=0) == R.E_RATIO
    assert create(mutate=lambda c: (setattr(c.rate.format, "layout", 3), setattr(c.rate, "in_num", 0))) == V.E_FORMAT
    # this library's: cycle, drop, repeat, reserved
    for cycle, drop in ((0, 0), (17, 1), (-1, 0), (5, 5), (5, -1), (1, 1), (16, 16)):
        assert create(cycle=cycle, drop=drop) == K.E_ARG, (cycle, drop)
    for cycle, drop in ((1, 0), (16, 15), (16, 0), (2, 1)):
        assert create(cycle=cycle, drop=drop, out_num=60) == K.E_ARG             # allowed (and then no model)
    assert create(mutate=lambda c: setattr(c.repeat, "tile_sad_min", 261121)) == K.E_ARG
    assert create(mutate=lambda c: setattr(c.repeat, "tile_sad_min", -1)) == K.E_ARG
    assert create(mutate=lambda c: c.repeat.reserved.__setitem__(2, 1)) == K.E_ARG
    assert create(mutate=lambda c: c.reserved.__setitem__(1, 1)) == K.E_ARG
    # these come before the limits on the derived ratio ...
    assert create(cycle=0, out_num=60 * 65) == K.E_ARG
    # ... which are fldr_rate_create's, on the DERIVED rate: 60 x 2 / 5 = 24 -> 24 x 64 is allowed, 24 x 65 is not
    assert create(out_num=24 * 64) == K.E_ARG
    assert create(out_num=24 * 65) == R.E_RATIO
    assert create(out_num=60 * 64, cycle=1, drop=0) == K.E_ARG and create(out_num=60 * 64 + 60, cycle=1, drop=0) == R.E_RATIO
    assert create(in_num=2 ** 25 + 1, out_num=2 ** 25, cycle=1, drop=0) == R.E_RATIO      # reduced terms above 2^24
    # a derived term that does not fit int32: (2^31 - 1) x 4 / 5 — though its ratio to the output rate, 4 / 5, would be fine
    assert create(in_num=2 ** 31 - 1, out_num=2 ** 31 - 1, cycle=5, drop=1) == R.E_RATIO
    assert create(in_num=2 ** 31 - 1, out_num=2 ** 31 - 1, cycle=1, drop=0) == K.E_ARG
    assert l.fldr_cadence_create(None, None, ctypes.byref(h)) == K.E_ARG
    n = ctypes.c_int()
    assert l.fldr_cadence_push(None, None, None, ctypes.byref(n), None) == K.E_ARG
    assert l.fldr_cadence_flush(None, None, ctypes.byref(n), None) == K.E_ARG
    assert l.fldr_cadence_reset(None) == K.E_ARG
    assert l.fldr_cadence_max_out(None) == K.E_ARG
    l.fldr_cadence_destroy(None)


@pytest.mark.parametrize("layout,depth", [("nv12", 8), ("i420", 10)])
def test_two_faults_at_once_answer_in_the_recorded_order(layout, depth):
    """The checks of a measure and of a create sit in headers this library shares with the pulldown and probe libraries
    (rate/tile_measure_host.h, rate/cycle_stream_host.h): which of two simultaneous faults is reported is decided there.  Every code
    here was recorded from the library as it was before that text was shared."""
    import fldr_cadence as K
    import fldr_rate as R
    import fldr_video as V
    H = W = 64
    _, base, fr = _frames(V, layout, depth)
    fmt, bad_fmt = V.Format(layout, depth=depth), V.Format(layout, depth=depth)
    bad_fmt.layout = 2
    assert K.repeat_measure_raw(H, W, fmt, fr, K.RepeatParams(-1), base + 16, None) == K.E_ARG         # a bad threshold and a misaligned state
    assert K.repeat_measure_raw(0, W, fmt, fr, None, None, None) == K.E_ARG                           # a bad size and no state
    assert K.repeat_measure_raw(H, W, bad_fmt, fr, None, base + 16, None) == V.E_FORMAT
    # the two frames are checked one after the other, each planes first: a short pitch in I0 comes before a missing plane in I1 ...
    _, base, fr = _frames(V, layout, depth)
    fr[0].pitch[0], fr[1].plane[0] = 2, None
    assert K.repeat_measure_raw(H, W, fmt, fr, None, base, None) == V.E_PITCH
    # ... and a missing chroma plane in I0 before a short luma pitch in I1
    _, base, fr = _frames(V, layout, depth)
    fr[0].plane[1], fr[1].pitch[0] = None, 2
    assert K.repeat_measure_raw(H, W, fmt, fr, None, base, None) == V.E_PLANE
    _, base, fr = _frames(V, layout, depth)
    fr[1].pitch[0] = 2
    assert K.repeat_measure_raw(H, W, fmt, fr, None, base + 16, None) == V.E_PITCH
    # the stream: fldr_rate_create's checks, then cycle, drop, the threshold and the reserved words, then the derived ratio
    l, h = K.lib(), ctypes.c_void_p()
    create = lambda **kw: _create(l, h, **kw)
    many = dict(in_num=30, in_den=1, out_num=24 * 65 * 4, out_den=1)        # the derived rate has too many outputs per frame
    big = dict(in_num=2 ** 31 - 1, in_den=1, out_num=2 ** 31 - 1, out_den=1)   # a derived term outside int32
    assert create(**many) == R.E_RATIO and create(**big) == R.E_RATIO          # alone
    assert create(cycle=0, in_num=0) == R.E_RATIO and create(cycle=17, H=1) == R.E_ARG
    assert create(cycle=0, **many) == K.E_ARG and create(drop=5, **big) == K.E_ARG
    assert create(mutate=lambda c: c.reserved.__setitem__(1, 1), **many) == K.E_ARG
    assert create(mutate=lambda c: setattr(c.repeat, "tile_sad_min", -1), **many) == K.E_ARG
    assert K.inner_rate_raw(0, 1, 0, 0)[0] == K.E_ARG and K.inner_rate_raw(30, 0, 5, 5)[0] == K.E_ARG
    assert K.inner_rate_raw(2 ** 31 - 1, 1, 17, 1)[0] == K.E_ARG


@pytest.mark.parametrize("in_rate,cycle,drop,want", [(60, 5, 3, Fraction(24)), ((60000, 1001), 5, 3, Fraction(24000, 1001)), (30, 5, 1, Fraction(24)),
                                                      (50, 2, 1, Fraction(25)), (24, 1, 0, Fraction(24)), ((30000, 1001), 16, 15, Fraction(1875, 1001))])
def test_the_derived_inner_rate(in_rate, cycle, drop, want):
    import fldr_cadence as K
    q = Fraction(*in_rate) if isinstance(in_rate, tuple) else Fraction(in_rate)
    assert K.inner_rate(in_rate, cycle, drop) == want == q * (cycle - drop) / cycle
    code, num, den = K.inner_rate_raw(q.numerator, q.denominator, cycle, drop)
    assert code == 0 and (num, den) == (want.numerator, want.denominator)     # reduced by the gcd


def test_the_derived_inner_rate_refuses_what_does_not_fit():
    import fldr_cadence as K
    import fldr_rate as R
    assert K.inner_rate_raw(2 ** 31 - 1, 1, 5, 1)[0] == R.E_RATIO               # numerator 4 (2^31 - 1)
    assert K.inner_rate_raw(1, 2 ** 31 - 1, 16, 15)[0] == R.E_RATIO             # denominator 16 (2^31 - 1)
    assert K.inner_rate_raw(2 ** 31 - 1, 1, 1, 0) == (0, 2 ** 31 - 1, 1)
    assert K.inner_rate_raw(2 ** 31 - 2, 1, 2, 1) == (0, 2 ** 30 - 1, 1)        # the reduced terms count, not the products
    assert K.inner_rate_raw(0, 1, 5, 3)[0] == R.E_RATIO and K.inner_rate_raw(60, 0, 5, 3)[0] == R.E_RATIO
    assert K.inner_rate_raw(60, 1, 5, 5)[0] == K.E_ARG and K.inner_rate_raw(60, 1, 0, 0)[0] == K.E_ARG
    assert K.lib().fldr_cadence_inner_rate(None, None, None) == K.E_ARG


# ---- the oracle alone ----------------------------------------------------------------------------------------------------------------------
def test_oracle_measure_on_hand_worked_frames():
    a = np.zeros((33, 65), np.uint8)                                         # tiles: 2 x 3; the last column and the last row are partial
    b = a.copy()
    b[0, 0] = 7                                                              # tile 0
    b[31, 63] = 3                                                            # tile 1, its last sample
    b[0, 64] = 9                                                             # tile 2 (one column wide)
    b[32, 31] = 9                                                            # tile 3 (one row high)
    b[32, 64] = 2                                                            # tile 5 (one sample)
    assert C.tile_sads((a,), (b,)).tolist() == [[7, 3, 9], [9, 0, 2]]
    assert C.measure((a,), (b,), tile_sad_min=9) == {"sad": 30, "max_tile_sad": 9, "max_tile": 2, "moving_tiles": 2, "repeat": 0}
    assert C.measure((a,), (b,), tile_sad_min=10) == {"sad": 30, "max_tile_sad": 9, "max_tile": 2, "moving_tiles": 0, "repeat": 1}
    assert C.measure((a,), (b,)) == C.measure((a,), (b,), tile_sad_min=2048) == C.measure((a,), (b,), tile_sad_min=None)
    assert C.measure((a,), (a,)) == {"sad": 0, "max_tile_sad": 0, "max_tile": 0, "moving_tiles": 0, "repeat": 1}
    assert C.measure((b,), (a,)) == C.measure((a,), (b,))                    # absolute differences
    white = np.full((64, 64), 255, np.uint8)
    assert C.measure((np.zeros_like(white),), (white,)) == {"sad": 4 * 261120, "max_tile_sad": 261120, "max_tile": 0, "moving_tiles": 4, "repeat": 0}
    # depth 10: P010 reads word >> 8, yuv420p10le (word & 0x3ff) >> 2; the other bits are ignored
    w0 = np.array([[0x1200, 0xffc0]], np.uint16)
    w1 = np.array([[0x15ff, 0x003f]], np.uint16)
    assert C.measure((w0,), (w1,), ("nv12", 10), 1)["sad"] == 3 + 255
    assert C.measure((w0,), (w1,), ("i420", 10), 1)["sad"] == abs((0x200 >> 2) - (0x1ff >> 2)) + abs((0x3c0 >> 2) - (0x3f >> 2))


def _m(max_tile_sad, sad=None, repeat=None):
    sad = max_tile_sad if sad is None else sad
    return {"sad": sad, "max_tile_sad": max_tile_sad, "max_tile": 0, "moving_tiles": int(max_tile_sad >= 2048),
            "repeat": int(max_tile_sad < 2048) if repeat is None else repeat}


def _keys(source, noise=lambda n: 3 + n % 4, motion=lambda n: 9000 + 10 * n):
    """Measures of a stream described by its runs: source[n] = (real frame, instance); a repeat measures `noise`, a new frame `motion`."""
    return [None] + [_m(noise(n)) if source[n][0] == source[n - 1][0] else _m(motion(n), 40 * motion(n)) for n in range(1, len(source))]


def _runs(counts, n, first_real=0, first_instance=0):
    out, k, inst = [], first_real, first_instance
    while len(out) < n:
        out.append((k, inst))
        inst += 1
        if inst == counts[k % len(counts)]:
            k, inst = k + 1, 0
    return out


@pytest.mark.parametrize("pattern", list(CF.PATTERNS))
def test_oracle_survivors_are_the_first_instances(pattern):
    cycle, drop, counts = CF.PATTERNS[pattern]
    src = _runs(counts, 4 * cycle)
    kept, reports = C.survivors(_keys(src), cycle, drop)
    assert kept == [n for n, (_, inst) in enumerate(src) if inst == 0]
    assert len(reports) == 4 and all(r["n_frames"] == cycle and bin(r["dropped_mask"]).count("1") == drop for r in reports)
    assert all(r["moving_dropped"] == 0 and r["still_kept"] == 0 for r in reports)
    assert [r["first_frame"] for r in reports] == [0, cycle, 2 * cycle, 3 * cycle]
    assert reports[0]["measure"][0] == C.ZERO                                # frame 0 has no key
    if pattern == "3:2":
        assert [r["dropped_mask"] for r in reports] == [0b10110] * 4          # A A A B B: frames 1, 2 and 4 go


def test_oracle_survivors_static_cut_start_inside_a_run_and_partial_cycle():
    # a static stretch: every key equal -> the lower frame numbers go first; frame 0 of the stream never goes
    kept, reports = C.survivors([None] + [_m(0)] * 9, 5, 3)
    assert kept == [0, 4, 8, 9] and [r["dropped_mask"] for r in reports] == [0b01110, 0b00111]
    assert [r["still_kept"] for r in reports] == [1, 2] and all(r["moving_dropped"] == 0 for r in reports)
    # equal max_tile_sad: the whole-frame sum decides, then the frame number
    kept, reports = C.survivors([None, _m(5, 50), _m(5, 40), _m(5, 40), _m(5, 60)], 5, 3)
    assert kept == [0, 4] and reports[0]["dropped_mask"] == 0b01110          # 40, 40, 50 go
    kept, reports = C.survivors([None, _m(5, 50), _m(5, 40), _m(5, 40), _m(4, 60)], 5, 2)
    assert kept == [0, 1, 3] and reports[0]["dropped_mask"] == 0b10100       # (4, 60) first, then the lower frame of the two (5, 40)
    # a cut in mid-cycle has the largest key and stays, though the cycle then holds a frame too many that moves
    src = _runs((3, 2), 10)
    keys = _keys(src)
    keys[7] = _m(200000, 9000000)                                            # a repeat position (C C C: frame 7) replaced by a new scene
    kept, reports = C.survivors(keys, 5, 3)
    assert kept == [0, 3, 7, 8] and reports[1]["moving_dropped"] == 1        # frame 5 (C, the least of the three that move) had to go instead
    # a start inside a run of repeats (A A | B B B C C ...): the first cycle may lose a real frame, later ones do not
    src = _runs((3, 2), 15, first_real=0, first_instance=1)                  # A A B B A' ... : runs of 2, 2, 3, 2, 3, ...
    kept, reports = C.survivors(_keys(src), 5, 3)
    firsts = [n for n, (_, inst) in enumerate(src) if inst == 0 or n == 0]
    assert [k for k in kept if k >= 5] == [n for n in firsts if n >= 5]
    assert all(r["moving_dropped"] == 0 for r in reports[1:])
    # a partial last cycle of m frames drops floor(m drop / cycle)
    for m, want in ((1, 0), (2, 1), (3, 1), (4, 2)):
        src = _runs((3, 2), 5 + m)
        kept, reports = C.survivors(_keys(src), 5, 3)
        assert reports[-1]["n_frames"] == m and bin(reports[-1]["dropped_mask"]).count("1") == want == m * 3 // 5
        assert len(kept) == 2 + m - want
    assert C.survivors([None], 5, 3) == ([0], [{"first_frame": 0, "n_frames": 1, "dropped_mask": 0, "moving_dropped": 0, "still_kept": 0,
                                                "measure": [C.ZERO]}])
    assert C.survivors([], 5, 3) == ([], [])
    # cycle 1, drop 0: nothing goes
    assert C.survivors([None] + [_m(0)] * 4, 1, 0)[0] == [0, 1, 2, 3, 4]
    # a wrong declaration: 2:2 content declared 5, 3 loses moving frames
    kept, reports = C.survivors(_keys(_runs((2,), 10)), 5, 3)
    assert sum(r["moving_dropped"] for r in reports) >= 1


# ---- the condition on the GPU test's streams -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,depth", CF.FORMATS)
@pytest.mark.parametrize("pattern", list(CF.PATTERNS))
def test_perturbed_repeats_leave_the_first_instances_as_survivors(pattern, layout, depth):
    """What tests/test_gpu_cadence.py assumes of its streams: every repeat is perturbed (no two container frames are equal), by one code
    on at most 8 luma samples, and the oracle's survivors are the first instance of every run, in every cycle."""
    cycle, drop, _ = CF.PATTERNS[pattern]
    frames, source = CF.stream(pattern, layout, depth, 3 * cycle if cycle == 5 else 6 * cycle)
    ms = CF.measures(frames, layout, depth)
    for n in range(1, len(frames)):
        if source[n][1]:                                                     # a repeat, perturbed against the real frame
            real = CF.real_frames(layout, depth)[source[n][0]]
            d = np.abs(C.S.y8(frames[n][0], layout, depth) - C.S.y8(real[0], layout, depth))
            assert 1 <= int((d != 0).sum()) <= 8 and int(d.max()) == 1
            assert all(np.array_equal(p, q) for p, q in zip(frames[n][1:], real[1:]))
            assert ms[n]["repeat"] == 1 and 1 <= ms[n]["sad"] <= 16
        else:
            assert ms[n]["repeat"] == 0 and ms[n]["max_tile_sad"] >= C.default()
    assert len(set(f[0].tobytes() for f in frames)) == len(frames)
    kept, reports = C.survivors(ms, cycle, drop)
    assert kept == [n for n, (_, inst) in enumerate(source) if inst == 0]
    assert all(r["moving_dropped"] == 0 and r["still_kept"] == 0 for r in reports)
    cut = [n for n, (k, inst) in enumerate(source) if k == CF.CUT_AT and inst == 0]
    assert len(cut) == 1 and ms[cut[0]]["max_tile_sad"] == max(m["max_tile_sad"] for m in ms[1:])
