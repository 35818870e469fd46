"""CPU checks of the pulldown API (include/fldr_pulldown.h, libfldr_pulldown.so): the library's symbol table and link, the header as
plain C99 / C++, the C example, the code-generation guards, the binding's struct mirrors, the argument checks of the three layers — which
happen before any device call, so they run without a GPU —, the derived inner rate, the oracle (tests/pulldown_oracle.py) alone on
hand-worked frames, and the condition tests/test_gpu_pulldown.py puts on its input streams."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import pulldown_frames as PF
import pulldown_oracle as O
from lib_checks import declared as _declared, disassemble as _disassemble, syms as _syms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fldr-vfi_amd")
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "fldr_pulldown.h")
LIB = os.path.join(PKG, "libfldr_pulldown.so")
EXAMPLE = os.path.join(ROOT, "examples", "fldr_ivtc.c")
BARRED = ("fldr_field", "fldr_chroma", "fldr_cadence", "fldr_repeat", "fldr_pipe")


# ---- the library ------------------------------------------------------------------------------------------------------------------------
def test_library_exports_exactly_the_header():
    declared = _declared(HDR, "FLDR_PULLDOWN_API")
    assert len(declared) == 12, sorted(declared)
    assert _syms(LIB, ["--defined-only"]) == declared
    import fldr_pulldown
    assert set(fldr_pulldown.EXPORTS) == declared
    for name in ("version", "error_string", "sizeof", "measure", "assemble", "create", "destroy", "max_out", "push", "flush", "reset", "inner_rate"):
        assert "fldr_pulldown_" + name in declared, name


def test_library_links_only_the_rate_video_and_model_apis():
    dyn = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    needed = set(re.findall(r"NEEDED.*\[(libfldr_\w+\.so)\]", dyn))
    assert needed == {"libfldr_rate.so", "libfldr_video.so"}, dyn
    assert re.search(r"R(UN)?PATH.*\[\$ORIGIN\b", dyn), dyn
    used = set(n for n in _syms(LIB, ["--undefined-only"]) if n.startswith("fldr_"))
    allowed = (_declared(os.path.join(INC, "fldr_rate.h"), "FLDR_RATE_API") | _declared(os.path.join(INC, "fldr_video.h"), "FLDR_VIDEO_API") |
               _declared(os.path.join(INC, "fldr_model.h"), "FLDR_MODEL_API"))
    assert used and used <= allowed, sorted(used)
    assert {"fldr_rate_create", "fldr_rate_push", "fldr_rate_flush", "fldr_rate_reset", "fldr_rate_destroy", "fldr_rate_error_string"} <= used


def test_header_and_library_name_none_of_the_libraries_beside_them():
    text = open(HDR).read().lower()
    raw = open(LIB, "rb").read().lower()
    for other in BARRED:
        assert other not in text and other.encode() not in raw, other
    for name in os.listdir(INC):
        if name != "fldr_pulldown.h":
            assert "fldr_pulldown" not in open(os.path.join(INC, name)).read().lower(), name
    for name in os.listdir(PKG):
        if re.fullmatch(r"libfldr_\w+\.so", name) and name != "libfldr_pulldown.so":
            assert b"fldr_pulldown" not in open(os.path.join(PKG, name), "rb").read(), name


@pytest.mark.parametrize("compiler", [["gcc", "-std=c99", "-x", "c"], ["g++", "-std=c++11", "-x", "c++"]])
def test_header_is_plain_c99_and_cxx(compiler, tmp_path):
    assert shutil.which(compiler[0]), compiler[0] + " not installed"
    src = tmp_path / "h.c"
    src.write_text('#include <stddef.h>\n#include "fldr_pulldown.h"\nint main(void) { fldr_pulldown_config c; fldr_pulldown_report r; fldr_pulldown_params p;\n'
                   '  c.cycle = FLDR_PULLDOWN_MAX_CYCLE; r.n_frames = 0; p.comb_thresh = FLDR_PULLDOWN_COMB_THRESH_DEFAULT;\n'
                   '  return fldr_pulldown_sizeof(2) == (int)sizeof(c) && c.cycle == 16 && r.n_frames == 0 && p.comb_thresh == 6 &&\n'
                   '         FLDR_PULLDOWN_STATE_BYTES == 8192 && sizeof(fldr_pulldown_result) == 96 && offsetof(fldr_pulldown_result, match) == 0 &&\n'
                   '         offsetof(fldr_pulldown_result, combed) == 4 && FLDR_PULLDOWN_POST_AVERAGE == 1 && FLDR_PULLDOWN_N == 2 ? 0 : 1; }\n')
    r = subprocess.run(compiler + ["-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I" + INC, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "hip" not in re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S).lower()


def test_header_defines_no_error_code_and_says_whose_it_returns():
    text = open(HDR).read()
    assert not re.findall(r"#define\s+FLDR_[A-Z0-9]+_E_[A-Z]+", text)
    for s in ("defines no code of its own", "FLDR_RATE_E_ARG", "FLDR_RATE_E_STATE", "FLDR_RATE_E_RATIO", "FLDR_RATE_E_DEVICE",
              "fldr_pulldown_error_string is fldr_rate_error_string"):
        assert s in text, s
    import fldr_pulldown as K
    import fldr_rate as R
    l = K.lib()
    for code in (R.E_ARG, R.E_STATE, R.E_RATIO, R.E_DEVICE, -101, -3, 0, -999):
        assert l.fldr_pulldown_error_string(code) == R.lib().fldr_rate_error_string(code)
    assert (K.E_ARG, K.E_STATE, K.E_RATIO, K.E_DEVICE) == (R.E_ARG, R.E_STATE, R.E_RATIO, R.E_DEVICE)


def test_header_says_where_the_defaults_come_from_and_what_is_out_of_scope():
    text = open(HDR).read()
    assert "synthetic content only" in text and "not on footage" in text and "A maintainer with footage should look at" in text
    for s in ("downloaded here and uploaded again", "a frame plus a cycle late", "cycle and drop are not detected", "plain three-line one",
              "one-line-high static detail", "chroma follows the luma decision", "4:2:2, packed and RGB interlaced formats are out of scope",
              "the stream is synchronous", "Validation order"):
        assert s in text, s
    assert O.defaults() == (6, 32, 1024)


def test_example_builds_with_cc(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    exe = tmp_path / "fldr_ivtc"
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + INC, "-o", str(exe), EXAMPLE, "-L" + PKG,
                        "-l:libfldr_pulldown.so", "-l:libfldr_rate.so", "-l:libfldr_video.so", "-l:libfldr_model.so", "-Wl,-rpath," + PKG],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    src = open(EXAMPLE).read()
    assert "hip" not in re.sub(r"/\*.*?\*/", "", src, flags=re.S).lower()
    u = subprocess.run([str(exe)], capture_output=True, text=True)            # no arguments: usage, no device touched
    assert u.returncode == 2 and "usage" in u.stderr and "cycle=" in u.stderr and "anchor=top|bottom" in u.stderr and "post=keep|average" in u.stderr
    for bad in (["w.npz", "64", "64", "30", "60", "cycle=5"],                 # no drop=
                ["w.npz", "64", "64", "30", "60", "cycle=5", "drop=5"],       # drop not below cycle
                ["w.npz", "64", "64", "30", "60", "cycle=17", "drop=1"],
                ["w.npz", "64", "66", "30", "60", "cycle=5", "drop=1"],       # H not a multiple of 4
                ["w.npz", "64", "64", "30", "60", "cycle=5", "drop=1", "anchor=left"],
                ["w.npz", "64", "64", "30", "60", "cycle=5", "drop=1", "post=blend"],
                ["w.npz", "64", "64", "30/0", "60", "cycle=5", "drop=1"]):
        u = subprocess.run([str(exe)] + bad, capture_output=True, text=True)
        assert u.returncode == 2 and "usage" in u.stderr, bad


def test_no_unsafe_packed_fp32_in_the_pulldown_library():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_pk_opsel.py"), LIB], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_kernels_use_16_byte_accesses_the_sad_instructions_integer_atomics_and_no_float():
    txt = "\n".join(_disassemble(LIB))
    for k in ("pulldown_zero_kernel", "pulldown_tiles_kernel", "pulldown_result_kernel", "pulldown_assemble_kernel"):
        assert k in txt, k
    assert re.search(r"\bv_sad_u8\b", txt) and re.search(r"\bv_sad_u16\b", txt)
    assert re.search(r"\bglobal_atomic_umax_x2\b", txt) and re.search(r"\bglobal_atomic_add_x2\b", txt)   # the 64-bit keys and sums
    assert re.search(r"\bglobal_load_dwordx4\b", txt) and re.search(r"\bglobal_store_dwordx4\b", txt)     # 16 bytes per lane
    # no float anywhere: no conversion, no float arithmetic (an integer division would bring v_cvt_f32_u32 and v_rcp with it)
    assert not re.search(r"\bv_(cvt_f|rcp|add_f|mul_f|fma_f|mac_f|pk_\w+_f)", txt)


def test_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    ks = KR.kernels(LIB)
    assert len(ks) == 11, [k["name"] for k in ks]         # zero, result, tiles x (3 sample forms x wide / per-sample), assemble x 3 sample forms
    for k in ks:
        assert k.get("scratch", -1) == 0 and k.get("vgpr_spills", -1) == 0 and k.get("sgpr_spills", -1) == 0, k


def test_binding_struct_sizes_and_version():
    import fldr_pulldown as K
    l = K.lib()
    text = open(HDR).read()
    assert l.fldr_pulldown_version() == K.PULLDOWN_VERSION == int(re.search(r"#define FLDR_PULLDOWN_VERSION (\d+)", text).group(1)) == 100
    for which, cls in enumerate((K.Params, K.Result, K.PulldownConfig, K.Report)):
        assert l.fldr_pulldown_sizeof(which) == ctypes.sizeof(cls)
    assert ctypes.sizeof(K.Params) == 32 and ctypes.sizeof(K.Result) == 96 and ctypes.sizeof(K.Report) == 104 + 16 * 96
    assert K.Result.match.offset == 0 and K.Result.combed.offset == 4
    assert l.fldr_pulldown_sizeof(4) == K.E_ARG and l.fldr_pulldown_sizeof(-1) == K.E_ARG
    for macro, v in (("FLDR_PULLDOWN_STATE_BYTES", K.STATE_BYTES), ("FLDR_PULLDOWN_MAX_CYCLE", K.MAX_CYCLE), ("FLDR_PULLDOWN_TILE", K.TILE),
                     ("FLDR_PULLDOWN_TILE_COMB_MAX", K.TILE_COMB_MAX), ("FLDR_PULLDOWN_TILE_SAD_MAX", K.TILE_SAD_MAX),
                     ("FLDR_PULLDOWN_COMB_THRESH_DEFAULT", K.COMB_THRESH_DEFAULT), ("FLDR_PULLDOWN_COMB_TILE_DEFAULT", K.COMB_TILE_DEFAULT),
                     ("FLDR_PULLDOWN_TILE_SAD_DEFAULT", K.TILE_SAD_DEFAULT), ("FLDR_PULLDOWN_C", K.C), ("FLDR_PULLDOWN_P", K.P), ("FLDR_PULLDOWN_N", K.N),
                     ("FLDR_PULLDOWN_POST_KEEP", K.POST_KEEP), ("FLDR_PULLDOWN_POST_AVERAGE", K.POST_AVERAGE)):
        assert int(re.search(r"#define %s\s+(\d+)" % macro, text).group(1)) == v, macro
    assert K.TILE_COMB_MAX == 16 * 32 and K.TILE_SAD_MAX == 16 * 32 * 255 and (K.C, K.P, K.N) == (O.C, O.P, O.N) and K.POST_AVERAGE == O.AVERAGE


# ---- argument errors without a device ---------------------------------------------------------------------------------------------------
H0 = W0 = 64


def _host(V, layout, depth, H=H0, W=W0, count=4):
    """`count` frames whose planes all point into one zeroed, 256-byte aligned host buffer, each frame in a part of its own."""
    b = 2 if depth == 10 else 1
    part = H * W * 2 * b
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


@pytest.mark.parametrize("layout", ["nv12", "i420"])
@pytest.mark.parametrize("depth", [8, 10])
def test_measure_argument_errors_before_any_device_call(layout, depth):
    import fldr_pulldown as K
    import fldr_video as V
    b = 2 if depth == 10 else 1
    buf, base, _ = _host(V, layout, depth)
    shapes = V.plane_shapes(layout, H0, W0)
    state = base + 4 * H0 * W0 * 2 * b

    def call(mutate=lambda fr, fmt: None, params=None, state=state, H=H0, W=W0, anchor=0, prev=True, nxt=True, cur=True, which=2):
        _, _, fr = _host(V, layout, depth)
        fmt = V.Format(layout, depth=depth)
        mutate(fr[which], fmt)
        return K.measure_raw(H, W, fmt, fr[0] if cur else None, fr[1] if prev else None, fr[2] if nxt else None, anchor, params, state, None)
    assert call(state=None) == K.E_STATE
    assert call(state=base + 128) == K.E_STATE and call(state=base + 16) == K.E_STATE
    for H in (0, -4, 2, 6, 62, 65, 2 ** 31 - 4):                           # at least 4, a multiple of 4, whole tiles inside 32 bits
        assert call(H=H) == K.E_ARG, H
    assert call(W=0) == K.E_ARG and call(W=-1) == K.E_ARG and call(H=4, W=2 ** 31 - 1) == K.E_ARG
    assert call(anchor=2) == K.E_ARG and call(anchor=-1) == K.E_ARG and call(anchor=1, state=None) == K.E_STATE
    assert call(cur=False) == K.E_ARG
    assert K.measure_raw(H0, W0, None, _host(V, layout, depth)[2][0], None, None, 0, K.Params(allowed=1), state, None) == K.E_ARG
    for bad in (dict(comb_thresh=-1), dict(comb_thresh=256), dict(comb_tile_min=-1), dict(comb_tile_min=513), dict(tile_sad_min=-1),
                dict(tile_sad_min=130561), dict(allowed=8), dict(allowed=-1)):
        assert call(params=K.Params(**bad)) == K.E_ARG, bad
    for ok in (dict(comb_thresh=255), dict(comb_thresh=1), dict(comb_tile_min=512), dict(tile_sad_min=130560), dict(allowed=7)):
        assert call(params=K.Params(**ok), state=None) == K.E_STATE, ok
    for i in range(4):
        p = K.Params()
        p.reserved[i] = 1
        assert call(params=p) == K.E_ARG
    # a frame may be NULL exactly when `allowed` does not need it; the default needs all three
    assert call(prev=False) == K.E_ARG and call(nxt=False) == K.E_ARG
    assert call(prev=False, params=K.Params(allowed=5), state=None) == K.E_STATE and call(prev=False, params=K.Params(allowed=7)) == K.E_ARG
    assert call(nxt=False, params=K.Params(allowed=3), state=None) == K.E_STATE and call(nxt=False, params=K.Params(allowed=4)) == K.E_ARG
    assert call(prev=False, nxt=False, params=K.Params(allowed=1), state=None) == K.E_STATE
    # the stated order: size and anchor, parameters, format, planes, pitches, state
    assert call(lambda fr, fmt: setattr(fmt, "layout", 2), params=K.Params(comb_thresh=-1), H=6) == K.E_ARG
    assert call(lambda fr, fmt: setattr(fmt, "layout", 2), params=K.Params(comb_thresh=-1)) == K.E_ARG
    assert call(lambda fr, fmt: (setattr(fmt, "layout", 2), fr.plane.__setitem__(0, None)), state=None) == V.E_FORMAT
    assert call(lambda fr, fmt: (fr.plane.__setitem__(0, None), fr.pitch.__setitem__(0, 1)), state=None) == V.E_PLANE
    assert call(lambda fr, fmt: fr.pitch.__setitem__(0, 2), state=None) == V.E_PITCH
    # a missing plane of the LAST frame is reported before a short pitch of the first
    _, _, fr = _host(V, layout, depth)
    fr[0].pitch[0] = 2
    fr[2].plane[0] = None
    assert K.measure_raw(H0, W0, V.Format(layout, depth=depth), fr[0], fr[1], fr[2], 0, None, state, None) == V.E_PLANE
    for field, val in (("layout", 2), ("matrix", 2), ("range", -1), ("depth", 9), ("depth", 12)):
        assert call(lambda fr, fmt: setattr(fmt, field, val)) == V.E_FORMAT, field
    assert call(lambda fr, fmt: fmt.reserved.__setitem__(3, 1)) == V.E_FORMAT
    for which in range(3):                                                  # every plane of every frame is checked, though only plane 0 is read
        for q in range(len(shapes)):
            assert call(lambda fr, fmt: fr.plane.__setitem__(q, None), which=which) == V.E_PLANE, (which, q)
            assert call(lambda fr, fmt: fr.pitch.__setitem__(q, shapes[q][1] * b - b), which=which) == V.E_PITCH, (which, q)
            if depth == 10:
                assert call(lambda fr, fmt: fr.plane.__setitem__(q, base + 1), which=which) == V.E_PLANE, (which, q)
                assert call(lambda fr, fmt: fr.pitch.__setitem__(q, shapes[q][1] * b + 1), which=which) == V.E_PITCH, (which, q)
    assert not buf.any()


@pytest.mark.parametrize("layout,depth", [("nv12", 8), ("i420", 10)])
def test_assemble_argument_errors_before_any_device_call(layout, depth):
    import fldr_pulldown as K
    import fldr_video as V
    b = 2 if depth == 10 else 1
    buf, base, _ = _host(V, layout, depth)
    shapes = V.plane_shapes(layout, H0, W0)
    decision = base + 4 * H0 * W0 * 2 * b

    def call(mutate=lambda fr, fmt: None, H=H0, W=W0, anchor=0, match=0, combed=0, decision=None, post=0, which=3, use=(True, True, True, True)):
        _, _, fr = _host(V, layout, depth)
        fmt = V.Format(layout, depth=depth)
        mutate(fr[which], fmt)
        fr = [f if u else None for f, u in zip(fr, use)]
        return K.assemble_raw(H, W, fmt, fr[0], fr[1], fr[2], fr[3], anchor, match, combed, decision, post, None)
    bad_format = lambda fr, fmt: setattr(fmt, "layout", 2)
    # every argument error comes before the format, so a call that is otherwise valid is shown to pass them by reaching it
    assert call(bad_format) == V.E_FORMAT
    for H in (0, 2, 6, 66, -4):
        assert call(H=H) == K.E_ARG, H
    assert call(W=0) == K.E_ARG and call(anchor=2) == K.E_ARG and call(anchor=-1) == K.E_ARG
    assert call(match=3) == K.E_ARG and call(match=-2) == K.E_ARG and call(post=2) == K.E_ARG and call(post=-1) == K.E_ARG
    assert call(match=-1) == K.E_ARG and call(match=-1, decision=decision + 2) == K.E_ARG          # read on the device: a pointer is needed
    assert call(bad_format, match=-1, decision=decision + 4) == V.E_FORMAT
    assert call(bad_format, match=-1, decision=decision, use=(True, False, False, True)) == V.E_FORMAT      # a NULL frame then stands for cur
    assert call(use=(False, True, True, True)) == K.E_ARG and call(use=(True, True, True, False)) == K.E_ARG
    assert call(match=1, use=(True, False, True, True)) == K.E_ARG and call(match=2, use=(True, True, False, True)) == K.E_ARG
    assert call(bad_format, match=0, use=(True, False, False, True)) == V.E_FORMAT
    assert call(bad_format, match=1, use=(True, True, False, True), post=1, combed=7, anchor=1) == V.E_FORMAT
    assert K.assemble_raw(H0, W0, None, None, None, None, None, 0, 0, 0, None, 0, None) == K.E_ARG
    # then planes and pitches of cur, prev, next, out
    for which in range(4):
        for q in range(len(shapes)):
            assert call(lambda fr, fmt: fr.plane.__setitem__(q, None), which=which) == V.E_PLANE, (which, q)
            assert call(lambda fr, fmt: fr.pitch.__setitem__(q, shapes[q][1] * b - b), which=which) == V.E_PITCH, (which, q)
    _, _, fr = _host(V, layout, depth)
    fr[0].pitch[0] = 2
    fr[3].plane[1] = None
    assert K.assemble_raw(H0, W0, V.Format(layout, depth=depth), fr[0], fr[1], fr[2], fr[3], 0, 0, 0, None, 0, None) == V.E_PLANE
    # last: out overlaps an input — the whole frame, one plane on another, the last byte of a plane
    fmt = V.Format(layout, depth=depth)
    for k in range(3):
        _, _, fr = _host(V, layout, depth)
        assert K.assemble_raw(H0, W0, fmt, fr[0], fr[1], fr[2], fr[k], 0, 0, 0, None, 0, None) == K.E_ARG, k
        _, _, fr = _host(V, layout, depth)
        fr[3].plane[1] = fr[k].plane[0] + H0 * W0 * b - b                   # out's chroma begins on the last sample of an input's luma
        assert K.assemble_raw(H0, W0, fmt, fr[0], fr[1], fr[2], fr[3], 0, 0, 0, None, 0, None) == K.E_ARG, k
    assert not buf.any()


def _create(l, h, **kw):
    import fldr_pulldown as K
    import fldr_video as V
    cfg = K.make_config(64, 64, V.Format("i420"), (30000, 1001), (60000, 1001), 5, 1)
    for k, v in kw.items():
        if k == "mutate":
            v(cfg)
        elif hasattr(cfg, k) and k not in ("rate",):
            setattr(cfg, k, v)
        else:
            setattr(cfg.rate, k, v)
    return l.fldr_pulldown_create(None, ctypes.byref(cfg), ctypes.byref(h))


def test_stream_argument_errors_before_any_device_call():
    import fldr_pulldown as K
    import fldr_rate as R
    import fldr_video as V
    l = K.lib()
    h = ctypes.c_void_p()
    create = lambda **kw: _create(l, h, **kw)
    ratio_bad = dict(out_num=24 * 65, out_den=1, in_num=30, in_den=1)        # 30 x 4 / 5 = 24 -> 24 x 65: one output too many per frame
    assert create() == K.E_ARG                                               # valid, no model
    assert create(**ratio_bad) == R.E_RATIO                                  # ... and what comes before the model is seen through this
    # fldr_rate_create's checks with its codes ...
    assert create(H=1) == R.E_ARG and create(device=-1) == R.E_ARG and create(scene=2) == R.E_ARG
    assert create(mutate=lambda c: c.rate.reserved.__setitem__(2, 1)) == R.E_ARG
    assert create(mutate=lambda c: setattr(c.rate.scene_params, "sad_permille", 1001)) == R.E_ARG
    assert create(mutate=lambda c: setattr(c.rate.format, "layout", 3)) == V.E_FORMAT
    for term in ("in_num", "in_den", "out_num", "out_den"):
        assert create(**{term: 0}) == R.E_RATIO and create(**{term: -24}) == R.E_RATIO, term
    # ... and in its order, before this library's
    assert create(mutate=lambda c: setattr(c.rate.format, "layout", 3), cycle=0) == V.E_FORMAT
    assert create(in_num=0, cycle=0) == R.E_RATIO and create(in_num=0, H=66) == R.E_RATIO
    # this library's, all before the derived ratio: H a multiple of 4, cycle, drop, anchor, post, the parameters, the reserved words
    for H in (2, 62, 66):
        assert create(H=H, **ratio_bad) == K.E_ARG, H
    for cycle, drop in ((0, 0), (17, 1), (-1, 0), (5, 5), (5, -1), (1, 1), (16, 16)):
        assert create(cycle=cycle, drop=drop, **ratio_bad) == K.E_ARG, (cycle, drop)
    for cycle, drop in ((1, 0), (16, 15), (16, 0), (2, 1)):
        assert create(cycle=cycle, drop=drop) == K.E_ARG                         # allowed (and then no model)
    for field, bad in (("anchor", 2), ("anchor", -1), ("post", 2), ("post", -1)):
        assert create(**dict(ratio_bad, **{field: bad})) == K.E_ARG, field
    assert create(anchor=1, post=1, **ratio_bad) == R.E_RATIO
    for field, bad in (("comb_thresh", 256), ("comb_thresh", -1), ("comb_tile_min", 513), ("tile_sad_min", 130561), ("allowed", 8), ("allowed", -1)):
        assert create(mutate=lambda c: setattr(c.params, field, bad), **ratio_bad) == K.E_ARG, field
    assert create(mutate=lambda c: c.params.reserved.__setitem__(3, 1), **ratio_bad) == K.E_ARG
    assert create(mutate=lambda c: c.reserved.__setitem__(3, 1), **ratio_bad) == K.E_ARG
    # the limits on the derived ratio are fldr_rate_create's, on the DERIVED rate: 30 x 4 / 5 = 24 -> 24 x 64 is allowed, 24 x 65 is not
    assert create(in_num=30, in_den=1, out_num=24 * 64, out_den=1) == K.E_ARG
    assert create(in_num=30, in_den=1, out_num=30 * 64, out_den=1, cycle=1, drop=0) == K.E_ARG
    assert create(in_num=30, in_den=1, out_num=30 * 64 + 30, out_den=1, cycle=1, drop=0) == R.E_RATIO
    assert create(in_num=2 ** 25 + 1, in_den=1, out_num=2 ** 25, out_den=1, cycle=1, drop=0) == R.E_RATIO      # reduced terms above 2^24
    assert create(in_num=2 ** 31 - 1, in_den=1, out_num=2 ** 31 - 1, out_den=1, cycle=5, drop=1) == R.E_RATIO  # a derived term outside int32
    assert l.fldr_pulldown_create(None, None, ctypes.byref(h)) == K.E_ARG
    n = ctypes.c_int()
    assert l.fldr_pulldown_push(None, None, None, ctypes.byref(n), None) == K.E_ARG
    assert l.fldr_pulldown_flush(None, None, ctypes.byref(n), None) == K.E_ARG
    assert l.fldr_pulldown_reset(None) == K.E_ARG
    assert l.fldr_pulldown_max_out(None) == K.E_ARG
    l.fldr_pulldown_destroy(None)


@pytest.mark.parametrize("layout,depth", [("nv12", 8), ("i420", 10)])
def test_two_faults_at_once_answer_in_the_recorded_order(layout, depth):
    """The checks of a measure and of a create sit in headers this library shares with the cadence and probe libraries
    (rate/tile_measure_host.h, rate/cycle_stream_host.h): which of two simultaneous faults is reported is decided there.  Every code
    here was recorded from the library as it was before that text was shared."""
    import fldr_pulldown as K
    import fldr_rate as R
    import fldr_video as V
    b = 2 if depth == 10 else 1
    buf, base, fr = _host(V, layout, depth)
    state = base + 4 * H0 * W0 * 2 * b
    fmt, bad_fmt = V.Format(layout, depth=depth), V.Format(layout, depth=depth)
    bad_fmt.layout = 2
    assert K.measure_raw(H0, W0, fmt, fr[0], fr[1], fr[2], 0, K.Params(comb_thresh=-1), state + 16, None) == K.E_ARG   # a bad parameter and a misaligned state
    assert K.measure_raw(H0, W0, fmt, fr[0], fr[1], fr[2], 2, None, None, None) == K.E_ARG                             # a bad anchor and no state
    assert K.measure_raw(H0, W0, bad_fmt, fr[0], None, fr[2], 0, None, state, None) == K.E_ARG                         # a frame `allowed` needs, and a bad format
    assert K.measure_raw(H0, W0, bad_fmt, fr[0], fr[1], fr[2], 0, None, state + 16, None) == V.E_FORMAT
    fr[1].pitch[0] = 2
    assert K.measure_raw(H0, W0, fmt, fr[0], fr[1], fr[2], 0, None, state + 16, None) == V.E_PITCH
    _, _, fr = _host(V, layout, depth)
    fr[0].pitch[1], fr[1].plane[1] = 2, None                                 # every plane of every frame before any pitch
    assert K.measure_raw(H0, W0, fmt, fr[0], fr[1], fr[2], 0, None, state, None) == V.E_PLANE
    _, _, fr = _host(V, layout, depth)
    fr[3].plane[0], fr[3].pitch[1] = fr[0].plane[0], 1                       # out on cur, and a short pitch in out: the frames before the overlap
    assert K.assemble_raw(H0, W0, fmt, fr[0], fr[1], fr[2], fr[3], 0, 0, 0, None, 0, None) == V.E_PITCH
    # the stream: fldr_rate_create's checks, then this library's, then the derived ratio
    l, h = K.lib(), ctypes.c_void_p()
    create = lambda **kw: _create(l, h, **kw)
    many = dict(in_num=30, in_den=1, out_num=24 * 65 * 4, out_den=1)        # the derived rate has too many outputs per frame
    big = dict(in_num=2 ** 31 - 1, in_den=1, out_num=2 ** 31 - 1, out_den=1)   # a derived term outside int32
    assert create(**many) == R.E_RATIO and create(**big) == R.E_RATIO          # alone
    assert create(cycle=0, in_num=0) == R.E_RATIO and create(H=66, in_num=0) == R.E_RATIO and create(cycle=17, H=1) == R.E_ARG
    assert create(cycle=0, **many) == K.E_ARG and create(drop=5, **big) == K.E_ARG
    assert create(mutate=lambda c: c.reserved.__setitem__(1, 1), **many) == K.E_ARG
    assert create(mutate=lambda c: setattr(c.params, "allowed", 8), **many) == K.E_ARG
    assert K.inner_rate_raw(0, 1, 0, 0)[0] == K.E_ARG and K.inner_rate_raw(30, 0, 5, 5)[0] == K.E_ARG
    assert K.inner_rate_raw(2 ** 31 - 1, 1, 17, 1)[0] == K.E_ARG


@pytest.mark.parametrize("in_rate,cycle,drop,want", [((30000, 1001), 5, 1, Fraction(24000, 1001)), (30, 5, 1, Fraction(24)), (25, 1, 0, Fraction(25)),
                                                      (60, 5, 3, Fraction(24)), ((30000, 1001), 16, 15, Fraction(1875, 1001))])
def test_the_derived_inner_rate(in_rate, cycle, drop, want):
    import fldr_pulldown as K
    q = Fraction(*in_rate) if isinstance(in_rate, tuple) else Fraction(in_rate)
    assert K.inner_rate(in_rate, cycle, drop) == O.inner_rate(in_rate, cycle, drop) == want == q * (cycle - drop) / cycle
    code, num, den = K.inner_rate_raw(q.numerator, q.denominator, cycle, drop)
    assert code == 0 and (num, den) == (want.numerator, want.denominator)     # reduced by the gcd


def test_the_derived_inner_rate_refuses_what_does_not_fit():
    import fldr_pulldown as K
    assert K.inner_rate_raw(2 ** 31 - 1, 1, 5, 1)[0] == K.E_RATIO               # numerator 4 (2^31 - 1)
    assert K.inner_rate_raw(1, 2 ** 31 - 1, 16, 15)[0] == K.E_RATIO             # denominator 16 (2^31 - 1)
    assert K.inner_rate_raw(2 ** 31 - 1, 1, 1, 0) == (0, 2 ** 31 - 1, 1)
    assert K.inner_rate_raw(2 ** 31 - 2, 1, 2, 1) == (0, 2 ** 30 - 1, 1)        # the reduced terms count, not the products
    assert K.inner_rate_raw(0, 1, 5, 1)[0] == K.E_RATIO and K.inner_rate_raw(30, 0, 5, 1)[0] == K.E_RATIO
    assert K.inner_rate_raw(30, 1, 5, 5)[0] == K.E_ARG and K.inner_rate_raw(30, 1, 0, 0)[0] == K.E_ARG
    assert K.lib().fldr_pulldown_inner_rate(None, None, None) == K.E_ARG


# ---- the oracle alone ----------------------------------------------------------------------------------------------------------------------
def _frame(rows):
    return (np.array(rows, np.uint8),)


def test_oracle_combing_on_hand_worked_frames():
    # 4 x 4, q = 0: the only row that counts is row 1 (row 3 is the last row); a = row 0, b = row 2
    cur = _frame([[100, 100, 100, 100], [106, 107, 93, 100], [100, 100, 100, 100], [0, 0, 0, 0]])
    prev = _frame([[0] * 4, [94, 92, 120, 100], [0] * 4, [255] * 4])
    nxt = _frame([[0] * 4, [100] * 4, [0] * 4, [255] * 4])
    r = O.measure(cur, prev, nxt, q=0)
    assert r["comb"] == [2, 2, 0]            # C: 36 is not above 36, 49 and 49 are; P: 36 is not, 64 and 400 are; N: m equal to a and b
    assert r["match"] == 2 and r["combed"] == 0 and r["max_tile_comb"] == [2, 2, 0] and r["max_tile"] == [0, 0, 0]
    assert O.measure(cur, prev, nxt, q=0, comb_thresh=7)["comb"] == [0, 2, 0]            # 49 is not above 49
    assert O.measure(cur, prev, nxt, q=0, comb_thresh=255)["comb"] == [0, 0, 0]
    # m between a and b never counts, however far from both
    cur = _frame([[0, 255, 10, 200], [128, 128, 200, 10], [255, 0, 200, 10], [9, 9, 9, 9]])
    assert O.measure(cur, cur, cur, q=0, comb_thresh=1)["comb"] == [0, 0, 0]
    # the extreme product: a = b = 0, m = 255 gives 65025, above 254^2 and not above 255^2
    cur = _frame([[0] * 4, [255] * 4, [0] * 4, [255] * 4])
    assert O.measure(cur, cur, cur, q=0, comb_thresh=254)["comb"] == [4, 4, 4] and O.measure(cur, cur, cur, q=0, comb_thresh=255)["comb"] == [0, 0, 0]
    # q = 1: the rows that count are the even ones but row 0: row 2, between rows 1 and 3
    assert O.measure(cur, cur, cur, q=1, comb_thresh=255)["comb"] == [0, 0, 0]   # rows 1 and 3 are 255, row 2 is 0: 255 x 255 again
    assert O.measure(cur, cur, cur, q=1, comb_thresh=254)["comb"] == [4, 4, 4] and O.measure(cur, cur, cur, q=1)["comb"] == [4, 4, 4]
    # rows 0 and H - 1 are skipped: an 8 x 8 frame whose only odd ones out are there
    flat = np.full((8, 8), 50, np.uint8)
    top, bottom = flat.copy(), flat.copy()
    top[0] = 250
    bottom[7] = 250
    assert O.measure((flat,), (top,), (bottom,), q=1)["comb"] == [0, 0, 0] and O.measure((flat,), (bottom,), (top,), q=0)["comb"] == [0, 0, 0]
    inner = flat.copy()
    inner[3] = 250
    assert O.measure((flat,), (inner,), (inner,), q=0)["comb"] == [0, 8, 8] and O.measure((flat,), (inner,), (inner,), q=1)["comb"] == [0, 0, 0]


def test_oracle_decision_ties_allowed_masks_and_the_repeat_words():
    flat = np.full((8, 8), 50, np.uint8)
    one, two = flat.copy(), flat.copy()
    one[3, 0] = 250                                                         # one combed sample as a candidate for q = 0
    two[3, :2] = 250
    r = O.measure((flat,), (flat.copy(),), (flat.copy(),))
    assert r["match"] == O.C and r["comb"] == [0, 0, 0]                        # all equal: C, then P, then N
    assert O.measure((one,), (flat,), (flat,))["match"] == O.P                 # P and N tie below C: P
    assert O.measure((one,), (two,), (flat,))["match"] == O.N
    assert O.measure((one,), (one,), (two,))["match"] == O.C                   # C and P tie: C
    # the allowed masks: the winner among those allowed only
    assert [O.measure((two,), (one,), (flat,), allowed=a)["match"] for a in range(1, 8)] == [0, 1, 1, 2, 2, 2, 2]
    # lexicographic: the largest tile first, the sum second — 40 x 40, two tile columns and rows
    cur = np.full((40, 40), 50, np.uint8)
    p, n = cur.copy(), cur.copy()
    p[1, 0:3] = 250                                                         # three in tile 0
    n[1, 0:2] = n[1, 32:34] = n[33, 0:2] = 250                             # two in each of tiles 0, 1 and 2: six in all
    r = O.measure((cur,), (p,), (n,), allowed=6)
    assert r["comb"] == [0, 3, 6] and r["max_tile_comb"] == [0, 3, 2] and r["match"] == O.N and r["max_tile"] == [0, 0, 0]
    n[1, 2] = 250                                                           # now three in tile 0: equal maxima, the smaller sum wins
    r = O.measure((cur,), (p,), (n,), allowed=6)
    assert r["max_tile_comb"] == [0, 3, 3] and r["match"] == O.P
    # combed: the largest tile of the match against comb_tile_min, inclusive
    assert O.measure((cur,), (p,), (n,), allowed=2, comb_tile_min=3)["combed"] == 1 and O.measure((cur,), (p,), (n,), allowed=2, comb_tile_min=4)["combed"] == 0
    # the repeat words: the anchor rows only
    moved = cur.copy()
    moved[0, 39] += 7                                                       # row 0 is an anchor row for q = 0, not for q = 1
    moved[35, 0] += 9                                                       # row 35 the other way round
    r0, r1 = O.measure((cur,), (moved,), (cur,), q=0, tile_sad_min=7), O.measure((cur,), (moved,), (cur,), q=1, tile_sad_min=10)
    assert (r0["dup_sad"], r0["dup_max_tile_sad"], r0["dup_max_tile"], r0["dup_moving_tiles"]) == (7, 7, 1, 1)
    assert (r1["dup_sad"], r1["dup_max_tile_sad"], r1["dup_max_tile"], r1["dup_moving_tiles"]) == (9, 9, 2, 0)
    none = O.measure((cur,), None, (cur,), allowed=5)
    assert (none["dup_sad"], none["dup_max_tile_sad"], none["dup_max_tile"], none["dup_moving_tiles"], none["comb"][1]) == (0, 0, 0, 0, 0)
    with pytest.raises(AssertionError):
        O.measure((cur,), None, (cur,), allowed=7)
    # depth 10: P010 reads word >> 8, yuv420p10le (word & 0x3ff) >> 2; the other bits are ignored
    w = np.array([[0x1200] * 2, [0x19ff, 0x18ff], [0x12ff] * 2, [0] * 2], np.uint16)      # y8: 0x12, (0x19, 0x18), 0x12
    assert O.measure((w,), (w,), (w,), ("nv12", 10))["comb"] == [1, 1, 1]          # 7 x 7 is above 36, 6 x 6 is not
    v = np.array([[0x48 | 0xfc00] * 2, [0x67, 0x60], [0x4b] * 2, [0] * 2], np.uint16)     # y8: 0x12, (0x19, 0x18), 0x12
    assert O.measure((v,), (v,), (v,), ("i420", 10))["comb"] == [1, 1, 1]


def test_oracle_assemble_and_the_average_at_the_edge_rows():
    cur = (np.arange(32, dtype=np.uint8).reshape(8, 4) * 3, np.arange(16, dtype=np.uint8).reshape(4, 4) + 100)
    prev = tuple(p + 50 for p in cur)
    nxt = tuple(p + 90 for p in cur)
    for q in (0, 1):
        for match, src in enumerate((cur, prev, nxt)):
            for combed in (0, 1):
                out = O.assemble(cur, prev, nxt, ("nv12", 8), q, match, combed, O.KEEP)
                for o, c, s in zip(out, cur, src):
                    assert np.array_equal(o[q::2], c[q::2]) and np.array_equal(o[1 - q::2], s[1 - q::2])
            assert all(np.array_equal(a, b) for a, b in zip(O.assemble(cur, prev, nxt, ("nv12", 8), q, match, 0, O.AVERAGE),
                                                            O.assemble(cur, prev, nxt, ("nv12", 8), q, match, 0, O.KEEP)))      # not combed: kept
    # q = 1: row 0 is rebuilt from row 1 twice; q = 0: the last row from the row above it twice
    y = np.array([[10, 11], [20, 23], [30, 33], [41, 44]], np.uint8)
    c = np.array([[1, 2], [5, 8]], np.uint8)
    out = O.assemble((y, c), (y, c), (y, c), ("nv12", 8), 1, 2, 1, O.AVERAGE)
    assert out[0].tolist() == [[20, 23], [20, 23], [31, 34], [41, 44]] and out[1].tolist() == [[5, 8], [5, 8]]
    out = O.assemble((y, c), (y, c), (y, c), ("nv12", 8), 0, 1, 1, O.AVERAGE)
    assert out[0].tolist() == [[10, 11], [20, 22], [30, 33], [30, 33]] and out[1].tolist() == [[1, 2], [1, 2]]
    # depth 10: P010 averages word >> 6 and writes it back canonical, yuv420p10le averages word & 0x3ff
    w = np.array([[0x0040 | 63, 0xffc0], [7, 7], [0x00c0, 0xff80 | 1], [9, 9]], np.uint16)
    out = O.assemble((w,), (w,), (w,), ("nv12", 10), 0, 0, 1, O.AVERAGE)[0]
    assert out[1].tolist() == [2 << 6, 1023 << 6] and out[3].tolist() == [0x00c0, 0xff80] and out[0].tolist() == w[0].tolist()
    v = np.array([[1 | 0xfc00, 1023], [7, 7], [2, 1022], [9, 9]], np.uint16)
    out = O.assemble((v,), (v,), (v,), ("i420", 10), 0, 0, 1, O.AVERAGE)[0]
    assert out[1].tolist() == [2, 1023] and out[3].tolist() == [2, 1022] and out[0].tolist() == v[0].tolist()


def _res(sad, moving=None, match=0, combed=0):
    return {"match": match, "combed": combed, "comb": [0, 0, 0], "max_tile_comb": [0, 0, 0], "max_tile": [0, 0, 0], "dup_sad": 40 * sad,
            "dup_max_tile_sad": sad, "dup_max_tile": 0, "dup_moving_tiles": int(sad >= 1024) if moving is None else moving}


def test_oracle_schedule_drops_the_repeated_anchor_fields():
    # 3:2 top field first, anchor top: the anchor fields are A B B C D
    rs = [_res(9000 + n) for n in range(10)]
    rs[2], rs[7] = _res(3, combed=1, match=1), _res(4)
    kept, reports = O.survivors(rs, 5, 1)
    assert kept == [0, 1, 3, 4, 5, 6, 8, 9] and [r["dropped_mask"] for r in reports] == [0b00100, 0b00100]
    assert [r["combed_mask"] for r in reports] == [0b00100, 0] and reports[0]["match"] == [0, 0, 1, 0, 0]
    assert all(r["moving_dropped"] == 0 and r["still_kept"] == 0 for r in reports) and [r["first_frame"] for r in reports] == [0, 5]
    # a still stretch: equal keys, the lower frame goes; frame 0 of the stream has no key and never goes
    kept, reports = O.survivors([_res(0)] * 10, 5, 1)
    assert kept == [0, 2, 3, 4, 6, 7, 8, 9] and [r["still_kept"] for r in reports] == [3, 4]
    kept, _ = O.survivors([_res(0)] + [_res(5000)] * 4, 5, 1)
    assert kept == [0, 2, 3, 4]                                             # frame 0 has the smallest words, and stays
    # the sum decides between equal largest tiles
    a, b = _res(7), _res(7)
    b["dup_sad"] -= 1
    assert O.survivors([_res(9000), a, b, _res(9000), _res(9000)], 5, 1)[0] == [0, 1, 3, 4]
    # a wrong declaration loses moving frames, and the report says so
    kept, reports = O.survivors([_res(9000)] * 10, 5, 1)
    assert [r["moving_dropped"] for r in reports] == [1, 1]
    # a partial last cycle of m frames drops floor(m drop / cycle)
    for m, want in ((1, 0), (2, 0), (4, 0), (5, 1)):
        kept, reports = O.survivors([_res(9000 + n) for n in range(5 + m)], 5, 1)
        assert reports[-1]["n_frames"] == m and bin(reports[-1]["dropped_mask"]).count("1") == want
    assert O.survivors([_res(1)] * 4, 1, 0)[0] == [0, 1, 2, 3] and O.survivors([], 5, 1) == ([], [])


def test_oracle_match_stream_masks_the_ends():
    g = np.random.default_rng(0)
    frames = [(g.integers(0, 256, (8, 8)).astype(np.uint8),) for _ in range(3)]
    results, matched = O.match_stream(frames)
    assert results[0] == O.measure(frames[0], None, frames[1], allowed=5) and results[2] == O.measure(frames[2], frames[1], None, allowed=3)
    assert results[1] == O.measure(frames[1], frames[0], frames[2])
    assert O.match_stream(frames[:1])[0] == [O.measure(frames[0], None, None, allowed=1)]
    assert O.match_stream(frames, allowed=2)[0][0]["match"] == 0            # P alone, and no previous frame: C
    assert all(np.array_equal(m[0][0::2], f[0][0::2]) for m, f in zip(matched, frames))


# ---- the condition on the GPU test's streams -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,depth", PF.FORMATS)
@pytest.mark.parametrize("name", PF.STREAMS)
def test_the_survivors_of_every_stream_are_its_film_frames(name, layout, depth):
    """What tests/test_gpu_pulldown.py assumes of its streams, at the header's defaults: the oracle's survivors are the film frames,
    exactly and in order, none lost; only frames of true video are flagged combed.  Two exceptions, both in the streams and not in
    the defaults: the perturbed stream's survivors may carry the perturbation (one code on at most 8 luma samples of a repeated field
    instance), and the frames of true video are not film — kept as matched, they keep their anchor field."""
    frames, film, spec = PF.stream(name, layout, depth)
    assert frames[0][0].shape == (PF.H, PF.W) == (256, 448)
    results, matched = O.match_stream(frames, (layout, depth), spec["anchor"])
    kept, reports = O.survivors(results, spec["cycle"], spec["drop"])
    assert len(kept) == len(film)
    video = set(range(3, 3 + PF.N_VIDEO)) if name == "video insert" else set()
    for i, k in enumerate(kept):
        if k in video:
            assert results[k]["combed"] == 1 and all(np.array_equal(a[0::2], b[0::2]) for a, b in zip(matched[k], film[i]))
            assert all(m >= 8 * O.defaults()[1] for m in results[k]["max_tile_comb"])      # every candidate combs, far above comb_tile_min
            continue
        assert results[k]["combed"] == 0 and results[k]["max_tile_comb"][results[k]["match"]] <= 2, (k, results[k])
        if name.endswith("perturbed"):
            d = np.abs(O.S.y8(matched[k][0], layout, depth) - O.S.y8(film[i][0], layout, depth))
            assert int((d != 0).sum()) <= 8 and int(d.max()) <= 1
            assert all(np.array_equal(a, b) for a, b in zip(matched[k][1:], film[i][1:]))
        else:
            assert all(np.array_equal(a, b) for a, b in zip(matched[k], film[i])), k
    assert all(r["moving_dropped"] == 0 for r in reports)
    if name.startswith("3:2"):
        assert [r["dropped_mask"] for r in reports] == ([0b10000] * 2 if "bff" in name else [0b00100] * 2)
        assert [r["match"] for r in reports] == [[0, 0, 2, 2, 0] if "bff" in name else [0, 0, 1, 1, 0]] * 2
        dropped = [n for n in range(len(frames)) if n not in kept]
        assert all(results[n]["dup_moving_tiles"] == 0 and results[n]["dup_sad"] <= 8 for n in dropped)
        assert all(results[n]["dup_max_tile_sad"] >= O.defaults()[2] for n in kept if n)
        if name.endswith("perturbed"):
            clean = PF.stream("3:2 tff", layout, depth)[0]
            changed = [n for n in range(len(frames)) if not np.array_equal(frames[n][0], clean[n][0])]
            assert changed == [2, 4, 7, 9] and all(results[n]["dup_sad"] >= 1 for n in dropped)      # every repeated field instance is perturbed
    elif name == "2:2 shifted":
        assert [r["match"][0] for r in reports] == [0, 2, 2, 2, 2, 2, 0]
