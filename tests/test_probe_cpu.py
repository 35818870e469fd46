"""CPU checks of the probe API (include/fldr_probe.h, libfldr_probe.so): the library's symbol table and link, the header as plain C99 /
C++, the C example, the code-generation guards, the binding's struct mirrors, the three headers' defaults, the argument checks of the
three layers — which happen before any device call, so they run without a GPU —, the oracle (tests/probe_oracle.py) against the
pulldown and cadence oracles and on hand-worked frames, the C classifier against the oracle's, and the verdict on every stream of
tests/probe_frames.py that tests/test_gpu_probe.py relies on."""
import ctypes
import functools
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import cadence_frames as CF
import cadence_oracle as CO
import probe_frames as F
import probe_oracle as O
import pulldown_oracle as PO
from lib_checks import declared as _declared, disassemble as _disassemble, syms as _syms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fldr-vfi_amd")
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "fldr_probe.h")
LIB = os.path.join(PKG, "libfldr_probe.so")
EXAMPLE = os.path.join(ROOT, "examples", "fldr_probe.c")
BARRED = ("fldr_field", "fldr_chroma", "fldr_cadence", "fldr_repeat", "fldr_pipe", "fldr_pulldown")


# ---- the library ------------------------------------------------------------------------------------------------------------------------
def test_library_exports_exactly_the_header():
    declared = _declared(HDR, "FLDR_PROBE_API")
    assert len(declared) == 12, sorted(declared)
    assert _syms(LIB, ["--defined-only"]) == declared
    import fldr_probe
    assert set(fldr_probe.EXPORTS) == declared
    for name in ("version", "error_string", "sizeof", "measure", "frame_class", "classify", "create", "push", "verdict_get", "result_get",
                 "reset", "destroy"):
        assert "fldr_probe_" + name in declared, name


def test_library_links_only_the_rate_video_and_model_apis():
    dyn = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    needed = set(re.findall(r"NEEDED.*\[(libfldr_\w+\.so)\]", dyn))
    assert needed == {"libfldr_rate.so", "libfldr_video.so"}, dyn
    assert re.search(r"R(UN)?PATH.*\[\$ORIGIN\b", dyn), dyn
    used = set(n for n in _syms(LIB, ["--undefined-only"]) if n.startswith("fldr_"))
    allowed = (_declared(os.path.join(INC, "fldr_rate.h"), "FLDR_RATE_API") | _declared(os.path.join(INC, "fldr_video.h"), "FLDR_VIDEO_API") |
               _declared(os.path.join(INC, "fldr_model.h"), "FLDR_MODEL_API"))
    assert used and used <= allowed, sorted(used)
    assert "fldr_rate_error_string" in used and not any("create" in n for n in used)       # no model, no converter: no forward runs


def test_header_and_library_name_none_of_the_libraries_beside_them():
    text = open(HDR).read().lower()
    raw = open(LIB, "rb").read().lower()
    for other in BARRED:
        assert other not in text and other.encode() not in raw, other
    for name in os.listdir(INC):
        if name != "fldr_probe.h":
            assert "fldr_probe" not in open(os.path.join(INC, name)).read().lower(), name
    for name in os.listdir(PKG):
        if re.fullmatch(r"libfldr_\w+\.so", name) and name != "libfldr_probe.so":
            assert b"fldr_probe" not in open(os.path.join(PKG, name), "rb").read(), name


@pytest.mark.parametrize("compiler", [["gcc", "-std=c99", "-x", "c"], ["g++", "-std=c++11", "-x", "c++"]])
def test_header_is_plain_c99_and_cxx(compiler, tmp_path):
    assert shutil.which(compiler[0]), compiler[0] + " not installed"
    src = tmp_path / "h.c"
    src.write_text('#include <stddef.h>\n#include "fldr_probe.h"\nint main(void) { fldr_probe_config c; fldr_probe_verdict v; fldr_probe_params p;\n'
                   '  c.window = FLDR_PROBE_MAX_WINDOW; v.kind = FLDR_PROBE_MIXED; p.comb_thresh = FLDR_PROBE_COMB_THRESH_DEFAULT;\n'
                   '  return fldr_probe_sizeof(3) == (int)sizeof(c) && c.window == 64 && v.kind == 4 && p.comb_thresh == 6 &&\n'
                   '         FLDR_PROBE_STATE_BYTES == 16384 && sizeof(fldr_probe_result) == 256 && offsetof(fldr_probe_result, comb) == 0 &&\n'
                   '         offsetof(fldr_probe_result, lap) == 144 && sizeof(fldr_probe_verdict) == 96 && FLDR_PROBE_N == 2 ? 0 : 1; }\n')
    r = subprocess.run(compiler + ["-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I" + INC, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "hip" not in re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S).lower()


def test_header_defines_no_error_code_and_says_whose_it_returns():
    text = open(HDR).read()
    assert not re.findall(r"#define\s+FLDR_[A-Z0-9]+_E_[A-Z]+", text)
    for s in ("defines no code of its own", "FLDR_RATE_E_ARG", "FLDR_RATE_E_STATE", "FLDR_RATE_E_DEVICE",
              "fldr_probe_error_string is fldr_rate_error_string"):
        assert s in text, s
    import fldr_probe as K
    import fldr_rate as R
    l = K.lib()
    for code in (R.E_ARG, R.E_STATE, R.E_RATIO, R.E_DEVICE, -101, -3, 0, -999):
        assert l.fldr_probe_error_string(code) == R.lib().fldr_rate_error_string(code)
    assert (K.E_ARG, K.E_STATE, K.E_DEVICE) == (R.E_ARG, R.E_STATE, R.E_DEVICE)


def _define(path, name):
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, open(path).read()).group(1))


def test_the_three_headers_defaults_agree_and_the_header_says_where_they_come_from():
    pd, cd = os.path.join(INC, "fldr_pulldown.h"), os.path.join(INC, "fldr_cadence.h")
    for name in ("COMB_THRESH_DEFAULT", "COMB_TILE_DEFAULT", "TILE_SAD_DEFAULT", "TILE", "TILE_COMB_MAX", "TILE_SAD_MAX", "MAX_CYCLE"):
        assert _define(HDR, "FLDR_PROBE_" + name) == _define(pd, "FLDR_PULLDOWN_" + name), name
    assert _define(HDR, "FLDR_PROBE_FRAME_TILE_SAD_DEFAULT") == _define(cd, "FLDR_REPEAT_TILE_SAD_DEFAULT") == CO.default()
    d = O.defaults()
    assert (d["comb_thresh"], d["comb_tile_min"], d["tile_sad_min"]) == PO.defaults() == (6, 32, 1024)
    assert d["frame_tile_sad_min"] == 2048 and d["min_moved"] == 4
    text = open(HDR).read()
    for s in ("synthetic content only", "not on footage", "Validation order", "one field interval away", "three intervals away",
              "plain three-line one", "4:2:2, packed and RGB formats are out of scope"):
        assert s in text, s


def test_example_builds_with_cc(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    exe = tmp_path / "fldr_probe"
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + INC, "-o", str(exe), EXAMPLE, "-L" + PKG,
                        "-l:libfldr_probe.so", "-l:libfldr_rate.so", "-l:libfldr_video.so", "-l:libfldr_model.so", "-Wl,-rpath," + PKG],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    src = open(EXAMPLE).read()
    assert "hip" not in re.sub(r"/\*.*?\*/", "", src, flags=re.S).lower()
    for word in ("fldr_fps", "fldr_film", "cycle=%d drop=%d", "fldr_ivtc", "anchor=%s", "fldr_deint", "tff=%d"):
        assert word in src, word
    u = subprocess.run([str(exe)], capture_output=True, text=True)            # no arguments: usage, no device touched
    assert u.returncode == 2 and "usage" in u.stderr and "window=N" in u.stderr and "anchor=top|bottom" in u.stderr
    for bad in (["64", "66", "-"], ["0", "64", "-"], ["64", "64", "-", "window=2"], ["64", "64", "-", "window=65"], ["64", "64", "-", "anchor=left"],
                ["64", "64", "-", "p12"]):
        u = subprocess.run([str(exe)] + bad, capture_output=True, text=True)
        assert u.returncode == 2 and "usage" in u.stderr, bad


def test_no_unsafe_packed_fp32_in_the_probe_library():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_pk_opsel.py"), LIB], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_kernels_use_16_byte_loads_the_sad_instructions_integer_atomics_and_no_float():
    txt = "\n".join(_disassemble(LIB))
    for k in ("probe_zero_kernel", "probe_tiles_kernel", "probe_result_kernel"):
        assert k in txt, k
    assert re.search(r"\bv_sad_u8\b", txt) and re.search(r"\bv_sad_u16\b", txt)
    assert re.search(r"\bglobal_atomic_umax_x2\b", txt) and re.search(r"\bglobal_atomic_add_x2\b", txt)   # the 64-bit keys and sums
    assert re.search(r"\bglobal_load_dwordx4\b", txt)                                                      # 16 bytes per lane
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
    import fldr_probe as K
    l = K.lib()
    text = open(HDR).read()
    assert l.fldr_probe_version() == K.PROBE_VERSION == int(re.search(r"#define FLDR_PROBE_VERSION (\d+)", text).group(1)) == 100
    for which, cls in enumerate((K.Params, K.Result, K.Verdict, K.ProbeConfig)):
        assert l.fldr_probe_sizeof(which) == ctypes.sizeof(cls)
    assert ctypes.sizeof(K.Params) == 48 and ctypes.sizeof(K.Result) == 256 and ctypes.sizeof(K.Verdict) == 96
    assert K.Result.comb.offset == 0 and K.Result.field_sad.offset == 96 and K.Result.lap.offset == 144 and K.Result.tff_sum.offset == 192
    assert l.fldr_probe_sizeof(4) == K.E_ARG and l.fldr_probe_sizeof(-1) == K.E_ARG
    for macro, v in (("STATE_BYTES", K.STATE_BYTES), ("MAX_CYCLE", K.MAX_CYCLE), ("TILE", K.TILE), ("TILE_COMB_MAX", K.TILE_COMB_MAX),
                     ("TILE_SAD_MAX", K.TILE_SAD_MAX), ("FRAME_TILE_SAD_MAX", K.FRAME_TILE_SAD_MAX), ("COMB_THRESH_DEFAULT", K.COMB_THRESH_DEFAULT),
                     ("COMB_TILE_DEFAULT", K.COMB_TILE_DEFAULT), ("TILE_SAD_DEFAULT", K.TILE_SAD_DEFAULT),
                     ("FRAME_TILE_SAD_DEFAULT", K.FRAME_TILE_SAD_DEFAULT), ("MIN_MOVED_DEFAULT", K.MIN_MOVED_DEFAULT), ("C", K.C), ("P", K.P),
                     ("N", K.N), ("MIN_WINDOW", K.MIN_WINDOW), ("MAX_WINDOW", K.MAX_WINDOW), ("UNKNOWN", K.UNKNOWN), ("PROGRESSIVE", K.PROGRESSIVE),
                     ("FILM", K.FILM), ("INTERLACED", K.INTERLACED), ("MIXED", K.MIXED), ("FRAME_STILL", K.FRAME_STILL), ("FRAME_PROG", K.FRAME_PROG),
                     ("FRAME_FILM", K.FRAME_FILM), ("FRAME_VIDEO", K.FRAME_VIDEO)):
        assert _define(HDR, "FLDR_PROBE_" + macro) == v, macro
    assert (K.UNKNOWN, K.PROGRESSIVE, K.FILM, K.INTERLACED, K.MIXED) == (O.UNKNOWN, O.PROGRESSIVE, O.FILM, O.INTERLACED, O.MIXED)
    assert (K.FRAME_STILL, K.FRAME_PROG, K.FRAME_FILM, K.FRAME_VIDEO) == (O.STILL, O.F_PROG, O.F_FILM, O.F_VIDEO)
    assert K.RESULT_KEYS == O.KEYS and K.VERDICT_KEYS == O.VERDICT_KEYS and K.MAX_CYCLE == O.MAX_CYCLE


# ---- argument errors without a device ---------------------------------------------------------------------------------------------------
H0 = W0 = 64


def _host(V, layout, depth, H=H0, W=W0, count=3):
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


BAD_PARAMS = (dict(comb_thresh=-1), dict(comb_thresh=256), dict(comb_tile_min=-1), dict(comb_tile_min=513), dict(tile_sad_min=-1),
              dict(tile_sad_min=130561), dict(frame_tile_sad_min=-1), dict(frame_tile_sad_min=261121), dict(min_moved=-1), dict(min_moved=65),
              dict(max_outliers=-1), dict(max_outliers=65), dict(anchor=2), dict(anchor=-1))
GOOD_PARAMS = (dict(comb_thresh=255), dict(comb_thresh=1), dict(comb_tile_min=512), dict(tile_sad_min=130560), dict(frame_tile_sad_min=261120),
               dict(min_moved=64), dict(max_outliers=64), dict(anchor=1))


@pytest.mark.parametrize("layout", ["nv12", "i420"])
@pytest.mark.parametrize("depth", [8, 10])
def test_measure_argument_errors_before_any_device_call(layout, depth):
    import fldr_probe as K
    import fldr_video as V
    b = 2 if depth == 10 else 1
    buf, base, _ = _host(V, layout, depth)
    shapes = V.plane_shapes(layout, H0, W0)
    state = base + 3 * H0 * W0 * 2 * b

    def call(mutate=lambda fr, fmt: None, params=None, state=state, H=H0, W=W0, prev=True, nxt=True, cur=True, which=2):
        _, _, fr = _host(V, layout, depth)
        fmt = V.Format(layout, depth=depth)
        mutate(fr[which], fmt)
        return K.measure_raw(H, W, fmt, fr[0] if cur else None, fr[1] if prev else None, fr[2] if nxt else None, params, state, None)
    # a valid call is shown to pass every check by reaching the last one, the state
    assert call(state=None) == K.E_STATE
    assert call(state=base + 128) == K.E_STATE and call(state=base + 16) == K.E_STATE
    for H in (0, -4, 2, 6, 62, 65, 2 ** 31 - 4):                           # at least 4, a multiple of 4, whole tiles inside 32 bits
        assert call(H=H) == K.E_ARG, H
    assert call(W=0) == K.E_ARG and call(W=-1) == K.E_ARG and call(H=4, W=2 ** 31 - 1) == K.E_ARG
    assert call(cur=False) == K.E_ARG
    assert K.measure_raw(H0, W0, None, _host(V, layout, depth)[2][0], None, None, None, state, None) == K.E_ARG
    for bad in BAD_PARAMS:
        assert call(params=K.Params(**bad)) == K.E_ARG, bad
    for ok in GOOD_PARAMS:
        assert call(params=K.Params(**ok), state=None) == K.E_STATE, ok
    for i in range(5):
        p = K.Params()
        p.reserved[i] = 1
        assert call(params=p) == K.E_ARG
    # prev and next may each be NULL
    assert call(prev=False, state=None) == K.E_STATE and call(nxt=False, state=None) == K.E_STATE and call(prev=False, nxt=False, state=None) == K.E_STATE
    # the stated order: size, parameters, format, planes, pitches, state
    assert call(lambda fr, fmt: setattr(fmt, "layout", 2), params=K.Params(comb_thresh=-1), H=6) == K.E_ARG
    assert call(lambda fr, fmt: setattr(fmt, "layout", 2), params=K.Params(comb_thresh=-1)) == K.E_ARG
    assert call(lambda fr, fmt: (setattr(fmt, "layout", 2), fr.plane.__setitem__(0, None)), state=None) == V.E_FORMAT
    assert call(lambda fr, fmt: (fr.plane.__setitem__(0, None), fr.pitch.__setitem__(0, 1)), state=None) == V.E_PLANE
    assert call(lambda fr, fmt: fr.pitch.__setitem__(0, 2), state=None) == V.E_PITCH
    # a missing plane of the LAST frame is reported before a short pitch of the first
    _, _, fr = _host(V, layout, depth)
    fr[0].pitch[0] = 2
    fr[2].plane[0] = None
    assert K.measure_raw(H0, W0, V.Format(layout, depth=depth), fr[0], fr[1], fr[2], None, state, None) == V.E_PLANE
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


def test_classify_and_stream_argument_errors_before_any_device_call():
    import fldr_probe as K
    import fldr_video as V
    l = K.lib()
    one, v = (K.Result * 1)(), K.Verdict()
    assert K.classify_raw(one, 1, None, v) == 0 and K.classify_raw(None, 0, None, v) == 0 and v.kind == K.UNKNOWN and v.n_frames == 0
    assert K.classify_raw(None, 1, None, v) == K.E_ARG and K.classify_raw(one, -1, None, v) == K.E_ARG and K.classify_raw(one, 1, None, None) == K.E_ARG
    for bad in BAD_PARAMS:
        assert K.classify_raw(one, 1, K.Params(**bad), v) == K.E_ARG, bad
        assert l.fldr_probe_frame_class(one, ctypes.byref(K.Params(**bad))) == K.E_ARG
    for ok in GOOD_PARAMS:
        assert K.classify_raw(one, 1, K.Params(**ok), v) == 0, ok
    assert l.fldr_probe_frame_class(None, None) == K.E_ARG and l.fldr_probe_frame_class(one, None) == K.FRAME_STILL
    # the stream: everything before the device.  A configuration that passes every check is seen to by asking for a device that cannot exist.
    h = ctypes.c_void_p()

    def create(mutate=lambda c: None, **kw):
        args = dict(H=64, W=64, fmt=V.Format("i420"), window=8, device=2 ** 20)
        args.update(kw)
        cfg = K.make_config(**args)
        mutate(cfg)
        return l.fldr_probe_create(ctypes.byref(cfg), ctypes.byref(h))
    assert l.fldr_probe_create(None, ctypes.byref(h)) == K.E_ARG and l.fldr_probe_create(ctypes.byref(K.make_config(64, 64, V.Format())), None) == K.E_ARG
    for H in (0, 2, 62, 66, -4):
        assert create(H=H) == K.E_ARG, H
    assert create(W=0) == K.E_ARG and create(device=-1) == K.E_ARG
    for w in (0, 2, 65, -1):
        assert create(window=w) == K.E_ARG, w
    for bad in BAD_PARAMS:
        assert create(params=K.Params(**bad)) == K.E_ARG, bad
    assert create(mutate=lambda c: c.params.reserved.__setitem__(4, 1)) == K.E_ARG
    assert create(mutate=lambda c: c.reserved.__setitem__(3, 1)) == K.E_ARG
    assert create(mutate=lambda c: setattr(c.format, "layout", 3)) == V.E_FORMAT
    assert create(mutate=lambda c: setattr(c.format, "layout", 3), window=2) == K.E_ARG       # the order: the window before the format
    assert not h.value
    assert l.fldr_probe_push(None, None) == K.E_ARG and l.fldr_probe_verdict_get(None, None) == K.E_ARG
    assert l.fldr_probe_result_get(None, 0, None, None) == K.E_ARG and l.fldr_probe_reset(None) == K.E_ARG
    l.fldr_probe_destroy(None)


@pytest.mark.parametrize("layout,depth", [("nv12", 8), ("i420", 10)])
def test_two_faults_at_once_answer_in_the_recorded_order(layout, depth):
    """The checks of a measure sit in a header this library shares with the cadence and pulldown libraries (rate/tile_measure_host.h):
    which of two simultaneous faults is reported is decided there.  Every code here was recorded from the library as it was before
    that text was shared."""
    import fldr_probe as K
    import fldr_video as V
    b = 2 if depth == 10 else 1
    buf, base, fr = _host(V, layout, depth)
    state = base + 3 * H0 * W0 * 2 * b
    fmt, bad_fmt = V.Format(layout, depth=depth), V.Format(layout, depth=depth)
    bad_fmt.layout = 2
    assert K.measure_raw(H0, W0, fmt, fr[0], fr[1], fr[2], K.Params(comb_thresh=-1), state + 16, None) == K.E_ARG   # a bad parameter and a misaligned state
    assert K.measure_raw(6, W0, fmt, fr[0], fr[1], fr[2], None, None, None) == K.E_ARG                              # a bad size and no state
    assert K.measure_raw(H0, W0, bad_fmt, fr[0], fr[1], fr[2], None, state + 16, None) == V.E_FORMAT
    fr[1].pitch[0] = 2
    assert K.measure_raw(H0, W0, fmt, fr[0], fr[1], fr[2], None, state + 16, None) == V.E_PITCH
    _, _, fr = _host(V, layout, depth)
    fr[0].pitch[1], fr[1].plane[1] = 2, None                                 # every plane of every frame before any pitch
    assert K.measure_raw(H0, W0, fmt, fr[0], fr[1], fr[2], None, state, None) == V.E_PLANE
    # the stream: size, window, parameters and reserved words all come before the format
    l, h = K.lib(), ctypes.c_void_p()

    def create(mutate):
        cfg = K.make_config(64, 64, V.Format("i420"), 8, 2 ** 20)
        cfg.format.layout = 3
        mutate(cfg)
        return l.fldr_probe_create(ctypes.byref(cfg), ctypes.byref(h))
    assert create(lambda c: None) == V.E_FORMAT
    assert create(lambda c: setattr(c, "H", 6)) == K.E_ARG and create(lambda c: setattr(c.params, "min_moved", 65)) == K.E_ARG
    assert create(lambda c: c.reserved.__setitem__(0, 1)) == K.E_ARG
    assert not buf.any() and not h.value


# ---- the oracle against its siblings and on hand-worked frames ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _measures(name, layout, depth):
    frames, _ = F.stream(name, layout, depth)
    return O.measure_stream(frames, (layout, depth))


@pytest.mark.parametrize("layout,depth", F.FORMATS)
@pytest.mark.parametrize("name", ["3:2 tff", "video insert", "video bff"])
def test_oracle_comb_and_field_words_are_the_pulldown_oracles_at_both_anchors(name, layout, depth):
    frames, _ = F.stream(name, layout, depth)
    for n, r in zip(range(1, len(frames) - 1), _measures(name, layout, depth)):
        for q in (0, 1):
            p = PO.measure(frames[n], frames[n - 1], frames[n + 1], (layout, depth), q)
            assert (r["comb"][q], r["max_tile_comb"][q], r["max_tile"][q]) == (p["comb"], p["max_tile_comb"], p["max_tile"]), (n, q)
            assert (r["field_sad"][q], r["field_max_tile_sad"][q], r["field_max_tile"][q], r["field_moving_tiles"][q]) == \
                   (p["dup_sad"], p["dup_max_tile_sad"], p["dup_max_tile"], p["dup_moving_tiles"]), (n, q)
    # non-default thresholds go the same way, and a missing frame's words are zero
    r = O.measure(frames[2], None, frames[3], (layout, depth), comb_thresh=20, tile_sad_min=5000)
    p = PO.measure(frames[2], None, frames[3], (layout, depth), 1, comb_thresh=20, tile_sad_min=5000, allowed=5)
    assert r["comb"][1] == p["comb"] and r["comb"][1][1] == 0 and r["field_sad"] == [0, 0] and r["repeat"] == 0 and r["lap"][1] == [0, 0]
    assert r["tff_sum"] == r["bff_sum"] == 0 and r["lap"][0][0] > 0 and r["lap"][2][0] > 0
    r = O.measure(frames[2], frames[1], None, (layout, depth))
    assert r["lap"][2] == [0, 0] and r["tff_sum"] == r["bff_sum"] == 0 and sum(r["field_sad"]) > 0 and all(r["comb"][q][2] == 0 for q in (0, 1))


@pytest.mark.parametrize("layout,depth", F.FORMATS)
@pytest.mark.parametrize("pattern", sorted(CF.PATTERNS))
def test_oracle_repeat_is_the_cadence_oracles(pattern, layout, depth):
    frames, source = CF.stream(pattern, layout, depth, F.N_CADENCE)
    want = CF.measures(frames, layout, depth)
    for n, r in zip(range(1, len(frames) - 1), _measures("repeats " + pattern, layout, depth)):
        assert (r["repeat"], r["frame_moving_tiles"], sum(r["field_sad"])) == (want[n]["repeat"], want[n]["moving_tiles"], want[n]["sad"]), n
        assert r["repeat"] == int(source[n][1] > 0)                            # a repeat is a later instance of a real frame
    # with equal thresholds, at another value too
    r = O.measure(frames[2], frames[1], frames[3], (layout, depth), frame_tile_sad_min=30000)
    assert r["frame_moving_tiles"] == CO.measure(frames[1], frames[2], (layout, depth), 30000)["moving_tiles"]


def _frame(rows):
    return (np.array(rows, np.uint8),)


def test_oracle_order_sums_on_hand_worked_frames():
    # 8 x 8: cur is flat 50 but for row 3 (100).  lap of C: row 2 and row 4 see one neighbour at 100: |50 + 100 - 100| = 50 per sample,
    # row 3 sees |50 + 50 - 200| = 100 per sample; rows 0 and 7 never count
    cur = np.full((8, 8), 50, np.uint8)
    cur[3] = 100
    r = O.measure((cur,), None, None)
    assert r["lap"][0] == [2 * 8 * 50, 8 * 100] and r["lap"][1] == r["lap"][2] == [0, 0] and r["tff_sum"] == r["bff_sum"] == 0
    # prev differs from cur on row 0 and row 7 only: excluded rows, so lap[P] is lap[C]; next differs on row 1 (odd) by 7 on 3 samples
    prev, nxt = cur.copy(), cur.copy()
    prev[0] = 0
    prev[7] = 255
    nxt[1, :3] += 7
    r = O.measure((cur,), (prev,), (nxt,))
    assert r["lap"][1] == r["lap"][0] == [800, 800]
    assert r["lap"][2] == [800, 800 + 3 * 14]                                   # |50 + 50 - 2 x 57| = 14
    assert r["tff_sum"] == r["lap"][1][1] + r["lap"][2][0] == 1600 and r["bff_sum"] == r["lap"][1][0] + r["lap"][2][1] == 1642
    # the largest word: rows alternating 0 and 255 in cur: |0 + 0 - 510| on odd rows, |255 + 255 - 0| on even; the inverse frame's rows equal
    # the lines of cur around them: nothing
    stripes = np.zeros((8, 8), np.uint8)
    stripes[1::2] = 255
    inv = 255 - stripes
    r = O.measure((stripes,), (stripes,), (inv,))
    assert r["lap"][0] == r["lap"][1] == [3 * 8 * 510, 3 * 8 * 510] and r["lap"][2] == [0, 0]      # rows 2, 4, 6 and 1, 3, 5
    assert r["comb"][0][0] == r["comb"][1][0] == 24 and r["comb"][0][2] == r["comb"][1][2] == 0
    # depth 10: P010 reads word >> 8, yuv420p10le (word & 0x3ff) >> 2; the other bits are ignored
    w = np.array([[0x1200] * 2, [0x19ff, 0x18ff], [0x12ff] * 2, [0] * 2], np.uint16)       # y8: 0x12, (0x19, 0x18), 0x12, 0
    assert O.measure((w,), None, None, ("nv12", 10))["lap"][0] == [11 + 12, 14 + 12]     # row 2: |25 + 0 - 36|, |24 + 0 - 36|; row 1: |36 - 50|, |36 - 48|
    v = np.array([[0x48 | 0xfc00] * 2, [0x67, 0x60], [0x4b] * 2, [0] * 2], np.uint16)      # the same y8
    assert O.measure((v,), None, None, ("i420", 10))["lap"][0] == O.measure((w,), None, None, ("nv12", 10))["lap"][0]


# ---- the classifier: the C function against the oracle's -----------------------------------------------------------------------------------
def _both(results, **params):
    import fldr_probe as K
    want = O.classify(results, **params)
    got = K.classify(results, K.Params(**params) if params else None)
    assert got == want, (got, want)
    for r in results:
        assert K.frame_class(r, K.Params(**params) if params else None) == O.frame_class(r, **params)
    return got


def _res(moved=1, c=(0, 0), p=(0, 0), n=(0, 0), tff=0, bff=0, field=(1, 1)):
    """A hand-made result: frame_moving_tiles, max_tile_comb[q][k] by candidate, the order sums, field_moving_tiles."""
    r = {k: 0 for k in O.KEYS}
    r.update(comb=[[0] * 3, [0] * 3], max_tile=[[0] * 3, [0] * 3], field_sad=[0, 0], field_max_tile_sad=[0, 0], field_max_tile=[0, 0],
             lap=[[0, 0] for _ in range(3)])
    r.update(max_tile_comb=[[c[0], p[0], n[0]], [c[1], p[1], n[1]]], frame_moving_tiles=moved, repeat=int(not moved), tff_sum=tff, bff_sum=bff,
             field_moving_tiles=list(field))
    return r


PROG, STILL = _res(), _res(moved=0, field=(0, 0))
FILM_P = _res(c=(300, 300), p=(0, 300), n=(300, 0))            # clean with prev for one anchor, with next for the other
VID_T, VID_B, VID_0 = (_res(c=(300, 300), p=(300, 300), n=(300, 300), tff=t, bff=b) for t, b in ((10, 20), (20, 10), (15, 15)))


@pytest.mark.parametrize("layout,depth", F.FORMATS)
@pytest.mark.parametrize("name", F.STREAMS)
def test_the_verdict_on_every_stream(name, layout, depth):
    """What tests/test_gpu_probe.py assumes of its streams, at the header's defaults with max_outliers 0: the expected verdict, from
    the oracle and from fldr_probe_classify alike."""
    _, want = F.stream(name, layout, depth)
    got = _both(_measures(name, layout, depth))
    assert {k: got[k] for k in want} == want, got
    assert got["irregular"] == 0 and got["n_frames"] == len(F.stream(name, layout, depth)[0]) - 2
    if name.startswith("video") and name != "video insert":
        # the margins of the order measure: every candidate of every frame combs far above the threshold, and the two sums differ widely
        for r in _measures(name, layout, depth):
            assert min(min(r["max_tile_comb"][q]) for q in (0, 1)) >= 4 * O.defaults()["comb_tile_min"]
            lo, hi = sorted((r["tff_sum"], r["bff_sum"]))
            assert 4 * lo < 3 * hi
    if name == "3:2 tff":
        assert [r["field_moving_tiles"][0] == 0 for r in _measures(name, layout, depth)] == [False, True, False, False, False, False, True, False]
        assert _both(_measures(name, layout, depth), anchor=1)["drop"] == 1


def test_classifier_on_seeded_random_results():
    g = np.random.default_rng(7)
    kinds = set()
    for trial in range(300):
        M = int(g.integers(0, 24))
        pool = [PROG, STILL, FILM_P, VID_T, VID_B, VID_0]
        weights = g.dirichlet(np.full(len(pool), 0.3))
        rs = []
        for _ in range(M):
            r = dict(pool[int(g.choice(len(pool), p=weights))])
            if g.random() < 0.3:
                r = _res(moved=int(g.integers(0, 3)), c=tuple(g.integers(0, 64, 2)), p=tuple(g.integers(0, 64, 2)), n=tuple(g.integers(0, 64, 2)),
                         tff=int(g.integers(0, 3)), bff=int(g.integers(0, 3)), field=tuple(g.integers(0, 2, 2)))
            rs.append(r)
        params = {} if trial % 3 == 0 else dict(comb_tile_min=int(g.integers(1, 64)), min_moved=int(g.integers(1, 8)), max_outliers=int(g.integers(0, 3)),
                                                 anchor=int(g.integers(0, 2)))
        kinds.add(_both(rs, **params)["kind"])
    assert kinds == {O.UNKNOWN, O.PROGRESSIVE, O.FILM, O.INTERLACED, O.MIXED}


def test_classifier_edge_cases():
    # fewer than min_moved moved frames
    assert _both([PROG] * 3 + [STILL] * 9)["kind"] == O.UNKNOWN and _both([PROG] * 4 + [STILL] * 9)["kind"] == O.PROGRESSIVE
    assert _both([PROG] * 3, min_moved=3)["kind"] == O.PROGRESSIVE and _both([], min_moved=1)["kind"] == O.UNKNOWN
    # a vote tie, with and without silent frames
    v = _both([VID_T, VID_B, VID_T, VID_B])
    assert (v["kind"], v["tff"], v["votes_tff"], v["votes_bff"]) == (O.INTERLACED, -1, 2, 2)
    v = _both([VID_T, VID_0, VID_0, VID_0, VID_B, VID_B])
    assert (v["tff"], v["votes_tff"], v["votes_bff"], v["n_video"]) == (0, 1, 2, 6)
    assert _both([VID_0] * 4)["tff"] == -1 and _both([VID_T] * 4 + [PROG])["mixed"] == 1
    # an all-zero r: 1, 0, nothing confirmed, not irregular
    v = _both([PROG] * 6)
    assert (v["cycle"], v["drop"], v["irregular"], v["confirmed"]) == (1, 0, 0, 0)
    # a non-periodic r: 1, 0, irregular
    v = _both([STILL] + [PROG] * 9)                                        # r[0] is never seen again
    assert (v["kind"], v["cycle"], v["drop"], v["irregular"], v["confirmed"]) == (O.PROGRESSIVE, 1, 0, 1, 0)
    # a period as long as the window is not seen (c < M), one of 16 is, one of 17 is not
    assert _both(([STILL] + [PROG] * 4) * 1)["irregular"] == 1
    v = _both(([STILL] + [PROG] * 15) * 2)
    assert (v["cycle"], v["drop"], v["confirmed"]) == (16, 1, 1)
    assert _both(([STILL] + [PROG] * 16) * 2)["irregular"] == 1
    # film: r comes from the anchor's field
    film = [_res(c=(300, 300), p=(0, 300), n=(300, 0), field=f) for f in ((1, 1), (0, 1), (1, 1), (1, 0), (1, 1))] * 2
    v0, v1 = _both(film), _both(film, anchor=1)
    assert (v0["kind"], v0["cycle"], v0["drop"], v0["anchor"], v0["confirmed"]) == (O.FILM, 5, 1, 0, 1) and (v1["cycle"], v1["drop"], v1["anchor"]) == (5, 1, 1)
    # max_outliers on either side of its threshold: two video frames among film
    rs = film + [VID_T, VID_T]
    assert _both(rs)["kind"] == O.MIXED and _both(rs, max_outliers=1)["kind"] == O.MIXED
    v = _both(rs, max_outliers=2)
    assert (v["kind"], v["n_video"], v["n_film"]) == (O.FILM, 2, 10)
    # ... and progressive outliers among video do not make it mixed
    rs = [VID_T] * 6 + [PROG]
    assert _both(rs)["mixed"] == 1 and _both(rs, max_outliers=1)["mixed"] == 0
    # every class an outlier: nothing left is progressive by the rule, whatever was counted
    assert _both([VID_T, FILM_P, PROG, PROG], max_outliers=2)["kind"] == O.PROGRESSIVE
    # comb_tile_min is exclusive below: a tile of exactly comb_tile_min combs
    edge = _res(c=(32, 0))
    assert _both([edge] * 4)["n_prog"] == 0 and _both([edge] * 4, comb_tile_min=33)["n_prog"] == 4
