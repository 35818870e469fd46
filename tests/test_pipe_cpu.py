"""CPU checks of the pipe API (include/fldr_pipe.h, libfldr_pipe.so): the library's symbol table and link, the header as plain C99 /
C++, the C example, the binding's struct mirror, the error strings, and the argument checks — which happen before any device call, so
they run without a GPU.  The library holds no device code (its device work is the rate library's), so there is nothing to
disassemble; a test holds that too."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest

from lib_checks import declared as _declared, syms as _syms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fldr-vfi_amd")
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "fldr_pipe.h")
LIB = os.path.join(PKG, "libfldr_pipe.so")
EXAMPLE = os.path.join(ROOT, "examples", "fldr_fps_async.c")
LINK = ["-L" + PKG, "-l:libfldr_pipe.so", "-l:libfldr_rate.so", "-l:libfldr_video.so", "-l:libfldr_model.so", "-Wl,-rpath," + PKG]


# ---- the library ------------------------------------------------------------------------------------------------------------------------
def test_library_exports_exactly_the_header():
    declared = _declared(HDR, "FLDR_PIPE_API")
    assert len(declared) == 13, sorted(declared)
    assert _syms(LIB, ["--defined-only"]) == declared
    import fldr_pipe
    assert set(fldr_pipe.EXPORTS) == declared
    for name in ("create", "destroy", "max_out", "pending", "input", "submit", "receive", "receive_view", "flush", "reset"):
        assert "fldr_pipe_" + name in declared, name


def test_library_links_only_the_rate_video_and_model_apis():
    dyn = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    assert re.search(r"NEEDED.*\[libfldr_rate\.so\]", dyn), dyn
    for other in ("hip", "shutter", "light"):
        assert not re.search(r"NEEDED.*\[libfldr_%s\.so\]" % other, dyn), dyn
    assert re.search(r"R(UN)?PATH.*\$ORIGIN", dyn), dyn
    used = set(n for n in _syms(LIB, ["--undefined-only"]) if n.startswith("fldr_"))
    allowed = (_declared(os.path.join(INC, "fldr_rate.h"), "FLDR_RATE_API") | _declared(os.path.join(INC, "fldr_video.h"), "FLDR_VIDEO_API") |
               _declared(os.path.join(INC, "fldr_model.h"), "FLDR_MODEL_API"))
    assert used and used <= allowed, sorted(used)
    # the enqueue-only entry points, and none of the synchronising converter underneath
    assert {"fldr_rate_forward", "fldr_scene_measure", "fldr_video_forward"} <= used
    assert not [n for n in used if n.startswith(("fldr_rate_push", "fldr_rate_create", "fldr_rate_flush", "fldr_video_session"))], sorted(used)


def test_the_libraries_below_know_nothing_of_the_pipe_api():
    for name in os.listdir(INC):
        if name != "fldr_pipe.h":
            assert "fldr_pipe" not in open(os.path.join(INC, name)).read().lower(), name
    for name in ("libfldr_hip.so", "libfldr_model.so", "libfldr_video.so", "libfldr_rate.so", "libfldr_shutter.so", "libfldr_light.so"):
        assert not [n for n in _syms(os.path.join(PKG, name), []) if "fldr_pipe" in n], name


def test_library_holds_no_device_code():
    """No kernel is added: the hot path is the rate library's forward between two copies.  Were there a code object, the rate
    library's disassembly checks would apply to it."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    assert KR.code_objects(LIB) == [] and KR.kernels(LIB) == []
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_pk_opsel.py"), LIB], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.parametrize("compiler", [["gcc", "-std=c99", "-x", "c"], ["g++", "-std=c++11", "-x", "c++"]])
def test_header_is_plain_c99_and_cxx(compiler, tmp_path):
    if not shutil.which(compiler[0]):
        pytest.skip(compiler[0] + " not installed")
    src = tmp_path / "h.c"
    src.write_text('#include "fldr_pipe.h"\nint main(void) { fldr_pipe_config c; c.depth = FLDR_PIPE_MAX_DEPTH;\n'
                   '  return fldr_pipe_sizeof(0) == (int)sizeof(c) && c.depth == 8 && FLDR_PIPE_E_ARG == -500 ? 0 : 1; }\n')
    r = subprocess.run(compiler + ["-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I" + INC, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "hip/" not in open(HDR).read()


def test_example_builds_with_cc(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if not cc:
        pytest.skip("no C compiler")
    exe = tmp_path / "fldr_fps_async"
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + INC, "-o", str(exe), EXAMPLE] + LINK,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    src = re.sub(r"/\*.*?\*/", "", open(EXAMPLE).read(), flags=re.S)
    assert "hip" not in src.lower()
    # no host copy of its own: the program reads into the pipe's frame and writes from its views
    assert "memcpy" not in src and "fldr_pipe_input" in src and "fldr_pipe_receive_view" in src and "fldr_pipe_submit(p, NULL)" in src
    for args in ([], ["w.npz", "64", "64", "24/0", "60"], ["w.npz", "64", "64", "24", "60", "depth=0"], ["w.npz", "64", "64", "24", "60", "depth=9"]):
        u = subprocess.run([str(exe)] + args, capture_output=True, text=True)      # usage, no device touched
        assert u.returncode == 2 and "usage" in u.stderr, args


def test_example_takes_the_command_line_of_fldr_fps_plus_a_depth():
    words = lambda path: re.search(r"usage: %s (.*?) <", open(path).read()).group(1)
    assert words(EXAMPLE) == words(os.path.join(ROOT, "examples", "fldr_fps.c")) + " [depth=N]"


def test_binding_struct_size_version_and_error_strings():
    import fldr_pipe as P
    import fldr_rate as R
    l = P.lib()
    text = open(HDR).read()
    assert l.fldr_pipe_version() == P.PIPE_VERSION == int(re.search(r"#define FLDR_PIPE_VERSION (\d+)", text).group(1)) == 100
    assert l.fldr_pipe_sizeof(0) == ctypes.sizeof(P.PipeConfig) == ctypes.sizeof(R.RateConfig) + 16
    assert l.fldr_pipe_sizeof(1) == P.E_ARG
    assert int(re.search(r"#define FLDR_PIPE_MAX_DEPTH\s+(\d+)", text).group(1)) == P.MAX_DEPTH == 8
    codes = dict((n, int(v)) for n, v in re.findall(r"#define FLDR_PIPE_E_([A-Z]+)\s+\((-?\d+)\)", text))
    assert codes == {"ARG": P.E_ARG, "FULL": P.E_FULL, "EMPTY": P.E_EMPTY, "DEVICE": P.E_DEVICE}
    for v in codes.values():
        assert v <= -500                                                       # apart from every range below
        assert l.fldr_pipe_error_string(v).decode().startswith("fldr_pipe: ") and "unknown" not in l.fldr_pipe_error_string(v).decode()
    assert "unknown" in l.fldr_pipe_error_string(-599).decode()
    assert l.fldr_pipe_error_string(0).decode() == "success"
    for v in (R.E_ARG, R.E_FORMAT, R.E_STATE, R.E_RATIO, R.E_DEVICE):          # the lower libraries' codes pass through
        assert l.fldr_pipe_error_string(v) == R.lib().fldr_rate_error_string(v) and l.fldr_pipe_error_string(v).decode().startswith("fldr_rate")
    assert l.fldr_pipe_error_string(-101).decode().startswith("fldr_video")
    assert l.fldr_pipe_error_string(-3).decode().startswith("fldr_model")
    assert l.fldr_pipe_error_string(2) == R.lib().fldr_rate_error_string(2)    # a hipError_t


# ---- argument errors without a device ---------------------------------------------------------------------------------------------------
def test_create_argument_errors_in_order_before_any_device_call():
    import fldr_pipe as P
    import fldr_rate as R
    import fldr_video as V
    l = P.lib()
    h = ctypes.c_void_p()

    def create(depth=3, **kw):
        cfg = P.pipe_config(64, 64, V.Format("i420"), 24, 60, depth)
        for k, v in kw.items():
            if k == "mutate":
                v(cfg)
            else:
                setattr(cfg.rate, k, v)
        return l.fldr_pipe_create(None, ctypes.byref(cfg), ctypes.byref(h))

    def chain(*mutations):
        """Every mutation applied at once: the code is that of the first check that fails."""
        def m(cfg):
            for f in mutations:
                f(cfg)
        return create(mutate=m)
    bad_size = lambda c: setattr(c.rate, "H", 1)
    bad_reserved = lambda c: c.rate.reserved.__setitem__(2, 1)
    bad_threshold = lambda c: setattr(c.rate.scene_params, "sad_permille", 1001)
    bad_format = lambda c: setattr(c.rate.format, "layout", 3)
    bad_ratio = lambda c: setattr(c.rate, "out_num", 0)
    bad_depth = lambda c: setattr(c, "depth", 9)
    # each alone: the rate library's own code, as fldr_rate_create returns it for the same config
    for mutate, code in ((bad_size, R.E_ARG), (bad_reserved, R.E_ARG), (bad_threshold, R.E_ARG), (bad_format, V.E_FORMAT), (bad_ratio, R.E_RATIO)):
        cfg = P.pipe_config(64, 64, V.Format("i420"), 24, 60, 3)
        mutate(cfg)
        assert l.fldr_pipe_create(None, ctypes.byref(cfg), ctypes.byref(h)) == code
        assert R.lib().fldr_rate_create(None, ctypes.byref(cfg.rate), ctypes.byref(h)) == code
    # the order: size, reserved, thresholds (all FLDR_RATE_E_ARG) before the format, the format before the ratio, the ratio before depth
    assert chain(bad_size, bad_format, bad_ratio, bad_depth) == R.E_ARG
    assert chain(bad_reserved, bad_format, bad_ratio, bad_depth) == R.E_ARG
    assert chain(bad_threshold, bad_format, bad_ratio, bad_depth) == R.E_ARG
    assert chain(bad_format, bad_ratio, bad_depth) == V.E_FORMAT
    assert chain(bad_ratio, bad_depth) == R.E_RATIO
    assert create(device=-1) == R.E_ARG and create(scene=2) == R.E_ARG and create(W=1) == R.E_ARG
    assert create(mutate=lambda c: setattr(c.rate.scene_params, "hist_permille", -1)) == R.E_ARG
    assert create(mutate=lambda c: c.rate.scene_params.reserved.__setitem__(0, 1)) == R.E_ARG
    assert create(mutate=lambda c: c.rate.format.reserved.__setitem__(4, 1)) == V.E_FORMAT
    for term in ("in_num", "in_den", "out_num", "out_den"):
        assert create(**{term: 0}) == R.E_RATIO and create(**{term: -24}) == R.E_RATIO, term
    assert create(in_num=1, out_num=65) == R.E_RATIO and create(in_num=2 ** 25 + 1, out_num=2 ** 25) == R.E_RATIO
    # then this library's: depth and its reserved words, then the model
    assert create(depth=0) == P.E_ARG and create(depth=9) == P.E_ARG and create(depth=-1) == P.E_ARG
    for i in range(3):
        assert create(mutate=lambda c: c.reserved.__setitem__(i, 1)) == P.E_ARG
    for depth in range(1, 9):
        assert create(depth=depth) == P.E_ARG                                  # valid, no model
    assert create(in_num=1, out_num=64) == P.E_ARG and create(in_num=24000, in_den=1001, out_num=120) == P.E_ARG
    assert l.fldr_pipe_create(None, None, ctypes.byref(h)) == P.E_ARG
    cfg = P.pipe_config(64, 64, V.Format("i420"), 24, 60, 3)
    assert l.fldr_pipe_create(None, ctypes.byref(cfg), None) == P.E_ARG
    assert not h.value


def test_every_entry_point_refuses_a_null_handle():
    import fldr_pipe as P
    import fldr_rate as R
    import fldr_video as V
    l = P.lib()
    n = ctypes.c_int(7)
    fr = V.Frame()
    res = R.SceneResult()
    assert l.fldr_pipe_max_out(None) == P.E_ARG and l.fldr_pipe_pending(None) == P.E_ARG
    assert l.fldr_pipe_input(None, ctypes.byref(fr)) == P.E_ARG
    assert l.fldr_pipe_submit(None, ctypes.byref(fr)) == P.E_ARG and l.fldr_pipe_submit(None, None) == P.E_ARG
    assert l.fldr_pipe_receive(None, ctypes.byref(fr), ctypes.byref(n), ctypes.byref(res)) == P.E_ARG
    assert l.fldr_pipe_receive_view(None, ctypes.byref(fr), ctypes.byref(n), ctypes.byref(res)) == P.E_ARG
    assert l.fldr_pipe_flush(None) == P.E_ARG and l.fldr_pipe_reset(None) == P.E_ARG
    l.fldr_pipe_destroy(None)
    assert n.value == 7
