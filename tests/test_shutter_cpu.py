"""CPU checks of the shutter API (include/fldr_shutter.h, libfldr_shutter.so): the window rule and the cut rule against the exact
rationals of tests/shutter_oracle.py, the reciprocal resolve divides with over every total, the library's symbol table and link, the
header as plain C99 / C++, the C example, the code-generation guards, the binding's struct mirrors, and the argument checks — which
happen before any device call, so they run without a GPU."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import shutter_oracle as SO
from lib_checks import declared as _declared, disassemble as _disassemble, syms as _syms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fldr-vfi_amd")
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "fldr_shutter.h")
LIB = os.path.join(PKG, "libfldr_shutter.so")

RATES = [(120, 24), (60, 24), ((60000, 1001), (24000, 1001)), (50, 25), (24, 60)]
SHUTTERS = [(1, 4), (1, 2), (1, 1)]
SUBS = [1, 2, 4, 8, 64]


def _valid(in_rate, out_rate, shutter, sub):
    """Whether a window can hold no grid point: s A sub < B, what create refuses."""
    q = SO._rate(in_rate) / SO._rate(out_rate)
    return SO._rate(shutter) * q * sub >= 1


# ---- the window rule ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("shutter", SHUTTERS)
@pytest.mark.parametrize("in_rate,out_rate", RATES)
def test_plan_is_the_rational_window_rule(in_rate, out_rate, shutter, sub):
    import fldr_rate
    import fldr_shutter as T
    cfg = T.config(in_rate, out_rate, shutter, sub)
    f, l = ctypes.c_int64(), ctypes.c_int64()
    rc = T.lib().fldr_shutter_plan(ctypes.byref(cfg), 0, ctypes.byref(f), ctypes.byref(l))
    if not _valid(in_rate, out_rate, shutter, sub):
        assert rc == T.E_RATIO                                      # a window that could hold no grid point
        return
    assert rc == 0
    N = 300
    q = SO._rate(in_rate) / SO._rate(out_rate)
    n_out = int((N - 1) / q) + 1                                    # the j with j A / B <= N - 1
    assert n_out == sum(len(p) for p in fldr_rate.schedule(N, in_rate, out_rate))
    prev_last = -1
    for j in range(n_out):
        got = T.plan(cfg, j)
        assert got == SO.window(j, in_rate, out_rate, shutter, sub), j
        first, last = got
        assert first <= last, "an empty window"
        assert first > prev_last, "windows overlap"
        assert Fraction(first, sub) >= j * q and Fraction(first - 1, sub) < j * q          # begins at the frame's own time
        assert Fraction(last, sub) < (j + SO._rate(shutter)) * q <= Fraction(last + 1, sub)
        prev_last = last
    assert T.plan(cfg, n_out)[0] > (N - 1) * sub                    # the next window begins behind the last frame
    # a large j: the products leave 64 bits, the rule stays exact
    big = 10 ** 12
    assert T.plan(cfg, big) == SO.window(big, in_rate, out_rate, shutter, sub)


def test_plan_small_cases():
    import fldr_shutter as T
    c = T.config(120, 24, (1, 2), 1)                                # frames 5 j .. 5 j + 2 (2.5 intervals: the points 5 j, +1, +2)
    assert [T.plan(c, j) for j in range(3)] == [(0, 2), (5, 7), (10, 12)]
    c = T.config(120, 24, 1, 1)
    assert [T.plan(c, j) for j in range(3)] == [(0, 4), (5, 9), (10, 14)]
    c = T.config(60, 24, (1, 2), 4)                                 # 2.5 intervals apart, 1.25 long: grid 10 j .. 10 j + 4
    assert [T.plan(c, j) for j in range(3)] == [(0, 4), (10, 14), (20, 24)]
    c = T.config(24, 60, 1, 8)                                      # 0.4 intervals apart and long: grid 3.2 j .. 3.2 (j + 1)
    assert [T.plan(c, j) for j in range(5)] == [(0, 3), (4, 6), (7, 9), (10, 12), (13, 15)]


@pytest.mark.parametrize("in_rate,out_rate,shutter,sub", [(120, 24, (1, 2), 1), (60, 24, (1, 2), 4), (24, 60, 1, 8), (50, 25, 1, 2),
                                                           ((60000, 1001), (24000, 1001), (1, 2), 8)])
@pytest.mark.parametrize("cuts", [(), (6,), (1,), (5, 6), (3, 9, 10)])
def test_schedule_follows_the_cut_rule(in_rate, out_rate, shutter, sub, cuts):
    """fldr_shutter.schedule (the library's windows + the header's push rule, as the converter plans) against the point-by-point
    statement of the oracle with injected cut flags."""
    import fldr_rate
    import fldr_shutter as T
    N = 14
    sched = T.schedule(N, in_rate, out_rate, shutter, sub, cuts)
    want = SO.outputs(N, in_rate, out_rate, shutter, sub, cuts)
    assert len(sched) == N + 1
    got = [dict(o, push=n) for n, push in enumerate(sched) for o in push]
    assert got == want
    assert [o["j"] for o in got] == list(range(len(got)))
    assert len(got) == sum(len(p) for p in fldr_rate.schedule(N, in_rate, out_rate))     # the count fldr_rate returns
    assert max(len(p) for p in sched) <= T.max_out(in_rate, out_rate)
    scene_of_frame = lambda i: sum(1 for c in cuts if c <= i)
    for o in got:
        assert o["points"], "an output without a point"
        # no output mixes two scenes: every frame it takes samples from lies in one
        frames = set()
        for i, k, src in o["points"]:
            if k == 0:
                frames.add(i)
            elif src is not None:
                frames.add(src)
            else:
                assert (i + 1) not in cuts, "an interpolation across a cut"
                frames.update((i, i + 1))
        assert len(set(scene_of_frame(i) for i in frames)) == 1, o
    if not cuts:
        assert all(not o["truncated"] for o in got if o["push"] < N)


def test_schedule_small_cases():
    import fldr_shutter as T
    s = T.schedule(11, 120, 24, 1, 1)                               # whole-interval exposure: five frames each
    assert [[o["j"] for o in p] for p in s] == [[], [], [], [], [0], [], [], [], [], [1], [], [2]]
    assert [i for i, k, src in s[4][0]["points"]] == [0, 1, 2, 3, 4] and not s[4][0]["truncated"]
    assert s[11][0]["points"] == [(10, 0, None)] and s[11][0]["truncated"]           # the flush: what exists of 10 .. 14
    s = T.schedule(11, 120, 24, 1, 1, cuts=(3,))                    # a cut between frames 2 and 3: output 0 holds 0, 1, 2 only
    assert [[o["j"] for o in p] for p in s][:5] == [[], [], [], [0], []]
    assert s[3][0]["points"] == [(0, 0, None), (1, 0, None), (2, 0, None)] and s[3][0]["truncated"]
    assert [i for i, k, src in s[9][0]["points"]] == [5, 6, 7, 8, 9]
    s = T.schedule(4, 60, 24, (1, 2), 4, cuts=(1,))                 # grid 0 .. 4 of a cut pair: 0 and the k = 1 point are frame 0's scene
    assert s[1][0]["points"] == [(0, 0, None), (0, 1, 0)] and s[1][0]["truncated"]


# ---- the reciprocal ---------------------------------------------------------------------------------------------------------------------
def test_reciprocal_equals_the_division_for_every_total():
    """x // (2 total) == ((x * mul) >> 32) >> shift for every total and every x <= 2047 total (x = 2 acc + total, acc <= 1023 total).
    Both sides are monotone step functions of x; the division steps exactly at the multiples of 2 total, so agreement at q d - 1 and
    q d for every quotient q up to the largest (and at the largest x) is agreement everywhere."""
    import fldr_shutter as T
    totals = np.arange(1, 65536, dtype=np.uint64)
    mul = np.empty(65535, np.uint64)
    shift = np.empty(65535, np.uint64)
    for i, t in enumerate(totals):
        m, s = T.reciprocal(int(t))
        assert m < 2 ** 32 and s < 32
        mul[i], shift[i] = m, s
    d = 2 * totals
    xmax = 2047 * totals
    for q in range(0, 1025):
        for x in (np.uint64(q) * d, np.maximum(np.uint64(q) * d, np.uint64(1)) - np.uint64(1), xmax):
            x = np.minimum(x, xmax)
            assert x.max() < 2 ** 32
            got = ((x * mul) >> np.uint64(32)) >> shift
            assert np.array_equal(got, x // d), q
    assert T.lib().fldr_shutter_reciprocal(0, ctypes.byref(ctypes.c_uint32()), ctypes.byref(ctypes.c_uint32())) == T.E_WEIGHT
    assert T.lib().fldr_shutter_reciprocal(65536, ctypes.byref(ctypes.c_uint32()), ctypes.byref(ctypes.c_uint32())) == T.E_WEIGHT
    assert T.lib().fldr_shutter_reciprocal(1, None, None) == T.E_ARG


def test_oracle_on_hand_worked_samples():
    a = np.array([[0, 10, 255]], np.uint8)
    b = np.array([[1, 11, 255]], np.uint8)
    assert SO.mix([(a,), (b,)], [1, 1], "nv12", 8)[0].tolist() == [[1, 11, 255]]          # halves round up
    assert SO.mix([(a,), (b,)], [3, 1], "nv12", 8)[0].tolist() == [[0, 10, 255]]          # 1 / 4 rounds down
    w = np.array([[0xffff, 0x0040 | 0x3f]], np.uint16)
    assert SO.value(w, "nv12", 10).tolist() == [[1023, 1]] and SO.value(w, "i420", 10).tolist() == [[1023, 0x7f]]
    assert SO.mix([(w,)], [7], "nv12", 10)[0].tolist() == [[1023 << 6, 1 << 6]]           # low six bits written as zero
    assert SO.mix([(w,)], [7], "i420", 10)[0].tolist() == [[1023, 0x7f]]                  # high bits masked


# ---- the library ------------------------------------------------------------------------------------------------------------------------
def test_library_exports_exactly_the_header():
    declared = _declared(HDR, "FLDR_SHUTTER_API")
    assert len(declared) == 17, sorted(declared)
    assert _syms(LIB, ["--defined-only"]) == declared
    import fldr_shutter
    assert set(fldr_shutter.EXPORTS) == declared


def test_library_links_only_the_rate_video_and_model_apis():
    dyn = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    assert re.search(r"NEEDED.*\[libfldr_rate\.so\]", dyn) and re.search(r"NEEDED.*\[libfldr_video\.so\]", dyn), dyn
    assert not re.search(r"NEEDED.*\[libfldr_hip\.so\]", dyn), dyn
    assert re.search(r"R(UN)?PATH.*\$ORIGIN", dyn), dyn
    used = set(n for n in _syms(LIB, ["--undefined-only"]) if n.startswith("fldr_"))
    allowed = (_declared(os.path.join(INC, "fldr_rate.h"), "FLDR_RATE_API") | _declared(os.path.join(INC, "fldr_video.h"), "FLDR_VIDEO_API") |
               _declared(os.path.join(INC, "fldr_model.h"), "FLDR_MODEL_API"))
    assert used and used <= allowed, sorted(used)
    assert {"fldr_video_forward", "fldr_scene_measure"} <= used


def test_the_other_headers_and_libraries_know_nothing_of_the_shutter_api():
    for name in ("fldr_hip.h", "fldr_model.h", "fldr_video.h", "fldr_rate.h", "fldr_video_test_hooks.h", "fldr_hip_test_hooks.h"):
        assert "fldr_shutter" not in open(os.path.join(INC, name)).read(), name
    for name in ("libfldr_hip.so", "libfldr_model.so", "libfldr_video.so", "libfldr_rate.so"):
        assert not [n for n in _syms(os.path.join(PKG, name), []) if "fldr_shutter" in n], name


@pytest.mark.parametrize("compiler", [["gcc", "-std=c99", "-x", "c"], ["g++", "-std=c++11", "-x", "c++"]])
def test_header_is_plain_c99_and_cxx(compiler, tmp_path):
    if not shutil.which(compiler[0]):
        pytest.skip(compiler[0] + " not installed")
    src = tmp_path / "h.c"
    src.write_text('#include "fldr_shutter.h"\nint main(void) { return fldr_shutter_sizeof(0) > 0 && FLDR_SHUTTER_MAX_SUB == 64 ? 0 : 1; }\n')
    r = subprocess.run(compiler + ["-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I" + INC, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "hip/" not in open(HDR).read()


def test_example_builds_with_cc(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if not cc:
        pytest.skip("no C compiler")
    exe = tmp_path / "fldr_cine"
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + INC, "-o", str(exe),
                        os.path.join(ROOT, "examples", "fldr_cine.c"), "-L" + PKG, "-l:libfldr_shutter.so", "-l:libfldr_rate.so", "-l:libfldr_video.so",
                        "-l:libfldr_model.so", "-Wl,-rpath," + PKG], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    src = open(os.path.join(ROOT, "examples", "fldr_cine.c")).read()
    assert "hip" not in re.sub(r"/\*.*?\*/", "", src, flags=re.S).lower()
    for args in ([], ["w.npz", "64", "64", "120/0", "24"], ["w.npz", "64", "64", "120", "24", "angle=0"], ["w.npz", "64", "64", "120", "24", "sub=65"],
                 ["w.npz", "64", "64", "120", "24", "angle=361"]):
        u = subprocess.run([str(exe)] + args, capture_output=True, text=True)             # usage, no device touched
        assert u.returncode == 2 and "usage" in u.stderr, args


def test_no_unsafe_packed_fp32_in_the_shutter_library():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_pk_opsel.py"), LIB], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_kernels_read_and_write_wide_and_store_with_vector_stores_only():
    txt = "\n".join(_disassemble(LIB))
    for name in ("shutter_accumulate_kernel", "shutter_resolve_kernel", "shutter_mix_kernel"):
        assert name in txt
    assert len(re.findall(r"\bv_pk_(add|mul|fma)_f32\b", txt)) == 0                     # no packed fp32
    assert re.search(r"\bglobal_load_dwordx4\b", txt) and re.search(r"\bglobal_store_dwordx4\b", txt)
    assert not re.search(r"\bs_(buffer_|scratch_)?(store|atomic)_", txt)                # vector stores only
    assert not re.search(r"\bscratch_(load|store)_", txt)
    assert re.search(r"\bv_mul_hi_u32\b", txt)                                         # the multiplied reciprocal


def test_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    ks = KR.kernels(LIB)
    assert len(ks) == 18, [k["name"] for k in ks]         # accumulate, resolve, mix x (3 sample forms x wide / per-sample)
    for k in ks:
        assert k.get("scratch", -1) == 0 and k.get("vgpr_spills", -1) == 0 and k.get("sgpr_spills", -1) == 0, k
        assert k["lds"] == 0 and k["vgpr"] <= 128, k      # at least four waves per SIMD


def test_binding_struct_sizes_and_version():
    import fldr_shutter as T
    l = T.lib()
    text = open(HDR).read()
    assert l.fldr_shutter_version() == T.SHUTTER_VERSION == int(re.search(r"#define FLDR_SHUTTER_VERSION (\d+)", text).group(1)) == 100
    for which, cls in enumerate((T.ShutterConfig, T.Info)):
        assert l.fldr_shutter_sizeof(which) == ctypes.sizeof(cls)
    assert ctypes.sizeof(T.Info) == 24
    assert l.fldr_shutter_sizeof(2) == T.E_ARG
    for name, v in (("E_ARG", T.E_ARG), ("E_FORMAT", T.E_FORMAT), ("E_ACC", T.E_ACC), ("E_WEIGHT", T.E_WEIGHT), ("E_RATIO", T.E_RATIO),
                    ("E_DEVICE", T.E_DEVICE)):
        assert re.search(r"#define FLDR_SHUTTER_%s\s+\((-?\d+)\)" % name, text).group(1) == str(v)
        assert v <= -300                                                       # apart from the rate, video and model ranges
        assert l.fldr_shutter_error_string(v).decode().startswith("fldr_shutter")
    for name, v in (("MAX_OUT", T.MAX_OUT), ("MAX_SUB", T.MAX_SUB), ("LAUNCH_FRAMES", T.LAUNCH_FRAMES), ("MAX_TOTAL", T.MAX_TOTAL)):
        assert int(re.search(r"#define FLDR_SHUTTER_%s\s+(\d+)" % name, text).group(1)) == v
    assert T.LAUNCH_FRAMES >= 8 and 2 * 1023 * T.MAX_TOTAL + T.MAX_TOTAL < 2 ** 32
    assert l.fldr_shutter_error_string(-203).decode().startswith("fldr_rate")     # rate codes pass through
    assert l.fldr_shutter_error_string(-101).decode().startswith("fldr_video")    # video codes through it
    assert l.fldr_shutter_error_string(-3).decode().startswith("fldr_model")      # and model codes through that
    assert l.fldr_shutter_error_string(0).decode() == "success"


def test_acc_bytes_is_four_bytes_per_sample():
    import fldr_shutter as T
    import fldr_video as V
    for layout in ("nv12", "i420"):
        for depth in (8, 10):
            for H, W in ((2, 2), (3, 5), (1080, 1920), (2159, 3837)):
                samples = sum(r * c for r, c in V.plane_shapes(layout, H, W))
                assert T.acc_bytes(H, W, V.Format(layout, depth=depth)) == (4 * samples + 255) // 256 * 256
    assert T.lib().fldr_shutter_acc_bytes(0, 4, ctypes.byref(V.Format())) == T.E_ARG
    assert T.lib().fldr_shutter_acc_bytes(4, 4, None) == T.E_ARG
    f = V.Format()
    f.depth = 12
    assert T.lib().fldr_shutter_acc_bytes(4, 4, ctypes.byref(f)) == V.E_FORMAT


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
    """accumulate, resolve and mix: every refusal, with host memory in place of device memory — nothing may touch it.  Every call made
    here carries a defect: a call without one would be enqueued."""
    import fldr_shutter as T
    import fldr_video as V
    l = T.lib()
    b = 2 if depth == 10 else 1
    shapes = V.plane_shapes(layout, 64, 64)
    buf, base, _ = _host_frames(V, layout, depth, 1)

    def run(which, damage=None, H=64, W=64, n=3, weights=(1, 2, 3), acc=base, total=6, fmt=True, frames=True, out=True):
        """One call of `which`; damage(format, the last source frame, the output frame) spoils valid arguments."""
        _, _, fr = _host_frames(V, layout, depth, max(n, 1))
        _, _, o = _host_frames(V, layout, depth, 1)
        f = V.Format(layout, depth=depth)
        if damage:
            damage(f, fr[max(n, 1) - 1], o[0])
        w = (ctypes.c_int32 * max(len(weights), 1))(*weights)
        fp = ctypes.byref(f) if fmt else None
        if which == "accumulate":
            rc = l.fldr_shutter_accumulate(H, W, fp, fr if frames else None, w, n, 1, acc, None)
        elif which == "resolve":
            rc = l.fldr_shutter_resolve(H, W, fp, acc, total, o if out else None, None)
        else:
            rc = l.fldr_shutter_mix(H, W, fp, fr if frames else None, w, n, o if out else None, None)
        assert rc != 0, "a test call without a defect"
        return rc
    for which in ("accumulate", "resolve", "mix"):
        assert run(which, H=0) == T.E_ARG and run(which, W=0) == T.E_ARG and run(which, H=-1) == T.E_ARG
        assert run(which, fmt=False) == T.E_ARG
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
    for which in ("accumulate", "mix"):
        assert run(which, frames=False) == T.E_ARG and run(which, n=0) == T.E_ARG and run(which, n=-3) == T.E_ARG
        for bad in ((0, 1, 1), (1, 256, 1), (1, 1, -1)):
            assert run(which, weights=bad) == T.E_WEIGHT, bad
    for which in ("resolve", "mix"):
        assert run(which, out=False) == T.E_ARG
    for q in range(len(shapes)):                                                          # the mix's output, behind valid sources
        assert run("mix", lambda f, fr, o: o.plane.__setitem__(q, None)) == V.E_PLANE
        assert run("mix", lambda f, fr, o: o.pitch.__setitem__(q, shapes[q][1] * b - b)) == V.E_PITCH
    assert run("mix", n=T.LAUNCH_FRAMES + 1, weights=(1,) * (T.LAUNCH_FRAMES + 1)) == T.E_ARG       # a mix is one launch
    for total in (0, -1, 65536):
        assert run("resolve", total=total) == T.E_WEIGHT, total
    for which in ("accumulate", "resolve"):
        for acc in (None, base + 128, base + 16):
            assert run(which, acc=acc) == T.E_ACC, acc
    assert not buf.any()


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
    import fldr_shutter as T
    import fldr_video as V
    l = T.lib()
    ones = (ctypes.c_int32 * 64)(*([1] * 64))

    def call(io, w0=1, w1=1, w=ones):
        return l.fldr_shutter_forward(None, ctypes.byref(io), w0, w1, w, None, 0, None)
    assert call(_io(V, layout=layout)) == V.E_ARG                           # valid io, no model: the video library's refusal
    assert l.fldr_shutter_forward(None, None, 1, 1, ones, None, 0, None) == T.E_ARG
    assert call(_io(V, layout=layout), w=None) == T.E_ARG
    cases = []
    for field, val in (("layout", 1 - V.LAYOUTS[layout]), ("matrix", 0), ("range", 1), ("depth", 10)):
        io = _io(V, layout=layout); setattr(io.out_format, field, val); cases.append((io, T.E_FORMAT))     # valid, but not the input's
    io = _io(V, layout=layout); io.in_format.depth = 0; cases.append((io, V.E_ARG))                         # 0 and 8 are one depth
    for field, val in (("layout", 2), ("matrix", 2), ("range", 2)):
        io = _io(V, layout=layout); setattr(io.in_format, field, val); setattr(io.out_format, field, val); cases.append((io, V.E_FORMAT))
    io = _io(V, layout=layout); io.in_[0].pitch[0] = 63; cases.append((io, V.E_PITCH))
    io = _io(V, layout=layout); io.out[0].pitch[1] = (32 if layout == "i420" else 64) - 1; cases.append((io, V.E_PITCH))
    io = _io(V, layout=layout); io.in_[1].plane[1] = None; cases.append((io, V.E_PLANE))
    io = _io(V, layout=layout); io.out[0].plane[0] = None; cases.append((io, V.E_PLANE))
    io = _io(V, layout=layout); io.n_t = 0; cases.append((io, V.E_ARG))
    io = _io(V, layout=layout); io.n_t = 65; cases.append((io, T.E_ARG))
    io = _io(V, layout=layout); io.t = None; cases.append((io, V.E_ARG))
    io = _io(V, layout=layout); io.W = 1; cases.append((io, V.E_ARG))
    for io, code in cases:
        assert call(io) == code
    assert call(_io(V, layout=layout), w0=-1) == T.E_WEIGHT and call(_io(V, layout=layout), w1=256) == T.E_WEIGHT
    assert call(_io(V, layout=layout, n_t=2), w=(ctypes.c_int32 * 2)(1, 0)) == T.E_WEIGHT
    assert call(_io(V, layout=layout), w0=0, w1=0) == V.E_ARG               # allowed: the sub-frames alone (and then no model)
    assert l.fldr_shutter_workspace_bytes(None, 64, 64, 1) == V.E_ARG


def test_converter_argument_errors_before_any_device_call():
    import fldr_shutter as T
    import fldr_video as V
    l = T.lib()
    h = ctypes.c_void_p()

    def create(**kw):
        cfg = T.config(120, 24, (1, 2), 1, 64, 64, V.Format("i420"), 0, True)
        for k, v in kw.items():
            if k == "mutate":
                v(cfg)
            else:
                setattr(cfg, k, v)
        f, la = ctypes.c_int64(), ctypes.c_int64()
        rc = l.fldr_shutter_create(None, ctypes.byref(cfg), ctypes.byref(h))
        if rc == T.E_RATIO or kw.get("sub") in (0, 65):
            assert l.fldr_shutter_plan(ctypes.byref(cfg), 0, ctypes.byref(f), ctypes.byref(la)) == rc      # plan refuses what create refuses
        return rc
    assert create() == T.E_ARG                                               # valid, no model
    for term in ("in_num", "in_den", "out_num", "out_den", "shutter_num", "shutter_den"):
        assert create(**{term: 0}) == T.E_RATIO and create(**{term: -24}) == T.E_RATIO, term
    assert create(shutter_num=3, shutter_den=2) == T.E_RATIO                 # exposure longer than the output interval
    assert create(shutter_num=2, shutter_den=2) == T.E_ARG                   # s = 1 is allowed
    assert create(in_num=24, out_num=60, sub=1) == T.E_RATIO                 # s A sub = 0.2 < 1: a window could hold no grid point
    assert create(in_num=24, out_num=60, sub=4) == T.E_RATIO                 # 0.8
    assert create(in_num=24, out_num=60, sub=5) == T.E_ARG                   # exactly 1
    assert create(in_num=60, out_num=24, shutter_num=1, shutter_den=4, sub=1) == T.E_RATIO        # 0.625
    assert create(in_num=60, out_num=24, shutter_num=1, shutter_den=4, sub=2) == T.E_ARG
    assert create(sub=0) == T.E_ARG and create(sub=65) == T.E_ARG and create(sub=64) == T.E_ARG
    assert create(in_num=1, out_num=63, shutter_num=1, shutter_den=1, sub=64) == T.E_ARG          # 63 + 1 outputs per push: allowed
    assert create(in_num=1, out_num=64, shutter_num=1, shutter_den=1, sub=64) == T.E_RATIO        # 65
    assert create(in_num=2 ** 25 + 1, out_num=2 ** 25) == T.E_RATIO          # reduced terms above 2^24
    assert create(shutter_num=2 ** 25 - 1, shutter_den=2 ** 25) == T.E_RATIO
    assert create(in_num=2 ** 24, out_num=1, shutter_num=1, shutter_den=1, sub=64) == T.E_RATIO   # a window of 2^30 points: more than 65535
    assert create(in_num=60000, in_den=1001, out_num=24000, out_den=1001) == T.E_ARG
    assert create(scene=2) == T.E_ARG and create(scene=-1) == T.E_ARG
    assert create(H=1) == T.E_ARG and create(device=-1) == T.E_ARG
    assert create(mutate=lambda c: c.reserved.__setitem__(2, 1)) == T.E_ARG
    assert create(mutate=lambda c: setattr(c.scene_params, "sad_permille", 1001)) == T.E_ARG
    assert create(mutate=lambda c: c.scene_params.reserved.__setitem__(0, 1)) == T.E_ARG
    assert create(mutate=lambda c: setattr(c.format, "layout", 3)) == V.E_FORMAT
    assert create(mutate=lambda c: setattr(c.format, "depth", 12)) == V.E_FORMAT
    assert l.fldr_shutter_create(None, None, ctypes.byref(h)) == T.E_ARG
    n = ctypes.c_int()
    f = ctypes.c_int64()
    cfg = T.config(120, 24)
    assert l.fldr_shutter_plan(None, 0, ctypes.byref(f), ctypes.byref(f)) == T.E_ARG
    assert l.fldr_shutter_plan(ctypes.byref(cfg), -1, ctypes.byref(f), ctypes.byref(f)) == T.E_ARG
    assert l.fldr_shutter_plan(ctypes.byref(cfg), 0, None, ctypes.byref(f)) == T.E_ARG
    assert l.fldr_shutter_push(None, None, None, None, ctypes.byref(n), None) == T.E_ARG
    assert l.fldr_shutter_flush(None, None, None, ctypes.byref(n)) == T.E_ARG
    assert l.fldr_shutter_reset(None) == T.E_ARG
    assert l.fldr_shutter_max_out(None) == T.E_ARG
    l.fldr_shutter_destroy(None)
