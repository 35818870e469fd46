"""CPU checks of the C model API (include/fldr_model.h, libfldr_model.so): the library's symbol table and link, the header as plain
C99 / C++, the C example, the packed-fp32 guard, the binding's struct mirrors and the .npz reader's refusal of malformed files —
which happens before any HIP call, so it runs without a GPU."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
import zipfile

import numpy as np
import pytest

import lib_checks
from lib_checks import declared as _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fldr-vfi_amd")
HDR = os.path.join(ROOT, "include", "fldr_model.h")
LIB = os.path.join(PKG, "libfldr_model.so")
WEIGHTS = os.path.join(PKG, "weights", "fLDRnet_X4K1000FPS_exp1_best_PSNR.npz")


def _syms(args):
    return lib_checks.syms(LIB, args)


def test_library_exports_exactly_the_header():
    declared = _declared(HDR, "FLDR_MODEL_API")
    assert len(declared) == 9, sorted(declared)
    assert _syms(["--defined-only"]) == declared
    import fldr_model
    assert set(fldr_model.EXPORTS) == declared


def test_library_links_only_the_public_abi_of_libfldr_hip():
    dyn = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    assert re.search(r"NEEDED.*\[libfldr_hip\.so\]", dyn), dyn
    assert re.search(r"R(UN)?PATH.*\$ORIGIN", dyn), dyn
    public = _declared(os.path.join(ROOT, "include", "fldr_hip.h"), "FLDR_API")
    used = set(n for n in _syms(["--undefined-only"]) if n.startswith("fldr_"))
    assert used and used <= public, sorted(used - public)
    assert "fldr_status_word" in used


@pytest.mark.parametrize("compiler", [["gcc", "-std=c99", "-x", "c"], ["g++", "-std=c++11", "-x", "c++"]])
def test_header_is_plain_c99_and_cxx(compiler, tmp_path):
    if not shutil.which(compiler[0]):
        pytest.skip(compiler[0] + " not installed")
    src = tmp_path / "h.c"
    src.write_text('#include "fldr_model.h"\nint main(void) { return fldr_model_sizeof(0) > 0 ? 0 : 1; }\n')
    r = subprocess.run(compiler + ["-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_example_builds_with_cc(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if not cc:
        pytest.skip("no C compiler")
    exe = tmp_path / "fldr_interp"
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", str(exe),
                        os.path.join(ROOT, "examples", "fldr_interp.c"), "-L" + PKG, "-l:libfldr_model.so", "-Wl,-rpath," + PKG],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    src = open(os.path.join(ROOT, "examples", "fldr_interp.c")).read()
    assert "hip" not in re.sub(r"/\*.*?\*/", "", src, flags=re.S).lower()
    u = subprocess.run([str(exe)], capture_output=True, text=True)            # no arguments: usage, no device touched
    assert u.returncode == 2 and "usage" in u.stderr


def test_no_unsafe_packed_fp32_in_the_model_library():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_pk_opsel as C
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_pk_opsel.py"), LIB], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert C is not None


def test_binding_struct_sizes_and_version():
    import fldr_model
    l = fldr_model.lib()
    assert [l.fldr_model_sizeof(i) for i in range(3)] == [ctypes.sizeof(c) for c in (fldr_model.Tensor, fldr_model.Config, fldr_model.IO)]
    assert l.fldr_model_sizeof(3) == fldr_model.E_ARG
    assert l.fldr_model_version() == fldr_model.MODEL_VERSION
    assert re.search(r"#define FLDR_MODEL_VERSION %d\b" % fldr_model.MODEL_VERSION, open(HDR).read())
    for name, code in (("E_WORKSPACE", -10), ("E_BATCH", -11), ("E_COMPRESSED", -14), ("E_TRUNCATED", -15), ("E_MISSING", -16),
                       ("E_TENSOR_SHAPE", -17), ("E_DTYPE", -18)):
        assert re.search(r"#define FLDR_MODEL_%s\s+\(%d\)" % (name, code), open(HDR).read()), name
        assert getattr(fldr_model, name) == code
        assert l.fldr_model_error_string(code).startswith(b"fldr_model: ")


# ---- the .npz reader: every malformed file is refused with its code before a HIP call ----------------------------------------------

def _arrays():
    z = np.load(WEIGHTS)
    return {k: z[k] for k in z.files}


def _create(path):
    import fldr_model
    cfg = fldr_model.Config(0, 5)
    h = ctypes.c_void_p()
    rc = fldr_model.lib().fldr_model_create_npz(os.fsencode(str(path)), ctypes.byref(cfg), ctypes.byref(h))
    assert not h.value or rc == 0
    if h.value:
        fldr_model.lib().fldr_model_destroy(h)
    return rc


def _hip_devices():
    import torch
    return torch.cuda.device_count() if torch.cuda.is_available() else 0


def test_npz_reader_accepts_the_shipped_file():
    import fldr_model
    rc = _create(WEIGHTS)
    # parsed and validated; what follows needs a device (FLDR_MODEL_E_DEVICE on a machine without one)
    assert rc == (0 if _hip_devices() else fldr_model.E_DEVICE), rc


def test_npz_reader_accepts_state_dict_aliases(tmp_path):
    import fldr_model
    a = _arrays()
    b = {("base_modules.1." + k[7:] if k.startswith("vfinet.") else k): v for k, v in a.items()}
    p = tmp_path / "alias.npz"
    np.savez(p, **b)
    assert _create(p) == (0 if _hip_devices() else fldr_model.E_DEVICE)


def test_npz_reader_refuses_a_compressed_entry(tmp_path):
    import fldr_model
    p = tmp_path / "c.npz"
    np.savez_compressed(p, **_arrays())
    assert _create(p) == fldr_model.E_COMPRESSED


def test_npz_reader_refuses_a_truncated_file(tmp_path):
    import fldr_model
    data = open(WEIGHTS, "rb").read()
    for cut in (len(data) // 2, len(data) - 30, 100):
        p = tmp_path / ("t%d.npz" % cut)
        p.write_bytes(data[:cut])
        assert _create(p) == fldr_model.E_TRUNCATED, cut


def test_npz_reader_refuses_a_missing_key(tmp_path):
    import fldr_model
    a = _arrays()
    del a["vfinet.refine_unet.dec1.bias"]
    p = tmp_path / "m.npz"
    np.savez(p, **a)
    assert _create(p) == fldr_model.E_MISSING


def test_npz_reader_refuses_a_wrong_shape(tmp_path):
    import fldr_model
    a = _arrays()
    a["vfinet.conv_flow1.weight"] = a["vfinet.conv_flow1.weight"][:, :95].copy()
    p = tmp_path / "s.npz"
    np.savez(p, **a)
    assert _create(p) == fldr_model.E_TENSOR_SHAPE


def test_npz_reader_refuses_a_wrong_dtype(tmp_path):
    import fldr_model
    for key, dt in (("EV8", np.float32), ("rec_ctx_ds.0.weight", np.float64), ("vfinet.conv_flow1.bias", np.float16)):
        a = _arrays()
        a[key] = a[key].astype(dt)
        p = tmp_path / "d.npz"
        np.savez(p, **a)
        assert _create(p) == fldr_model.E_DTYPE, key


def test_npz_reader_refuses_other_files(tmp_path):
    import fldr_model
    p = tmp_path / "x.npz"
    p.write_bytes(b"not a zip file at all" * 10)
    assert _create(p) == fldr_model.E_FORMAT
    assert _create(tmp_path / "absent.npz") == fldr_model.E_IO
    with zipfile.ZipFile(tmp_path / "e.npz", "w") as z:                      # a zip without the tensors
        z.writestr("readme.txt", "x")
    assert _create(tmp_path / "e.npz") in (fldr_model.E_FORMAT, fldr_model.E_MISSING)


def test_create_refuses_bad_config_before_touching_a_device():
    import fldr_model
    l = fldr_model.lib()
    h = ctypes.c_void_p()
    for cfg in (fldr_model.Config(0, 2), fldr_model.Config(0, 8), fldr_model.Config(-1, 5)):
        assert l.fldr_model_create_npz(os.fsencode(WEIGHTS), ctypes.byref(cfg), ctypes.byref(h)) == fldr_model.E_ARG
    assert l.fldr_model_create(None, 0, ctypes.byref(fldr_model.Config(0, 5)), ctypes.byref(h)) == fldr_model.E_ARG
    assert l.fldr_model_workspace_bytes(None, 256, 256, 1) == fldr_model.E_ARG
    assert l.fldr_model_forward(None, None, None, 0, None) == fldr_model.E_ARG
