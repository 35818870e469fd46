"""CPU checks of the 10-bit path through libfldr_hip.so and libfldr_model.so: the new entry points are exported and bound, the model
API grew two enum values and no function, field or byte, the headers still compile as C99 / C++11, and the 16-bit instantiation of the
fused synthesis kernel keeps the counted wait of the other product instantiations."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fldr-vfi_amd")
INC = os.path.join(ROOT, "include")
NEW_HIP = ("fldr_ingest_u16", "fldr_ingest_pyramid_u16", "fldr_quantize_u16", "fldr_dec23_synth_u16")


def test_new_entry_points_are_declared_exported_and_bound():
    import fldr_hip
    hdr = open(os.path.join(INC, "fldr_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "libfldr_hip.so")], capture_output=True, text=True, check=True).stdout
    syms = set(l.split()[-1] for l in out.splitlines() if l.strip())
    for name in NEW_HIP:
        assert re.search(r"FLDR_API\s+int\s+%s\s*\(" % name, hdr), name
        assert name in syms and name in fldr_hip.EXPORTS, name
        getattr(fldr_hip.lib(), name)
    for fn in ("ingest_pyramid_u16", "quantize_u16"):
        assert callable(getattr(fldr_hip, fn))
    import fldr_harness
    assert callable(fldr_harness.interpolate_u16)


def test_new_entry_points_refuse_bad_arguments_before_any_launch():
    """Null pointers and a white level outside 1 .. 65535 are FLDR_E_ARG; no device is needed to be told so."""
    import fldr_hip
    l = fldr_hip.lib()
    buf = (ctypes.c_uint16 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    lv = (ctypes.c_void_p * 1)(p)
    assert l.fldr_ingest_pyramid_u16(None, lv, 1, 1023, 1, 8, 8, 8, 8, None) == -1
    assert l.fldr_ingest_pyramid_u16(p, lv, 1, 0, 1, 8, 8, 8, 8, None) == -1
    assert l.fldr_ingest_pyramid_u16(p, lv, 1, 65536, 1, 8, 8, 8, 8, None) == -1
    assert l.fldr_ingest_pyramid_u16(ctypes.c_void_p(p.value + 1), lv, 1, 1023, 1, 8, 8, 8, 8, None) == -1       # odd address
    assert l.fldr_ingest_pyramid_u16(p, lv, 8, 1023, 1, 8, 8, 8, 8, None) == -1                                  # more than 7 levels
    assert l.fldr_ingest_pyramid_u16(p, lv, 1, 1023, 1, 8, 8, 24, 8, None) == -2                                 # pad >= size
    assert l.fldr_ingest_u16(p, None, 1023, 1, 8, 8, 8, 8, None) == -1
    assert l.fldr_quantize_u16(p, 1, None, 1023, 1, 8, 8, 8, 8, None) == -1
    assert l.fldr_quantize_u16(p, 1, p, 0, 1, 8, 8, 8, 8, None) == -1
    assert l.fldr_quantize_u16(p, 1, p, 1023, 1, 9, 8, 8, 8, None) == -1                                         # crop larger than the frame


def test_model_api_grew_two_values_and_nothing_else():
    import fldr_model as M
    hdr = open(os.path.join(INC, "fldr_model.h")).read()
    assert re.search(r"FLDR_MODEL_IN_U10_PLANAR\s*=\s*3\b", hdr) and re.search(r"FLDR_MODEL_OUT_U10_PLANAR\s*=\s*3\b", hdr)
    assert (M.IN_U10_PLANAR, M.OUT_U10_PLANAR) == (3, 3)
    assert (M.IN_PYRAMID, M.IN_U8_PLANAR, M.IN_U8_INTERLEAVED, M.OUT_F64, M.OUT_U8_PLANAR, M.OUT_U8_INTERLEAVED) == (0, 1, 2, 0, 1, 2)
    assert M.MODEL_VERSION == 101 and M.lib().fldr_model_version() == 101
    # sizeof(fldr_model_tensor), fldr_model_config, fldr_model_io as they were before the 10-bit forms
    assert [M.lib().fldr_model_sizeof(i) for i in range(3)] == [56, 32, 160]
    assert len(set(re.findall(r"FLDR_MODEL_API\s+[^;(]*?\b(fldr_[a-z0-9_]+)\s*\(", hdr))) == 9
    assert callable(M.NativeModel.interpolate_u10)


@pytest.mark.parametrize("compiler", [["gcc", "-std=c99", "-x", "c"], ["g++", "-std=c++11", "-x", "c++"]])
@pytest.mark.parametrize("header", ["fldr_hip.h", "fldr_model.h"])
def test_headers_are_plain_c99_and_cxx(compiler, header, tmp_path):
    if not shutil.which(compiler[0]):
        pytest.skip(compiler[0] + " not installed")
    src = tmp_path / "h.c"
    src.write_text('#include "%s"\nint main(void) { return 0; }\n' % header)
    r = subprocess.run(compiler + ["-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I" + INC, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_16_bit_synthesis_instantiation_keeps_the_counted_wait(tmp_path):
    """As test_host_cpu's listing check of the fp64 and 8-bit instantiations: behind its LDS-DMA pieces every consumer wave of
    dec23_synth_kernel<uint16_t> issues exactly three vector-memory stores on every path, so `s_waitcnt vmcnt(3)` proves the pieces
    landed; no compiler-placed vmcnt(0) in between, no scratch."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = str(tmp_path / "dec23.s")
    subprocess.run([hipcc, "@" + os.path.join(PKG, "csrc", "hipcc_flags.rsp"), "-fvisibility=hidden", "-I" + INC, "-S", "--cuda-device-only",
                    os.path.join(PKG, "csrc", "dec23_kernels.hip"), "-o", out], check=True, capture_output=True, timeout=600)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_dma_waits as C
    problems, notes = C.check(out, "dec23_synth_kernelItE", expect_counted=3)
    assert not problems, (problems, notes)
    assert "[(3, [3])]" in notes[0], notes


def test_new_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    ks = [k for k in KR.kernels(os.path.join(PKG, "libfldr_hip.so"))
          if re.search(r"ingest_pyramid_kernelIt|ingest_u16_kernel|quantize_u16_kernel|dec23_synth_kernelIt", k["name"])]
    assert len(ks) == 5, [k["name"] for k in ks]
    for k in ks:
        assert k["scratch"] == 0 and k["vgpr_spills"] == 0, k
