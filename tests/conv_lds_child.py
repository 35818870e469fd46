"""Child program of tests/test_gpu_conv_ops.py::test_lds_limit_follows_ascending_cin: the stride-2 convolutions whose dynamic-LDS size
grows with cin, run with ASCENDING cin through one kernel instantiation each in a FRESH process (the limits the launchers remember are
process-wide), every result held to the float64 bound of tests/conv_float_ref.py.  6 x 10 inputs, one sample.  Exit status 0 = all
within the bound; anything else (an assertion, a refused launch) is a non-zero status with the story on stderr.

  cout 32, cin 8 then 40    fldr_conv2d_s2_spk and the pair form: conv4x4s2_dma_spk_kernel (89 KB -> 154 KB of LDS; 40 is the widest
                            input whose weights fit next to its two window stages in 160 KB);
  the same, s2_dma hook 0,  conv4x4s2_pers_spk_kernel<32, 1, 2> (test build; 61 KB -> 141 KB, 48 the widest input within 156 KB);
  cin 8 then 48
  cout 16, cin 8 then 32    conv4x4s2_pers_spk_kernel<16, 1, 4> (53 KB -> 77 KB, 32 the widest input within 80 KB);
  cout 16, cin 4, 32, 64    fldr_conv2d_s2_split on fp32 sources: conv4x4s2_pers_kernel<16, 1, 4> up to cin 32, the tiled kernel at 64.
cin 64 on a packed source is beyond every one of the three packed-source kernels: it must be REFUSED (FLDR_E_SHAPE), never run."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(os.path.dirname(HERE), "fldr-vfi_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import conv_cases as CC  # noqa: E402
import conv_float_ref as R  # noqa: E402
import test_gpu_conv_ops as T  # noqa: E402


def case(cin, cout):
    spec = CC.Spec("s%d->%d" % (cin, cout), (cin,), cout, 4, 2, True, False, None, (False,), True)
    return CC.Case(spec, 1, 6, 10, "unit", "plain")


def refused(hip, c, dev):
    D = T._inputs(c, dev)
    assert not hip.s2_spk_ok(D["w"]), c.spec.name
    try:
        hip.conv2d_s2_spk(hip.spk_pack(D["srcs"][0]), D["w"], D["b"], relu=True)
    except hip.FldrError as e:
        print("%s on a packed source refused: %s" % (c.spec.name, e))
    else:
        raise AssertionError("%s on a packed source: beyond every kernel's LDS, expected FLDR_E_SHAPE" % c.spec.name)


def main():
    import fldr_hip as hip
    hip.lib()
    dev = torch.device("cuda:0")
    hip.device_status(reset=True)
    for cin in (8, 40):
        T._show(case(cin, 32), T._s2_spk_forms(hip, case(cin, 32), dev))
    refused(hip, case(64, 32), dev)
    for cin in (8, 32):
        T._show(case(cin, 16), T._s2_spk_forms(hip, case(cin, 16), dev))
    refused(hip, case(64, 16), dev)
    for cin in (4, 32, 64):
        c = case(cin, 16)
        d, ref, terms = R.reference(c)
        D = T._inputs(c, dev)
        got = hip.conv2d(D["srcs"], D["w"], D["b"], stride=2, relu=True, precision="split")
        T._show(c, {"split": T._within(T._label(c) + " fp32 sources", got, ref, terms.bound("split"))})
    T._clean(hip)
    with hip.test_hooks() as L:
        hip.device_status(reset=True)
        assert L.fldr_debug_s2_dma(0) == 0
        try:
            for cin in (8, 48):
                T._show(case(cin, 32), T._s2_spk_forms(hip, case(cin, 32), dev))
            refused(hip, case(64, 32), dev)
        finally:
            L.fldr_debug_s2_dma(1)
        T._clean(hip)
    torch.cuda.synchronize()
    print("lds limit child: ok")


if __name__ == "__main__":
    main()
