"""Seeded inputs of the convolution tests, shared by the CPU tests (tests/test_conv_ref_cpu.py: the float64 statement of
tests/conv_float_ref.py against fp32 torch, an emulation of the split operands and six mutants) and the GPU tests
(tests/test_gpu_conv_ops.py: every convolution entry point against the float64 statement within the derived bound).  Plain torch-CPU
generators; every tensor depends only on its case.

Layer specs: the twelve layers of the model (CONVS of tests/test_gpu_parity.py, imported) and generic ones the model never uses:
cin 1, 3, 7, 26, 100; cout 1, 6 (4 stored), 16, 17, 48, 96; 3x3 stride 1 and 4x4 stride 2 (cout up to 64; 96 is refused by the
library and listed apart); concatenations whose last source is no multiple of 8 channels; a nearest-x2 source first and second; with
and without bias, ReLU and an fp32 residual.

Output shapes: all convolution tiles are 8 x 32 (the ring has an 8 x 16 variant): one pixel, one row, one column, 2 x 2, one short of
a tile, one tile, one past it in both directions, the narrow tile and one past it, and three tile rows by three tile columns.  The
stride-2 shapes are INPUT sizes (output (H + 2 - 4) // 2 + 1): a one-pixel output, odd sizes, one tile, one output past it from an odd
and from an even input, one output row, one output column.  N = 3 on one shape per list.

Data kinds (activations):
  unit   uniform in [-1, 1];
  relu   max(randn, 0): exact zeros on half of the pixels;
  mixed  per-channel magnitudes log-spaced from 1e-6 to 1e3 (shuffled over the channels) times uniform [-1, 1]: crosses 2^-14, where
         the fp16 `hi` of the split goes subnormal, and 0.25, where `lo` does;
  dark   uniform in [-1e-3, 1e-3]: every `lo` subnormal.
Weight kinds: `plain` randn / sqrt(fan-in); `spike` the same / 32 with ONE weight at 1e3 / (32 sqrt(fan-in)), i.e. 1e3 times the
rest: the power-of-two prepack scale follows the spike and pushes the low halves of all other weights towards fp16's subnormals.
Biases are 0.1 randn (scaled with the data for `dark`), residuals uniform in [-1, 1] times the data's magnitude.  No value reaches
65504 and no output does: tests/test_conv_ref_cpu.py asserts it on the magnitude sum S of every case, so fldr_range_status stays
clean."""
import math
from collections import namedtuple

import torch

from test_gpu_parity import CONVS

Spec = namedtuple("Spec", "name parts cout k stride relu residual store up2 bias")
Case = namedtuple("Case", "spec N H W kind wkind")        # H, W: the output size of a stride-1 case, the INPUT size of a stride-2 case

MODEL_NAMES = ["rec_ctx_ds.2", "conv_flow1", "conv_flow2.0", "conv_flow_bottom.8", "conv_flow2.8", "enc1", "enc2", "enc3", "dec0", "dec1", "dec2", "dec3"]
assert len(CONVS) == len(MODEL_NAMES)
MODEL = [Spec(n, tuple(p), co, k, s, relu, res, store, tuple(bool(u) for u in (up2 or [False] * len(p))), True)
         for n, (p, co, k, s, relu, res, store, up2) in zip(MODEL_NAMES, CONVS)]

GENERIC = [
    Spec("g1->1", (1,), 1, 3, 1, False, False, None, (False,), False),
    Spec("g3->16", (3,), 16, 3, 1, True, True, None, (False,), True),
    Spec("g7->17", (7,), 17, 3, 1, False, False, None, (False,), True),
    Spec("g26->48", (26,), 48, 3, 1, True, False, None, (False,), False),
    Spec("g100->96", (100,), 96, 3, 1, True, True, None, (False,), True),
    Spec("g8+16+3->6/4", (8, 16, 3), 6, 3, 1, False, True, 4, (False, False, False), True),
    Spec("g16+8+2->64", (16, 8, 2), 64, 3, 1, True, False, None, (False, False, False), True),
    Spec("gup16+24+5->96", (16, 24, 5), 96, 3, 1, True, False, None, (True, False, False), True),
    Spec("g16+up8+2->16", (16, 8, 2), 16, 3, 1, True, True, None, (False, True, False), False),
    Spec("s1->1", (1,), 1, 4, 2, False, False, None, (False,), False),
    Spec("s7->17", (7,), 17, 4, 2, True, False, None, (False,), True),
    Spec("s3+3+1->6/4", (3, 3, 1), 6, 4, 2, False, False, 4, (False, False, False), True),
    Spec("s26->48", (26,), 48, 4, 2, True, False, None, (False,), True),
    Spec("s100->64", (100,), 64, 4, 2, True, False, None, (False,), False),
    Spec("s8->16", (8,), 16, 4, 2, True, False, None, (False,), True),
    Spec("s24->17", (24,), 17, 4, 2, False, False, None, (False,), True),
    Spec("s40->32", (40,), 32, 4, 2, True, False, None, (False,), False),
]
SPECS = MODEL + GENERIC
REFUSED_S2 = Spec("s16->96", (16,), 96, 4, 2, True, False, None, (False,), True)      # 4x4 stride 2 beyond 64 outputs: no kernel takes it

# (N, H, W)
SHAPES_3X3 = [(1, 1, 1), (1, 1, 33), (2, 9, 1), (1, 2, 2), (1, 7, 31), (2, 8, 32), (3, 9, 33), (1, 8, 16), (2, 8, 17), (1, 17, 65)]
SHAPES_UP2 = [(1, 2, 2), (2, 8, 32), (3, 10, 34), (1, 16, 66)]
SHAPES_S2 = [(1, 2, 2), (2, 3, 5), (1, 16, 64), (3, 17, 65), (2, 18, 66), (1, 2, 70), (1, 40, 2)]
# the shapes either side of a tile edge: the only ones the kernel-variant tests (test build) run
TILE_EDGE_3X3 = [(7, 31), (8, 32), (9, 33), (8, 16), (8, 17)]
TILE_EDGE_UP2 = [(8, 32), (10, 34)]
TILE_EDGE_S2 = [(16, 64), (17, 65), (18, 66)]
# stride-2 inputs with no output row or column: refused by every entry point
DEGENERATE_S2 = [(1, 6), (6, 1), (1, 1)]

KINDS = ["unit", "relu", "mixed", "dark"]
WKINDS = ["plain", "spike", "plain"]


def shapes_of(spec):
    return SHAPES_S2 if spec.stride == 2 else (SHAPES_UP2 if any(spec.up2) else SHAPES_3X3)


def cases(specs=None):
    """Every (spec, shape) once; the data and weight kinds rotate so that every spec meets every data kind and both weight kinds over
    its shapes, and every shape meets them over the specs."""
    out = []
    for si, spec in enumerate(SPECS):
        if specs is not None and spec not in specs:
            continue
        for hi, (N, H, W) in enumerate(shapes_of(spec)):
            out.append(Case(spec, N, H, W, KINDS[(si + hi) % len(KINDS)], WKINDS[(si + 2 * hi) % len(WKINDS)]))
    return out


def tile_edge(case):
    s = case.spec
    return (case.H, case.W) in (TILE_EDGE_S2 if s.stride == 2 else (TILE_EDGE_UP2 if any(s.up2) else TILE_EDGE_3X3))


def out_size(case):
    if case.spec.stride == 2:
        return (case.H + 2 - 4) // 2 + 1, (case.W + 2 - 4) // 2 + 1
    return case.H, case.W


def _gen(case, salt):
    seed = 77003 + salt
    for k in (SPECS.index(case.spec) if case.spec in SPECS else 99, case.N, case.H, case.W, KINDS.index(case.kind), WKINDS.index(case.wkind)):
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _uniform(g, shape):
    return torch.rand(*shape, generator=g) * 2 - 1


def magnitude(kind):
    """The typical size of a value of the kind: what biases and residuals are scaled with."""
    return 1e-3 if kind == "dark" else 1.0


def activation(kind, shape, g):
    N, C, H, W = shape
    if kind == "unit":
        return _uniform(g, shape)
    if kind == "relu":
        return torch.relu(torch.randn(*shape, generator=g))
    if kind == "dark":
        return _uniform(g, shape) * 1e-3
    assert kind == "mixed", kind
    e = torch.linspace(-6.0, 3.0, C) if C > 1 else torch.tensor([-3.0])
    mag = (10.0 ** e.double()).float()[torch.randperm(C, generator=g)]
    return _uniform(g, shape) * mag.view(1, C, 1, 1)


def weights(spec, wkind, g):
    cin, n = sum(spec.parts), sum(spec.parts) * spec.k * spec.k
    w = torch.randn(spec.cout, cin, spec.k, spec.k, generator=g) / math.sqrt(n)
    if wkind == "spike":
        w = w / 32
        i = int(torch.randint(0, w.numel(), (1,), generator=g))
        w.view(-1)[i] = 1e3 / (32 * math.sqrt(n)) * (1.0 if w.view(-1)[i] >= 0 else -1.0)
    return w


def make(case):
    """-> dict(srcs: fp32 sources (a nearest-x2 source at half the size), w, b or None, res or None: fp32, of the STORED output's shape)."""
    s = case.spec
    g = _gen(case, 0)
    srcs = [activation(case.kind, (case.N, c, case.H // 2 if u else case.H, case.W // 2 if u else case.W), g) for c, u in zip(s.parts, s.up2)]
    w = weights(s, case.wkind, g)
    m = magnitude(case.kind)
    b = torch.randn(s.cout, generator=g) * 0.1 * m if s.bias else None
    Ho, Wo = out_size(case)
    res = _uniform(g, (case.N, s.store or s.cout, Ho, Wo)) * m if s.residual else None
    return dict(srcs=srcs, w=w, b=b, res=res)
