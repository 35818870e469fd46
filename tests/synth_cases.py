"""Seeded inputs of the synthesis tests, shared by the CPU tests (tests/test_synth_ref_cpu.py: the float64 statement of
tests/synth_float_ref.py against a literal transcription, emulations of the kernels' arithmetic and eleven mutants) and the GPU tests
(tests/test_gpu_synth_ops.py: fldr_dec3_synth, fldr_dec3_synth_spk, fldr_synth_tail and fldr_dec23_synth in every output form against
the statement within the derived bound).  Plain torch-CPU generators; every tensor depends only on its case.

Families.  "dec3": the inputs of the two dec3 + blend kernels (d2 [N,16,h,w], w3, b3); fldr_synth_tail runs on the logits of the
same cases.  "dec23": the inputs of the fused kernel (dec1 [N,32,h/2,w/2], enc1 [N,16,h,w], w2, b2, w3, b3).  (h, w) is the HALF
resolution; the frame is 2h x 2w.

Shapes.  The dec3 tiles are 8 x 32 at half resolution, dec23's as well (16 frame rows per tile row): one pixel, one row, one column,
2 x 2, one short of a tile, one tile, one past it in both directions, three tiles by three; dec23 needs even h and w (dec1 lives at a
quarter of the frame): the same edges in even numbers.  N = 3 on (9, 33) and on (18, 66) (27 tiles: several per workgroup once the
test build lowers the workgroup count).

Regimes.
  exact    every operand dyadic, so that every fp32 product and every partial sum of both convolutions is exact in ANY order, the
           hi + lo split holds every value and the weights' `lo` halves are 0: a correct kernel's logits are the statement's bit for
           bit and only the tail's arithmetic is left to bound.  dec1 / enc1: multiples of 2^-10 in [0, 2); w2: a quarter of the taps
           set, multiples of 1/4 in [-1/2, 1/2]; b2: multiples of 1/16 in [-1, 1]; w3: multiples of 1/4 in [-1/2, 1/2] times 2^-6;
           b3: multiples of 2^-6 in [-1, 1]; the dec3 family's d2: ReLU of multiples of 2^-12 (three standard deviations of 3), like
           the dec2 values of the other family.  Pattern "stripes": channel k < 6 of d2 (of enc1, passed on by a one-tap w2) is 64 on
           the columns x = k mod 6 and w3 passes half of it to logit k: every candidate leads by 32 on a stripe of its own.
  bias     w3 = 0: the logits are exactly b3 for every kernel, whatever d2 is (generic data).  Patterns: flat; one candidate ahead by
           10, 40 or 100 (the candidate rotates with the case); (-85, +85) alternating in both parities on two samples with t = 0 and
           t = 1: on one sample of each the candidates with a non-zero t weight are 170 below the others.
  generic  conv_cases' activation kinds relu, mixed and dark with weights plain and spike: geometry and data ranges, not last bits
           (the chained bound of two stacked layers is of the order of 1e-3).

Candidates are uniform in [-1.2, 1.2], so both clamps of the rounded forms act; `equal`: all six are one tensor (the frame is then
that tensor to a few fp64 ulps); `near`: six tensors within 0.05 of a common one, as six estimates of one frame are (the only
kinds, with `equal`, whose frame bound is below 1 % of a 16-bit code: the white level 65535 runs on those); `pair`: candidates 4 and 5
are the channel-strided planes of an [N,3,2,H,W] tensor, as I0 / I1 are in the model.  t differs per sample and rotates through T_VALUES: the edge values 0, 1, 2^-24, 1 - 2^-24, 0.125, 0.5, whose fp32 `1 - t`
is exact, and two values whose fp32 `1 - t` is ROUNDED (2^-25: 1 - t = 1; fp32(1/3)): only on those can a float64 `1 - t` be told
from the fp32 one."""
from collections import namedtuple

import torch

import conv_cases as CC

Case = namedtuple("Case", "fam regime pattern N h w cand")

T_PARAM = 1.5616
SPEC2 = CC.Spec("dec2", (32, 16), 16, 3, 1, True, False, None, (True, False), True)
SPEC3 = CC.Spec("dec3", (16,), 6, 3, 1, False, False, None, (True,), True)
assert SPEC2 in CC.MODEL and SPEC3 in CC.MODEL

DEC3_SHAPES = [(1, 1, 1), (1, 1, 33), (2, 9, 1), (1, 2, 2), (2, 7, 31), (2, 8, 32), (3, 9, 33), (1, 17, 65)]
DEC23_SHAPES = [(1, 2, 2), (2, 2, 34), (1, 10, 2), (2, 6, 30), (1, 8, 32), (2, 10, 34), (3, 18, 66)]
TILE_EDGE_DEC3 = [(7, 31), (8, 32), (9, 33)]
TILE_EDGE_DEC23 = [(6, 30), (8, 32), (10, 34)]
MULTI_TILE_DEC23 = (3, 18, 66)

T_EDGE = [0.0, 1.0, 2.0 ** -24, 1.0 - 2.0 ** -24, 0.125, 0.5]
T_ROUNDED = [2.0 ** -25, 1.0 / 3.0]                    # fp32 1 - t is rounded
T_VALUES = T_EDGE + T_ROUNDED

BIAS_PATTERNS = ["flat", "lead10", "lead40", "lead100", "alt85a", "alt85b"]
GENERIC_PATTERNS = ["relu/plain", "mixed/spike", "dark/plain", "relu/spike", "mixed/plain", "dark/spike"]
CAND_KINDS = ["uniform", "equal", "near", "pair", "uniform"]


def _cases():
    out = []
    for fam, shapes in (("dec3", DEC3_SHAPES), ("dec23", DEC23_SHAPES)):
        for i, (N, h, w) in enumerate(shapes):
            mine = [("exact", "dyadic", N), ("generic", GENERIC_PATTERNS[i % 6], N)]
            if i in (2, 5):
                mine.append(("exact", "stripes", N))
            for p in (BIAS_PATTERNS[(2 * i) % 6], BIAS_PATTERNS[(2 * i + 1) % 6]):
                mine.append(("bias", p, 2 if p.startswith("alt85") else N))
            for regime, pattern, n in mine:
                out.append(Case(fam, regime, pattern, n, h, w, CAND_KINDS[len(out) % len(CAND_KINDS)]))
    return out


CASES = _cases()


def cases(fam=None, regime=None):
    return [c for c in CASES if (fam is None or c.fam == fam) and (regime is None or c.regime == regime)]


def label(case):
    return "%-5s %-7s %-11s N %d %2dx%-2d %-7s" % (case.fam, case.regime, case.pattern, case.N, case.h, case.w, case.cand)


def tile_edge(case):
    return (case.h, case.w) in (TILE_EDGE_DEC3 if case.fam == "dec3" else TILE_EDGE_DEC23)


def _gen(case, salt=0):
    seed = 91009 + salt
    for k in (CASES.index(case) if case in CASES else 999, case.N, case.h, case.w):
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def t_values(case):
    """fp32 [N]: alt85 cases t = (0, 1); otherwise T_VALUES rotated by the case's rank in its family and regime, so that every edge value meets every regime."""
    if case.pattern.startswith("alt85"):
        return torch.tensor([0.0, 1.0], dtype=torch.float32)
    mine = [c for c in CASES if c.fam == case.fam and c.regime == case.regime and not c.pattern.startswith("alt85")]
    i = mine.index(case) if case in mine else 0
    return torch.tensor([T_VALUES[(i + 3 * n) % len(T_VALUES)] for n in range(case.N)], dtype=torch.float64).float()


def bias_pattern(case):
    """b3 of a bias-only case."""
    p = case.pattern
    if p == "flat":
        return torch.full((6,), 0.25)
    if p == "alt85a":
        return torch.tensor([-85.0, 85.0] * 3)
    if p == "alt85b":
        return torch.tensor([85.0, -85.0] * 3)
    b = torch.zeros(6)
    b[(CASES.index(case) if case in CASES else 0) % 6] = float(p[4:])
    return b


def _dyadic(g, shape, lo, hi, step):
    """Multiples of `step` (a power of two) in [lo step, hi step)."""
    return torch.randint(lo, hi, shape, generator=g).float() * step


def _stripes(N, C, h, w):
    x = torch.zeros(N, C, h, w)
    for k in range(6):
        x[:, k, :, k::6] = 64.0
    return x


def candidates(case, g):
    """-> (list of six fp32 [N,3,H,W], the [N,3,2,H,W] pair tensor whose planes candidates 4 and 5 are, or None)."""
    N, H, W = case.N, 2 * case.h, 2 * case.w
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * 1.2
    if case.cand == "equal":
        return [u(N, 3, H, W)] * 6, None
    if case.cand == "near":
        base = u(N, 3, H, W)
        return [base + u(N, 3, H, W) * (0.05 / 1.2) for _ in range(6)], None
    cands = [u(N, 3, H, W) for _ in range(4)]
    pair = u(N, 3, 2, H, W)
    cands += [pair[:, :, 0], pair[:, :, 1]]
    return cands, (pair if case.cand == "pair" else None)


def make(case):
    """-> dict(dec1, enc1, w2, b2 (dec23) or d2 (dec3); w3, b3; cands, pair; t): fp32 CPU tensors."""
    g = _gen(case)
    N, h, w = case.N, case.h, case.w
    d = {}
    exact, stripes = case.regime == "exact", case.pattern == "stripes"
    if exact:
        kind, wkind = None, None
    elif case.regime == "generic":
        kind, wkind = case.pattern.split("/")
    else:
        kind, wkind = "relu", "plain"
    if case.fam == "dec23":
        assert h % 2 == 0 and w % 2 == 0
        if exact:
            d["dec1"] = _dyadic(g, (N, 32, h // 2, w // 2), 0, 2048, 2.0 ** -10)
            d["enc1"] = _dyadic(g, (N, 16, h, w), 0, 2048, 2.0 ** -10)
            d["w2"] = _dyadic(g, (16, 48, 3, 3), -2, 3, 0.25) * (torch.rand(16, 48, 3, 3, generator=g) < 0.25).float()
            d["b2"] = _dyadic(g, (16,), -16, 17, 1.0 / 16)
            if stripes:
                d["enc1"][:, :6] = _stripes(N, 6, h, w)
                d["w2"].zero_()
                d["b2"].zero_()
                for k in range(6):
                    d["w2"][k, 32 + k, 1, 1] = 1.0
        else:
            d["dec1"] = CC.activation(kind, (N, 32, h // 2, w // 2), g)
            d["enc1"] = CC.activation(kind, (N, 16, h, w), g)
            d["w2"] = CC.weights(SPEC2, wkind, g)
            d["b2"] = torch.randn(16, generator=g) * 0.1 * CC.magnitude(kind)
    else:
        if exact:
            d["d2"] = torch.relu(torch.round(torch.randn(N, 16, h, w, generator=g) * 3 * 4096) / 4096)
            if stripes:
                d["d2"] = _stripes(N, 16, h, w)
        else:
            d["d2"] = torch.relu(CC.activation(kind, (N, 16, h, w), g))           # dec2's output is post-ReLU
    if exact:
        d["w3"] = _dyadic(g, (6, 16, 3, 3), -2, 3, 0.25) * 2.0 ** -6
        d["b3"] = _dyadic(g, (6,), -64, 65, 2.0 ** -6)
        if stripes:
            d["w3"].zero_()
            d["b3"].zero_()
            for k in range(6):
                d["w3"][k, k, 1, 1] = 0.5
    elif case.regime == "bias":
        d["w3"] = torch.zeros(6, 16, 3, 3)
        d["b3"] = bias_pattern(case)
    else:
        d["w3"] = CC.weights(SPEC3, wkind, g)
        d["b3"] = torch.randn(6, generator=g) * 0.3
    d["cands"], d["pair"] = candidates(case, g)
    d["t"] = t_values(case)
    return d


def whites(case):
    """The white levels of the rounded forms a dec23 case runs: 255 (the 8-bit form), 1023, and 65535 where the frame bound stays
    below 1 % of a code (synth_float_ref's condition on ill pixels)."""
    return [255, 1023] + ([65535] if case.cand in ("near", "equal") else [])


def crops(case):
    """(Hc, Wc) of the rounded forms: the frame, a crop that cuts the last tile row and column (7 rows and 14 columns short; a tile is
    16 x 64 frame pixels), and 2 x 2."""
    H, W = 2 * case.h, 2 * case.w
    out = []
    for c in ((H, W), (max(2, H - 7), max(2, W - 14)), (2, 2)):
        if c not in out:
            out.append(c)
    return out


def row_limits(case):
    """Row limits of a dec23 case: one tile row (16 frame rows) and a tile boundary +- 1, where the frame has that many rows."""
    H = 2 * case.h
    return [r for r in (15, 16, 17, 31, 32, 33) if r <= H]
