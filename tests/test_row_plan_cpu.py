"""fldr_synth_row_plan (csrc/row_plan.h) against an independent model of the fused synthesis path, no GPU.

The plan is derived BACKWARDS from the crop.  The model here runs FORWARDS: given the plan's counts it works out, stage by stage, which
rows every kernel would write and how many leading rows of each tensor come out RIGHT, from the layer shapes of fLDRnet.py (3x3 pad 1,
4x4 stride 2 pad 1, nearest x2) and the kernels' tile heights, and then asks whether the shown rows of the frame are right.  Two kinds of
reader: dec23_synth and the 3x3 ring convolutions read every row their active tiles reach (such a row must have been written); the
stride-2 encoders are given the number of rows their source holds and treat everything below as zero padding (they never read an
unwritten row, but an output row whose window reaches the padding is wrong)."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fldr-vfi_amd"))

STAGES = ("prep2", "splat", "enc1", "enc2", "enc3", "dec0", "dec1", "dec23")
TILE = {"prep2": 4, "splat": 24, "enc1": 8, "enc2": 8, "enc3": 8, "dec0": 8, "dec1": 8, "dec23": 16}
HEIGHTS = tuple(range(256, 2305, 256)) + (8, 24, 264, 328, 1096)      # + heights whose halves, quarters or eighths are odd or hold less than a tile


def full_rows(H):
    return {"prep2": H, "splat": H, "enc1": H // 2, "enc2": H // 4, "enc3": H // 8, "dec0": H // 8, "dec1": H // 4, "dec23": H}


@pytest.fixture(scope="module")
def plan():
    import fldr_hip
    lib = fldr_hip.lib()

    def get(H, Hc):
        p = fldr_hip.SynthRows()
        rc = lib.fldr_synth_row_plan(H, Hc, ctypes.byref(p))
        assert rc == 0, (H, Hc, rc)
        return {k: int(getattr(p, k)) for k in STAGES}
    return get


def written(count, tile, full):
    """Rows a launch limited to `count` writes: whole tile rows, clipped to the tensor."""
    return min(full, -(-count // tile) * tile)


def s2_right(out_written, src_right, src_written, src_full):
    """Leading output rows of a 4x4 stride-2 pad-1 convolution that are right: row r reads source rows 2r-1 .. 2r+2 (inside the
    tensor), all of which must be right.  Called with src_rows = src_written: nothing at or below that row is read."""
    assert src_right <= src_written <= src_full
    return leading(out_written, lambda r: min(2 * r + 2, src_full - 1) < src_right)


def leading(n, ok):
    """How many of the rows 0 .. n-1 pass `ok`, counted from the top until the first that does not."""
    r = 0
    while r < n and ok(r):
        r += 1
    return r


def check(H, Hc, p):
    """-> None, or a string saying what goes wrong with plan `p` for an H-row frame shown down to row Hc."""
    F = full_rows(H)
    h2, h4, h8 = H // 2, H // 4, H // 8
    W = {k: written(p[k], TILE[k], F[k]) for k in STAGES}
    for k in STAGES:
        if not 0 < p[k] <= F[k]:
            return "%s: %d rows of a %d-row tensor" % (k, p[k], F[k])
    if W["dec23"] < Hc:
        return "the frame stops at row %d" % W["dec23"]
    # ---- every row an active tile of a strict reader reaches has been written ----
    R = -(-p["dec23"] // 16)                                     # dec23: tile rows; tile row k reads enc1 rows 8k-2 .. 8k+9, dec1 rows 4k-1 .. 4k+4
    if min(h2 - 1, 8 * R + 1) >= W["enc1"]:
        return "dec23 reads enc1 row %d of %d" % (min(h2 - 1, 8 * R + 1), W["enc1"])
    if min(h4 - 1, 4 * R) >= W["dec1"]:
        return "dec23 reads dec1 row %d of %d" % (min(h4 - 1, 4 * R), W["dec1"])
    if min(H - 1, 16 * R - 1) >= min(W["splat"], W["prep2"]):
        return "the blend reads candidate row %d of %d" % (min(H - 1, 16 * R - 1), min(W["splat"], W["prep2"]))
    low = min(h4 - 1, W["dec1"])                                 # dec1: rows < n read rows <= n of enc2 and rows <= n >> 1 of dec0
    if low >= W["enc2"]:
        return "dec1 reads enc2 row %d of %d" % (low, W["enc2"])
    if (low >> 1) >= W["dec0"]:
        return "dec1 reads dec0 row %d of %d" % (low >> 1, W["dec0"])
    if min(h8 - 1, W["dec0"]) >= W["enc3"]:
        return "dec0 reads enc3 row %d of %d" % (min(h8 - 1, W["dec0"]), W["enc3"])
    # ---- how many leading rows are right ----
    right_f = min(W["splat"], W["prep2"])                        # the frame-resolution planes: what is written is right
    right_e1 = s2_right(W["enc1"], right_f, right_f, H)
    right_e2 = s2_right(W["enc2"], right_e1, W["enc1"], h2)
    right_e3 = s2_right(W["enc3"], right_e2, W["enc2"], h4)
    right_d0 = leading(W["dec0"], lambda r: min(r + 1, h8 - 1) < right_e3)                 # 3x3: row r reads rows r-1 .. r+1
    right_d1 = leading(W["dec1"], lambda r: min(r + 1, h4 - 1) < right_e2 and (min(r + 1, h4 - 1) >> 1) < right_d0)
    # frame row y = half-resolution row i: dec3 reads dec2 rows i-1 .. i+1, dec2 row j reads enc1 rows j-1 .. j+1 and dec1 rows (j-1)>>1 .. (j+1)>>1
    i = (Hc - 1) >> 1
    j = min(i + 1, h2 - 1)
    if min(j + 1, h2 - 1) >= right_e1:
        return "frame row %d needs enc1 row %d, right are %d" % (Hc - 1, min(j + 1, h2 - 1), right_e1)
    if (min(j + 1, h2 - 1) >> 1) >= right_d1:
        return "frame row %d needs dec1 row %d, right are %d" % (Hc - 1, min(j + 1, h2 - 1) >> 1, right_d1)
    if Hc > right_f:
        return "frame row %d needs its candidates, right are %d rows" % (Hc - 1, right_f)
    return None


def test_the_model_catches_a_short_plan(plan):
    """The check is not vacuous: one tile row less of any stage is caught (where the stage is limited at all)."""
    H, Hc = 2304, 2160
    p = plan(H, Hc)
    assert check(H, Hc, p) is None
    for k in STAGES:
        if p[k] < full_rows(H)[k] or k == "dec23":
            q = dict(p)
            q[k] = p[k] - TILE[k]
            assert check(H, Hc, q) is not None, k


@pytest.mark.parametrize("H", HEIGHTS)
def test_every_crop_height_is_covered(plan, H):
    F = full_rows(H)
    prev = None
    for Hc in range(1, H + 1):
        p = plan(H, Hc)
        bad = check(H, Hc, p)
        assert bad is None, (H, Hc, p, bad)
        for k in STAGES:
            assert p[k] == F[k] or p[k] % TILE[k] == 0, (H, Hc, k, p[k])                 # whole tiles, or the tensor
            assert prev is None or p[k] >= prev[k], (H, Hc, k, prev[k], p[k])            # monotone in the crop
        prev = p
    assert prev == F                                                                       # Hc == H: every stage has all its rows


def test_the_4k_plan(plan):
    """3840 x 2160 padded to 2304 rows: the counts of DESIGN section 5 (tile rows: dec23 135 of 144, enc1 137, enc2 69, dec1 68, dec0 35,
    enc3 36 = all, image splat 91 of 96)."""
    assert plan(2304, 2160) == {"prep2": 2184, "splat": 2184, "enc1": 1096, "enc2": 552, "enc3": 288, "dec0": 280, "dec1": 544, "dec23": 2160}
    assert plan(1280, 1080) == {"prep2": 1128, "splat": 1128, "enc1": 568, "enc2": 288, "enc3": 152, "dec0": 144, "dec1": 280, "dec23": 1088}


def test_bad_arguments(plan):
    import fldr_hip
    lib = fldr_hip.lib()
    p = fldr_hip.SynthRows()
    assert lib.fldr_synth_row_plan(256, 0, ctypes.byref(p)) == -1
    assert lib.fldr_synth_row_plan(256, 257, ctypes.byref(p)) == -1
    assert lib.fldr_synth_row_plan(0, 0, ctypes.byref(p)) == -1
    assert lib.fldr_synth_row_plan(256, 8, None) == -1
    assert lib.fldr_synth_row_plan(260, 8, ctypes.byref(p)) == -2                          # not a multiple of 8: no plan
    assert fldr_hip.synth_row_plan(256, 256) is None and fldr_hip.synth_row_plan(260, 100) is None
    assert fldr_hip.synth_row_plan(256, 100).dec23 == 112
