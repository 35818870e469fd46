"""Both sides of the frame-size limits of fldr_field_weave and fldr_interlace_weave.  An accepted call of either library launches a kernel,
so the limits are reached through tests/weave_limits.hip: a stand-alone program over the header that fills both libraries' plane walks
(fldr-vfi_amd/video/weave_walk_host.h), which makes no HIP call and runs without a GPU.  The rules are stated here from the words of
include/fldr_field.h and include/fldr_interlace.h; the program is held to them."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
LAYOUTS = ("nv12", "i420")


def _planes(layout, depth, H, W):
    """(row bytes, rows) of every plane (fldr_video.h)."""
    b, cw = (2 if depth == 10 else 1), (W + 1) // 2
    chroma = [(2 * cw * b, H // 2)] if layout == "nv12" else [(cw * b, H // 2)] * 2
    return [(W * b, H)] + chroma


def _g(row_bytes):
    return (row_bytes + 15) // 16


def field_plane_rule(layout, depth, H, W):
    """fldr_field.h: "with g = ceil(row bytes / 16) of a plane and R its rows, g * g * R / 2 must stay below 2^32"."""
    return all(_g(rb) * _g(rb) * R // 2 < 2 ** 32 for rb, R in _planes(layout, depth, H, W))


def field_sum_rule(layout, depth, H, W):
    """fldr_field.h: "and the sum of g * R / 2 over the planes below 2^31"."""
    return sum(_g(rb) * R // 2 for rb, R in _planes(layout, depth, H, W)) < 2 ** 31


def interlace_plane_rule(layout, depth, H, W):
    """fldr_interlace.h: "a frame is refused ... when g x g x R >= 2^32 = 4294967296 in a plane"."""
    return not any(_g(rb) * _g(rb) * R >= 4294967296 for rb, R in _planes(layout, depth, H, W))


def interlace_sum_rule(layout, depth, H, W):
    """fldr_interlace.h: "or when the planes' g x R sum to more than 2^31 - 1 = 2147483647"."""
    return not sum(_g(rb) * R for rb, R in _planes(layout, depth, H, W)) > 2147483647


RULES = {"field": (field_plane_rule, field_sum_rule), "interlace": (interlace_plane_rule, interlace_sum_rule)}


@pytest.fixture(scope="module")
def takes(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no hipcc"
    exe = str(tmp_path_factory.mktemp("weave_limits") / "weave_limits")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-Wall", "-Wno-unused-function", "-I" + INC, os.path.join(ROOT, "tests", "weave_limits.hip"),
                        "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr

    def run(library, layout, depth, H, W):
        r = subprocess.run([exe, library, layout, str(depth), str(H), str(W)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stdout.strip() in ("accept", "refuse"), (r.returncode, r.stdout, r.stderr)
        want = all(rule(layout, depth, H, W) for rule in RULES[library])
        assert (r.stdout.strip() == "accept") == want, (library, layout, depth, H, W, r.stdout)
        return want
    return run


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("library,depth,last,first", [("field", 8, 741440, 741441), ("field", 10, 370720, 370721),
                                                      ("interlace", 8, 524272, 524273), ("interlace", 10, 262136, 262137)])
def test_the_widest_frame_of_four_rows(takes, library, depth, last, first, layout):
    """At H = 4 the luma plane binds: g * g * 2 < 2^32 gives g <= 46340 for the deinterlacer, g * g * 4 < 2^32 gives g <= 32767 for the
    interlacer; 16 samples a group at depth 8, 8 at depth 10."""
    g_max = {"field": 46340, "interlace": 32767}[library]
    assert last == g_max * (16 if depth == 8 else 8) and first == last + 1
    assert takes(library, layout, depth, 4, last) is True
    assert takes(library, layout, depth, 4, first) is False
    assert RULES[library][1](layout, depth, 4, first)                       # it is the plane's rule that refuses, not the sum's


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_examples_of_the_field_header(takes, layout):
    """"At depth 8 that allows 15360 x 8640 and refuses 16384 x 8640; at depth 10 it allows 8192 x 4320 and refuses 15360 x 8640." """
    assert takes("field", layout, 8, 8640, 15360) is True
    assert takes("field", layout, 8, 8640, 16384) is False
    assert takes("field", layout, 10, 4320, 8192) is True
    assert takes("field", layout, 10, 8640, 15360) is False


def test_the_example_of_the_interlace_header(takes):
    """"7680 x 4320 at depth 10 has g = 960 in plane 0: 960 x 960 x 4320 = 3981312000, inside the limit." """
    assert _g(7680 * 2) == 960
    for layout in LAYOUTS:
        assert takes("interlace", layout, 10, 4320, 7680) is True


@pytest.mark.parametrize("library,H", [("field", 2 ** 31 - 4), ("interlace", 2 ** 30 - 4)])
def test_the_sum_of_the_planes_alone_refuses(takes, library, H):
    """Two groups a row (W = 32, NV12, depth 8) and the tallest frame whose luma plane passes both of its own tests — g * g * rows judged
    is 2^32 - 8 (field) or 2^32 - 16 (interlace), its items are 2^31 - 4 or 2^31 - 8 — : every plane is inside the plane's rule, the luma
    plane alone inside the sum's, and the chroma plane's items carry the sum past 2^31 - 1.  One group a row (W = 16) halves every count
    and the same height is taken."""
    plane_rule, sum_rule = RULES[library]
    assert plane_rule("nv12", 8, H, 32) and not sum_rule("nv12", 8, H, 32)
    rb, R = _planes("nv12", 8, H, 32)[0]
    assert _g(rb) * (R // 2 if library == "field" else R) <= 2 ** 31 - 1
    assert takes(library, "nv12", 8, H, 32) is False
    assert takes(library, "nv12", 8, H, 16) is True
