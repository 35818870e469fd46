"""The four converter kernels of the video library ALONE on the GPU (fldr-vfi_amd/video/video_kernels.hip: YUV 4:2:0 -> planar BGR pair
and planar BGR -> YUV 4:2:0, at 8 and at 10 bits, wide-access `VEC` form and per-sample form, NV12 / P010 and I420 / yuv420p10le), through
the hooks of libfldr_video_test.so (include/fldr_video_test_hooks.h, fldr_video.debug_to_planar / debug_from_planar / debug_last_path).
Through fldr_video_forward they only ever see in-gamut frames and what the network emits, at a handful of model-valid sizes; here they get

  (a) every 8-bit (Y, U, V) triple, (b) every 8-bit (B, G, R) triple, (c) every 10-bit value of each channel against the corners of the
  other two, (d) noise and hard edges of extreme codes, (e) a sweep over sizes from 2 x 2, pitches and single misaligned planes with the
  chosen form asserted, the bytes around every output plane guarded by a sentinel and the input gaps filled two ways, and (f) the proof
  that the hooks run the product's converters: a forward's planar pair and output frame are the hooks' bit for bit.

Every comparison is exact, against tests/yuv_oracle.py (depth 8) and tests/yuv_hd_oracle.py (depth 10): no tolerance, no skipped position.
The coverage statements of (a) - (c) and the expected form of (e) are conditions on the test's own inputs and are asserted on the CPU next
to the GPU comparisons.  What costs is the numpy oracle, not the GPU.

Measured wall time of this file on one MI355X box (16 host threads): 34 s for its 37 tests (the 8-bit exhaustive input frames 3.4 - 4.0 s
per format, the output ones 1.9 - 2.4 s, each size sweep under 1 s); tests/test_gpu_video.py alone takes about as long."""
import functools
import os

import numpy as np
import pytest
import torch

import yuv_hd_oracle as HD
import yuv_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = [(m, r) for m in HD.MATRICES for r in HD.RANGES]
LAYOUTS = ("nv12", "i420")
BASE = 64                                  # byte offset of an "aligned" plane in its buffer: there is a "before" to guard


@pytest.fixture(scope="module")
def V(dev):
    import fldr_video
    fldr_video.test_hooks()
    return fldr_video


def _fmt(V, layout, mat, rng, depth):
    return V.Format(layout, mat, rng, depth)


def _oracle(depth):
    """(yuv420_to_bgr, bgr_to_yuv420, yuv444_to_rgb, rgb_to_yuv444) of the oracle of this depth, all as f(..., mat, rng)."""
    if depth == 8:
        return O.yuv420_to_bgr, O.bgr_to_yuv420, O.yuv444_to_rgb, O.rgb_to_yuv444
    return (lambda Y, U, Vp, m, r: HD.yuv420_to_bgr(Y, U, Vp, m, r, 10), lambda b, m, r: HD.bgr_to_yuv420(b, m, r, 10),
            lambda Y, U, Vp, m, r: HD.yuv444_to_rgb(Y, U, Vp, m, r, 10), lambda R, G, B, m, r: HD.rgb_to_yuv444(R, G, B, m, r, 10))


# ---- planes in guarded byte buffers -----------------------------------------------------------------------------------------------
def _upload(host, dev):
    return torch.from_numpy(host).to(dev)


def _body(host, off, pitch, rows, rb):
    return np.lib.stride_tricks.as_strided(host[off:], (rows, rb), (pitch, 1))


def _place(plane, dev, off=0, pitch=None, fill=0):
    """A host plane of container words (uint8 / uint16, [rows, cols]) as a device view `off` bytes into a byte buffer filled with `fill`,
    rows `pitch` bytes apart.  -> (view, buffer, (off, pitch, rows, row bytes, dtype))."""
    plane = np.ascontiguousarray(plane)
    rows, cols = plane.shape
    rb = cols * plane.itemsize
    pitch = rb if pitch is None else pitch
    assert pitch >= rb and off % plane.itemsize == 0 and pitch % plane.itemsize == 0
    n = off + rows * pitch + 64
    host = np.full(n, fill, np.uint8)
    _body(host, off, pitch, rows, rb)[:] = plane.view(np.uint8).reshape(rows, rb)
    buf = _upload(host, dev)
    assert buf.data_ptr() % 256 == 0, "device allocations are 256-byte aligned: the offsets of this file are the planes' alignment"
    if plane.itemsize == 1:
        view = buf.as_strided((rows, cols), (pitch, 1), off)
    else:
        view = buf.view(torch.uint16).as_strided((rows, cols), (pitch // 2, 1), off // 2)
    return view, buf, (off, pitch, rows, rb, plane.dtype)


def _fetch(buf, geom, fill=None):
    """The plane back on the host; with `fill`: every byte of the buffer outside the plane's rows must still hold it."""
    off, pitch, rows, rb, dtype = geom
    host = buf.cpu().numpy()
    plane = np.ascontiguousarray(_body(host, off, pitch, rows, rb)).view(dtype)
    if fill is not None:
        outside = np.ones(host.size, bool)
        outside[(off + np.arange(rows)[:, None] * pitch + np.arange(rb)[None, :]).ravel()] = False
        touched = np.flatnonzero(outside & (host != fill))
        assert touched.size == 0, "bytes outside the plane's rows were written: buffer offsets %s (plane at %d, pitch %d, %d x %d bytes)" % (
            touched[:8], off, pitch, rows, rb)
    return plane


def _frame_to_dev(planes, dev):
    return tuple(_place(p, dev)[0] for p in planes)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if np.array_equal(got, want):
        return
    bad = np.argwhere(got != want)
    first = tuple(bad[0])
    pytest.fail("%s: %d of %d samples differ; first at %s: got %d, want %d; mismatches by x %% 4: %s" % (
        what, len(bad), got.size, first, int(got[first]), int(want[first]), np.bincount(bad[:, -1] % 4, minlength=4).tolist()))


def _vec_rule(W, depth, views):
    """The path choice as video_kernels.hip states it: W % 4 == 0 and every plane pointer and pitch 4-byte (depth 8) / 8-byte (depth 10)
    aligned (the planar side is 256-byte aligned by the hooks' contract)."""
    a = 4 if depth == 8 else 8
    return W % 4 == 0 and all(v.data_ptr() % a == 0 and (v.stride(0) * v.element_size()) % a == 0 for v in views)


def _to_planar(V, frames, fmt):
    pair = V.debug_to_planar(frames, fmt)
    torch.cuda.synchronize()
    return pair.cpu().numpy(), V.debug_last_path()


def _planar_dev(bgr, dev):
    t = _upload(np.ascontiguousarray(bgr), dev)
    assert t.data_ptr() % 256 == 0
    return t


def _from_planar(V, planar_dev, fmt, out_views):
    V.debug_from_planar(planar_dev, fmt, out=out_views)
    torch.cuda.synchronize()
    return V.debug_last_path()


def _container_ok(planes, layout, depth):
    """Depth 10: P010 words have their low six bits zero, yuv420p10le words are <= 1023."""
    if depth == 10:
        for p in planes:
            assert (int((p & 63).max()) == 0) if layout == "nv12" else (int(p.max()) <= 1023), layout


def _convert_in(V, dev, yuv_pair, layout, mat, rng, depth, dirt=None):
    """Two frames of code-value planes -> the GPU's planar pair (tight planes), and the form taken."""
    frames = [_frame_to_dev(HD.pack_planes(*yuv, layout, depth, dirt=dirt), dev) for yuv in yuv_pair]
    got, path = _to_planar(V, frames, _fmt(V, layout, mat, rng, depth))
    assert path == int(_vec_rule(yuv_pair[0][0].shape[1], depth, frames[0] + frames[1]))
    return got


def _convert_out(V, dev, bgr, layout, mat, rng, depth):
    """One planar BGR frame -> the GPU's (Y, U, V) code values (tight planes; the container's unused bits checked)."""
    H, W = bgr.shape[1:]
    dt = HD.dtype_of(depth)
    placed = [_place(np.zeros(s, dt), dev, off=BASE, fill=0xA5) for s in V.plane_shapes(layout, H, W)]
    path = _from_planar(V, _planar_dev(bgr, dev), _fmt(V, layout, mat, rng, depth), tuple(p[0] for p in placed))
    assert path == int(_vec_rule(W, depth, [p[0] for p in placed]))
    planes = [_fetch(buf, geom, fill=0xA5) for _, buf, geom in placed]
    _container_ok(planes, layout, depth)
    return HD.unpack_planes(planes, layout, depth)


# ---- tap indices of the definition (chroma sample (i, j) at luma (2i, 2j + 1/2)), written out here for the purity masks ------------
def _up_taps(n, cn, vertical):
    """Chroma indices the upsampling reads for luma index 0 .. n-1 along one axis: (first, second)."""
    p = np.arange(n)
    if vertical:                                                         # even y: rows y/2 - 1, y/2; odd y: (y-1)/2, (y+1)/2
        a, b = np.where(p % 2 == 0, p // 2 - 1, (p - 1) // 2), np.where(p % 2 == 0, p // 2, (p + 1) // 2)
    else:                                                                # even x: column x/2 twice; odd x: (x-1)/2, (x+1)/2
        a, b = np.where(p % 2 == 0, p // 2, (p - 1) // 2), np.where(p % 2 == 0, p // 2, (p + 1) // 2)
    return np.clip(a, 0, cn - 1), np.clip(b, 0, cn - 1)


def _pure_up(n, cn, block):
    """(along x, along y): luma indices whose two chroma taps both lie in the chroma block (`block` samples) under their own luma block."""
    a, b = _up_taps(n, cn, vertical=False), _up_taps(n, cn, vertical=True)
    own = np.arange(n) // (2 * block)
    return (a[0] // block == own) & (a[1] // block == own), (b[0] // block == own) & (b[1] // block == own)


def _down_taps(cn, n, vertical):
    """Luma indices the downsampling reads for chroma index 0 .. cn-1 along one axis."""
    i = np.arange(cn)
    if vertical:
        return [2 * i, np.minimum(2 * i + 1, n - 1)]
    return [np.clip(2 * i - 1, 0, n - 1), 2 * i, np.minimum(2 * i + 1, n - 1)]


def _pure_down(cn, n, block, vertical):
    """(chroma indices along one axis whose luma taps all lie in one luma block of `block` pixels, that block's index)."""
    taps = _down_taps(cn, n, vertical)
    own = taps[0 if vertical else 1] // block
    ok = np.ones(cn, bool)
    for t in taps:
        ok &= t // block == own
    return ok, own


# ---- (a) every 8-bit (Y, U, V) triple through the input kernel ----------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _all_yuv_frames():
    """Two 4096 x 4096 frames: chroma constant over 8 x 8-sample blocks (U = block column, V = block row), each 16 x 16 luma block
    holding all 256 Y values: in frame 0 as 16 ly + lx, in frame 1 permuted so that the 46 values frame 0 has on impure positions (local
    column 15, local rows 0 and 15) come first on frame 1's pure positions (a cyclic shift by (8, 8) does not do: four values per block
    stay impure, a full impure column always crosses the other arrangement's impure rows).  -> (frames, pure mask [4096, 4096])."""
    n = 4096
    c = np.arange(n // 2) // 8
    U = np.ascontiguousarray(np.broadcast_to(c[None, :], (n // 2, n // 2)).astype(np.uint8))
    Vp = np.ascontiguousarray(np.broadcast_to(c[:, None], (n // 2, n // 2)).astype(np.uint8))
    px, py = _pure_up(n, n // 2, 8)
    pure = py[:, None] & px[None, :]
    inner = pure[16:32, 16:32].ravel()                                     # an inner block: 210 pure positions
    arr0 = np.arange(256)
    arr1 = np.empty(256, np.int64)
    arr1[np.argsort(~inner, kind="stable")] = np.argsort(inner, kind="stable")     # pure positions first <- frame 0's impure values first
    l = np.arange(n) % 16
    frames = [(a.reshape(16, 16)[l[:, None], l[None, :]].astype(np.uint8), U, Vp) for a in (arr0, arr1)]
    return frames, pure


def _yuv_codes(Y):
    b = np.arange(4096, dtype=np.uint32) // 16
    return (Y.astype(np.uint32) << 16) | (b[None, :] << 8) | b[:, None]      # Y, U = block column, V = block row


def test_the_two_arrangements_put_every_triple_on_a_pure_pixel():
    """The condition on the inputs of (a), on the CPU alone: 210 pure positions per block (local column 15 and local rows 0 and 15 are
    not), one arrangement leaves 46 Y values per block uncovered, the two together cover all 2^24 (Y, U, V) triples."""
    frames, pure = _all_yuv_frames()
    blk = pure[16:32, 16:32]
    assert int(blk.sum()) == 210 and not blk[:, 15].any() and not blk[0].any() and not blk[15].any()
    seen = np.zeros(1 << 24, bool)
    seen[_yuv_codes(frames[0][0])[pure]] = True
    assert 45 << 16 < int((~seen).sum()) <= 46 << 16                     # 46 per block, fewer in the blocks on the frame's clamped edges
    seen[_yuv_codes(frames[1][0])[pure]] = True
    assert seen.all(), "%d triples are on no pure pixel" % int((~seen).sum())


@pytest.mark.parametrize("mat,rng", FORMATS)
def test_every_8_bit_yuv_triple_through_the_input_kernel(V, dev, mat, rng):
    frames, pure = _all_yuv_frames()
    seen = np.zeros(1 << 24, bool)
    b = np.arange(4096, dtype=np.uint32) // 16
    want = np.empty((2, 3, 4096, 4096), np.uint8)
    for f, (Y, U, Vp) in enumerate(frames):
        seen[_yuv_codes(Y)[pure]] = True
        want[f] = O.yuv420_to_bgr(Y, U, Vp, mat, rng)
        # a pure pixel is the 4:4:4 conversion of its triple
        ys = Y[pure]
        us = np.broadcast_to(b[None, :], Y.shape)[pure]
        vs = np.broadcast_to(b[:, None], Y.shape)[pure]
        R, G, B = O.yuv444_to_rgb(ys, us, vs, mat, rng)
        for c, ref in enumerate((B, G, R)):
            assert np.array_equal(want[f, c][pure], ref)
    assert seen.all()                                                    # before any GPU call: all 2^24 triples sit on pure pixels
    for layout in LAYOUTS:
        got = _convert_in(V, dev, frames, layout, mat, rng, 8)
        _same(got, want, "all (Y, U, V) triples, %s %s %s" % (layout, mat, rng))
        for f in range(2):
            for c in range(3):
                assert np.array_equal(got[f, c][pure], want[f, c][pure])    # the pure pixels: yuv444_to_rgb of their triple (shown above)


# ---- (b) every 8-bit (B, G, R) triple through the output kernel ---------------------------------------------------------------------
CHROMA_SET = np.unique(np.concatenate([[0, 1, 254, 255], np.round(np.linspace(2, 253, 60)).astype(np.int64)]))


@functools.lru_cache(maxsize=1)
def _all_bgr_frames():
    """(a 4096 x 4096 frame holding a seeded permutation of all 2^24 triples, a frame of constant 4 x 2 blocks holding every triple over
    CHROMA_SET^3, one block each)."""
    perm = np.random.default_rng(24).permutation(1 << 24).astype(np.uint32).reshape(4096, 4096)
    full = np.stack([(perm & 255), (perm >> 8) & 255, perm >> 16]).astype(np.uint8)
    n = len(CHROMA_SET)
    t = np.arange(n ** 3).reshape(n * n // 8, 8 * n)                       # block grid: 512 x 512 for 64 values
    blocks = np.stack([CHROMA_SET[t % n], CHROMA_SET[(t // n) % n], CHROMA_SET[t // (n * n)]]).astype(np.uint8)     # B, G, R
    return full, np.ascontiguousarray(blocks.repeat(2, axis=1).repeat(4, axis=2))


@pytest.mark.parametrize("mat,rng", FORMATS)
def test_every_8_bit_bgr_triple_through_the_output_kernel(V, dev, mat, rng):
    full, blocks = _all_bgr_frames()
    # luma is per pixel: all 2^24 triples are pixels of `full`
    seen = np.zeros(1 << 24, bool)
    seen[(full[2].astype(np.uint32) << 16) | (full[1].astype(np.uint32) << 8) | full[0]] = True
    assert seen.all()
    want_full = O.bgr_to_yuv420(full, mat, rng)
    y444 = O.rgb_to_yuv444(full[2], full[1], full[0], mat, rng)[0]
    assert np.array_equal(want_full[0], y444)
    # chroma: every triple over CHROMA_SET^3 has a chroma sample all of whose six taps read its own block
    n = len(CHROMA_SET)
    assert n >= 64 and {0, 1, 254, 255} <= set(CHROMA_SET.tolist()) and int(np.diff(CHROMA_SET[2:-2]).max()) <= 5
    H, W = blocks.shape[1:]
    ok_i, blk_i = _pure_down(W // 2, W, 4, vertical=False)
    ok_j, blk_j = _pure_down(H // 2, H, 2, vertical=True)
    pure = ok_j[:, None] & ok_i[None, :]
    tid = (blk_j[:, None] * (W // 4) + blk_i[None, :])[pure]               # the block (= triple) index of each pure chroma sample
    assert np.array_equal(np.unique(tid), np.arange(n ** 3))
    Bv, Gv, Rv = CHROMA_SET[tid % n], CHROMA_SET[(tid // n) % n], CHROMA_SET[tid // (n * n)]
    _, u444, v444 = O.rgb_to_yuv444(Rv, Gv, Bv, mat, rng)
    want_blocks = O.bgr_to_yuv420(blocks, mat, rng)
    assert np.array_equal(want_blocks[1][pure], u444) and np.array_equal(want_blocks[2][pure], v444)
    for layout in LAYOUTS:
        for name, bgr, want in (("all (B, G, R) triples", full, want_full), ("constant 4 x 2 blocks", blocks, want_blocks)):
            got = _convert_out(V, dev, bgr, layout, mat, rng, 8)
            for g, w, pl in zip(got, want, "YUV"):
                _same(g, w, "%s, %s %s %s, plane %s" % (name, layout, mat, rng, pl))
        assert np.array_equal(got[1][pure], u444) and np.array_equal(got[2][pure], v444)


# ---- (c) 10-bit values ----------------------------------------------------------------------------------------------------------------
Y_CORNERS = (0, 64, 512, 940, 1023)
C_CORNERS = (0, 64, 512, 960, 1023)
RGB_CORNERS = (0, 1, 512, 1022, 1023)


def _yuv10_requirements():
    """The (Y, U, V) triples (c) promises, as blocks (U, V, the Y values the block must show on pure pixels) and as 30-bit codes."""
    allv = np.arange(1024)
    blocks = []
    for u in C_CORNERS:
        for v in C_CORNERS:
            blocks += [(u, v, allv[k:k + 196]) for k in range(0, 1024, 196)]            # every Y against the chroma corners
    for x in range(1024):
        for c in C_CORNERS:
            blocks += [(x, c, np.array(Y_CORNERS)), (c, x, np.array(Y_CORNERS))]        # every U, every V against the corners of the other two
    allv, cy, cc = np.arange(1024, dtype=np.int64), np.array(Y_CORNERS, dtype=np.int64), np.array(C_CORNERS, dtype=np.int64)
    code = lambda Y, U, Vp: ((Y << 20) | (U << 10) | Vp).ravel()
    promised = np.concatenate([code(*np.meshgrid(allv, cc, cc, indexing="ij")), code(*np.meshgrid(cy, allv, cc, indexing="ij")),
                               code(*np.meshgrid(cy, cc, allv, indexing="ij"))])
    return blocks, promised


@functools.lru_cache(maxsize=1)
def _yuv10_block_frames():
    """Two frames of 16 x 16 luma blocks over constant 8 x 8 chroma blocks, as in (a): a block's promised Y values sit on its 14 x 14
    inner positions (pure: computed from the taps by the test), the rest of its luma is uniform noise; the two frames hold the blocks in
    different seeded orders.  -> (frames, per frame the codes Y << 20 | U << 10 | V of its pure pixels, the promised codes)."""
    blocks, codes = _yuv10_requirements()
    nb = int(np.ceil(np.sqrt(len(blocks))))
    n = 16 * nb
    g = np.random.default_rng(1010)
    frames, pure_codes = [], []
    px, py = _pure_up(n, n // 2, 8)
    pure = py[:, None] & px[None, :]
    for f in range(2):
        order = g.permutation(nb * nb)
        Y = g.integers(0, 1024, (n, n)).astype(np.uint16)
        Ub = g.integers(0, 1024, nb * nb)
        Vb = g.integers(0, 1024, nb * nb)
        for k, (u, v, ys) in enumerate(blocks):
            by, bx = divmod(int(order[k]), nb)
            Ub[order[k]], Vb[order[k]] = u, v
            inner = Y[16 * by + 1:16 * by + 15, 16 * bx + 1:16 * bx + 15]
            flat = inner.reshape(-1).copy()
            flat[:len(ys)] = ys
            inner[:] = flat.reshape(14, 14)
        U = np.ascontiguousarray(Ub.reshape(nb, nb).repeat(8, axis=0).repeat(8, axis=1).astype(np.uint16))
        Vp = np.ascontiguousarray(Vb.reshape(nb, nb).repeat(8, axis=0).repeat(8, axis=1).astype(np.uint16))
        frames.append((Y, U, Vp))
        Uf = Ub.reshape(nb, nb).repeat(16, axis=0).repeat(16, axis=1)
        Vf = Vb.reshape(nb, nb).repeat(16, axis=0).repeat(16, axis=1)
        pure_codes.append(np.unique(((Y.astype(np.int64) << 20) | (Uf << 10) | Vf)[pure]))
    return frames, pure, pure_codes, codes


def _uniform_yuv(H, W, depth, seed):
    g = np.random.default_rng(seed)
    ch, cw = HD.chroma_size(H, W)
    dt = HD.dtype_of(depth)
    return tuple(g.integers(0, 1 << depth, s).astype(dt) for s in ((H, W), (ch, cw), (ch, cw)))


@pytest.mark.parametrize("mat,rng", FORMATS)
def test_10_bit_value_sweeps_through_the_input_kernel(V, dev, mat, rng):
    frames, pure, pure_codes, codes = _yuv10_block_frames()
    assert len(codes) == 3 * 1024 * 25
    for f in range(2):
        assert np.isin(codes, pure_codes[f]).all(), "frame %d: a promised (Y, U, V) is on no pure pixel" % f
    assert frames[0][0].shape[0] <= 4096
    uniform = [_uniform_yuv(2048, 2048, 10, seed) for seed in (31, 32)]
    dirt = np.random.default_rng(77)
    for name, pair in (("block frames", frames), ("uniform planes", uniform)):
        want = np.stack([HD.yuv420_to_bgr(*yuv, mat, rng, 10) for yuv in pair])
        if pair is frames:                                               # a pure pixel is the 4:4:4 conversion of its triple
            for f, (Y, U, Vp) in enumerate(pair):
                Uf, Vf = U.repeat(2, axis=0).repeat(2, axis=1), Vp.repeat(2, axis=0).repeat(2, axis=1)     # constant blocks: the block's value
                R, G, B = HD.yuv444_to_rgb(Y[pure], Uf[pure], Vf[pure], mat, rng, 10)
                for c, ref in enumerate((B, G, R)):
                    assert np.array_equal(want[f, c][pure], ref)
        for layout in LAYOUTS:
            got = _convert_in(V, dev, pair, layout, mat, rng, 10, dirt=dirt)
            _same(got, want, "10-bit %s, %s %s %s" % (name, layout, mat, rng))


def _bgr10_requirements():
    allv = np.arange(1024)
    cs = np.array(RGB_CORNERS)
    A, P, Q = (a.ravel() for a in np.meshgrid(allv, cs, cs, indexing="ij"))
    B = np.concatenate([A, P, P])
    G = np.concatenate([P, A, Q])
    R = np.concatenate([Q, Q, A])
    return B, G, R


@functools.lru_cache(maxsize=1)
def _bgr10_block_frame():
    """Constant 4 x 2 blocks: every value 0 .. 1023 of each of B, G, R against every pair of RGB_CORNERS in the other two."""
    B, G, R = _bgr10_requirements()
    cols = 320
    rows = -(-len(B) // cols)
    g = np.random.default_rng(3)
    trip = g.integers(0, 1024, (3, rows * cols))
    trip[:, :len(B)] = np.stack([B, G, R])
    trip = trip[:, g.permutation(rows * cols)]
    return np.ascontiguousarray(trip.reshape(3, rows, cols).repeat(2, axis=1).repeat(4, axis=2).astype(np.uint16))


@pytest.mark.parametrize("mat,rng", FORMATS)
def test_10_bit_value_sweeps_through_the_output_kernel(V, dev, mat, rng):
    blocks = _bgr10_block_frame()
    H, W = blocks.shape[1:]
    assert H <= 4096 and W <= 4096
    ok_i, blk_i = _pure_down(W // 2, W, 4, vertical=False)
    ok_j, blk_j = _pure_down(H // 2, H, 2, vertical=True)
    pure = ok_j[:, None] & ok_i[None, :]
    sample = blocks[:, ::2, ::4].astype(np.int64)                           # one value per block
    Bp, Gp, Rp = (sample[c][blk_j[:, None], blk_i[None, :]][pure] for c in range(3))
    have = np.unique((Bp << 20) | (Gp << 10) | Rp)
    B, G, R = _bgr10_requirements()
    assert np.isin((B.astype(np.int64) << 20) | (G << 10) | R, have).all(), "a promised (B, G, R) has no pure chroma sample"
    y444, u444, v444 = HD.rgb_to_yuv444(Rp, Gp, Bp, mat, rng, 10)
    want_blocks = HD.bgr_to_yuv420(blocks, mat, rng, 10)
    assert np.array_equal(want_blocks[1][pure], u444) and np.array_equal(want_blocks[2][pure], v444)
    uniform = np.random.default_rng(41).integers(0, 1024, (3, 2048, 2048)).astype(np.uint16)
    want_uniform = HD.bgr_to_yuv420(uniform, mat, rng, 10)
    for layout in LAYOUTS:
        for name, bgr, want in (("uniform planes", uniform, want_uniform), ("constant 4 x 2 blocks", blocks, want_blocks)):
            got = _convert_out(V, dev, bgr, layout, mat, rng, 10)
            for g_, w, pl in zip(got, want, "YUV"):
                _same(g_, w, "10-bit %s, %s %s %s, plane %s" % (name, layout, mat, rng, pl))
        assert np.array_equal(got[1][pure], u444) and np.array_equal(got[2][pure], v444)


# ---- (d) noise and hard edges ---------------------------------------------------------------------------------------------------------
def _extremes(depth):
    e = np.array([0, 1, 15, 16, 235, 240, 254, 255])
    return e if depth == 8 else np.concatenate([4 * e, [1023]])


def _rectangles(shape, depth, g, n=160):
    """A plane that takes only extreme codes, in random rectangles (hard edges in both directions, down to single samples)."""
    e = _extremes(depth)
    h, w = shape
    p = np.full(shape, e[g.integers(len(e))], HD.dtype_of(depth))
    for _ in range(n):
        y0, x0 = int(g.integers(h)), int(g.integers(w))
        p[y0:y0 + int(g.integers(1, max(h // 3, 2))), x0:x0 + int(g.integers(1, max(w // 3, 2)))] = e[g.integers(len(e))]
    return p


def _content(kind, shapes, depth, seed):
    g = np.random.default_rng(seed)
    if kind == "noise":
        return [g.integers(0, 1 << depth, s).astype(HD.dtype_of(depth)) for s in shapes]
    return [_rectangles(s, depth, g) for s in shapes]


@pytest.mark.parametrize("H,W", [(1080, 1920), (271, 487)])
@pytest.mark.parametrize("kind", ["noise", "edges"])
@pytest.mark.parametrize("depth", [8, 10])
def test_noise_and_hard_edges(V, dev, depth, kind, H, W):
    to_bgr, to_yuv, _, _ = _oracle(depth)
    ch, cw = HD.chroma_size(H, W)
    yuv_pair = [tuple(_content(kind, [(H, W), (ch, cw), (ch, cw)], depth, 100 * depth + f)) for f in range(2)]
    bgr = np.stack(_content(kind, [(H, W)] * 3, depth, 7 * depth))
    dirt = np.random.default_rng(5) if depth == 10 else None
    on_clamp = []
    for mat, rng in FORMATS:
        want_pair = np.stack([to_bgr(*yuv, mat, rng) for yuv in yuv_pair])
        on_clamp.append(float(np.mean((want_pair == 0) | (want_pair == (1 << depth) - 1))))
        want_yuv = to_yuv(bgr, mat, rng)
        for layout in LAYOUTS:
            what = "%s %d-bit %dx%d %s %s %s" % (kind, depth, H, W, layout, mat, rng)
            _same(_convert_in(V, dev, yuv_pair, layout, mat, rng, depth, dirt=dirt), want_pair, what + " -> BGR")
            for g_, w, pl in zip(_convert_out(V, dev, bgr, layout, mat, rng, depth), want_yuv, "YUV"):
                _same(g_, w, what + " -> " + pl)
    print("%s, depth %d, %dx%d: share of the oracle's BGR samples on a clamp, per format: %s" % (kind, depth, H, W, ["%.3f" % c for c in on_clamp]))
    assert min(on_clamp) > 0.1                                           # such input does drive the clamps


# ---- (e) sizes, pitches and alignment ---------------------------------------------------------------------------------------------------
SWEEP_H = (2, 3, 4, 5, 7, 8, 9, 201, 256)
SWEEP_W = (2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 254, 255, 256, 257, 258, 260, 1023, 1024, 1026)


def _row_bytes(layout, depth, W):
    b, cw = depth // 8 if depth == 8 else 2, (W + 1) // 2
    return [b * W, b * 2 * cw] if layout == "nv12" else [b * W, b * cw, b * cw]


def _sweep_cases(layout, depth, W):
    """[(name, (offsets, pitches) of the frame under test, (offsets, pitches) of an aligned frame, expected form)], bytes per plane.  The
    output kernel gets the first geometry; the input kernel gets it for one of its two frames and the aligned one for the other, so a
    single plane of a single frame decides the form."""
    a, b = (4, 1) if depth == 8 else (8, 2)
    rb = _row_bytes(layout, depth, W)
    npl = len(rb)
    base = [BASE] * npl
    tight = (base, list(rb))
    if W % 4:
        odd = ([BASE + b] * npl, [r + 3 * b for r in rb])
        return [("tight", tight, tight, 0), ("odd pitch, odd address", odd, odd, 0)]
    padded = (base, [(r + a - 1) // a * a + 2 * a for r in rb])
    cases = [("tight", tight, tight, int(all(r % a == 0 for r in rb))), ("padded", padded, padded, 1)]
    for p in range(npl):
        for d in ((1, 2) if depth == 8 else (2, 4)):
            off, pit = list(base), list(padded[1])
            off[p] += d
            pit[p] += d
            cases.append(("plane %d moved %d bytes" % (p, d), (off, padded[1]), padded, 0))
            cases.append(("plane %d pitch + %d bytes" % (p, d), (base, pit), padded, 0))
    return cases


def _place_frame(planes, dev, offs, pitches, fill):
    placed = [_place(p, dev, off=o, pitch=q, fill=fill) for p, o, q in zip(planes, offs, pitches)]
    return tuple(p[0] for p in placed), placed


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("depth", [8, 10])
def test_input_kernel_over_sizes_pitches_and_alignments(V, dev, depth, layout):
    to_bgr = _oracle(depth)[0]
    seen, n = {0: 0, 1: 0}, 0
    for hi, H in enumerate(SWEEP_H):
        for wi, W in enumerate(SWEEP_W):
            pair = [_uniform_yuv(H, W, depth, 1000 * H + W + f) for f in range(2)]
            cases = _sweep_cases(layout, depth, W)
            wants = {}
            for ci, (name, geom, aligned, expect) in enumerate(cases):
                mat, rng = FORMATS[(hi + wi + ci) % 4]
                if (mat, rng) not in wants:
                    wants[(mat, rng)] = np.stack([to_bgr(*yuv, mat, rng) for yuv in pair])
                results = []
                for fill in (0x00, 0xFF):                                # the bytes between, before and behind the input rows
                    dirt = np.random.default_rng(ci) if depth == 10 else None
                    frames = []
                    for f in range(2):
                        offs, pitches = geom if f == ci % 2 else aligned
                        frames.append(_place_frame(HD.pack_planes(*pair[f], layout, depth, dirt=dirt), dev, offs, pitches, fill)[0])
                    got, path = _to_planar(V, frames, _fmt(V, layout, mat, rng, depth))
                    what = "%dx%d %s depth %d, %s (%s %s)" % (H, W, layout, depth, name, mat, rng)
                    assert path == expect == int(_vec_rule(W, depth, frames[0] + frames[1])), what
                    _same(got, wants[(mat, rng)], what)
                    results.append(got)
                assert np.array_equal(results[0], results[1])                # the gap bytes of the input have no effect
                seen[expect] += 1
                n += 1
    print("input sweep, %s depth %d: %d cases, %d on the VEC form, %d per sample" % (layout, depth, n, seen[1], seen[0]))
    assert seen[0] > 50 and seen[1] > 50                                 # the sweep did not end up on one form only


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("depth", [8, 10])
def test_output_kernel_over_sizes_pitches_and_alignments(V, dev, depth, layout):
    to_yuv = _oracle(depth)[1]
    dt = HD.dtype_of(depth)
    seen, n = {0: 0, 1: 0}, 0
    for hi, H in enumerate(SWEEP_H):
        for wi, W in enumerate(SWEEP_W):
            bgr = np.random.default_rng(1000 * H + W).integers(0, 1 << depth, (3, H, W)).astype(dt)
            planar = _planar_dev(bgr, dev)
            wants = {}
            for ci, (name, (offs, pitches), _, expect) in enumerate(_sweep_cases(layout, depth, W)):
                mat, rng = FORMATS[(hi + wi + ci) % 4]
                if (mat, rng) not in wants:
                    wants[(mat, rng)] = to_yuv(bgr, mat, rng)
                for fill in (0xA5, 0x5A):                                # the sentinel around the planes (and under them, before the call)
                    views, placed = _place_frame([np.full(s, fill * 0x0101 if depth == 10 else fill, dt) for s in V.plane_shapes(layout, H, W)],
                                                 dev, offs, pitches, fill)
                    path = _from_planar(V, planar, _fmt(V, layout, mat, rng, depth), views)
                    what = "%dx%d %s depth %d, %s (%s %s)" % (H, W, layout, depth, name, mat, rng)
                    assert path == expect == int(_vec_rule(W, depth, views)), what
                    planes = [_fetch(buf, geom, fill=fill) for _, buf, geom in placed]
                    _container_ok(planes, layout, depth)
                    for g_, w, pl in zip(HD.unpack_planes(planes, layout, depth), wants[(mat, rng)], "YUV"):
                        _same(g_, w, what + ", plane " + pl)
                seen[expect] += 1
                n += 1
    print("output sweep, %s depth %d: %d cases, %d on the VEC form, %d per sample" % (layout, depth, n, seen[1], seen[0]))
    assert seen[0] > 50 and seen[1] > 50


# ---- (f) the hooks run the product's converters -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nv(dev):
    import fldr_harness as Hn
    import fldr_model
    import fldr_video
    nm = fldr_model.NativeModel.from_npz(Hn.DEFAULT_WEIGHTS, device=dev.index or 0)
    yield fldr_video.NativeVideo(nm)
    nm.close()


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.uint16 else t


@pytest.mark.parametrize("H,W", [(256, 256), (201, 333)])
@pytest.mark.parametrize("depth", [8, 10])
def test_a_forwards_conversions_are_the_hooks_bit_for_bit(V, nv, dev, depth, H, W):
    import fldr_harness as Hn
    to_yuv = _oracle(depth)[1]
    u8 = Hn.synthetic_pair(H, W, seed=3).numpy()
    bgr = u8 if depth == 8 else (u8.astype(np.uint16) * 4 + np.random.default_rng(4).integers(0, 4, u8.shape).astype(np.uint16))
    for li, layout in enumerate(LAYOUTS):
        mat, rng = FORMATS[(li + (H & 1) + depth // 10) % 4]
        fmt = _fmt(V, layout, mat, rng, depth)
        frames = [_frame_to_dev(HD.pack_planes(*to_yuv(bgr[i], mat, rng), layout, depth), dev) for i in range(2)]
        ws = nv.workspace(H, W, 1)
        outs = nv.forward(frames, [0.5], fmt, fmt, ws=ws)
        torch.cuda.synchronize()
        pair, planar = nv.planar(ws, H, W, 1, depth, depth)
        assert pair.data_ptr() % 256 == 0 and planar[0].data_ptr() % 256 == 0
        hook_pair = V.debug_to_planar(frames, fmt)
        hook_out = V.debug_from_planar(planar[0], fmt)
        torch.cuda.synchronize()
        assert torch.equal(_bits(hook_pair), _bits(pair)), (layout, "the input conversion")
        for a, b in zip(hook_out, outs[0]):
            assert torch.equal(_bits(a), _bits(b)), (layout, "the output conversion")
        assert not bool((_bits(outs[0][0]) == 0).all())
