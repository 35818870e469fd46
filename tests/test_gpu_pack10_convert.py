"""The two converters of libfldr_pack10.so alone (fldr_pack10.to_planar / from_planar) on the GPU, bit for bit against the containers of
tests/yuv_pack10_oracle.py on the colour definition of tests/yuv_chroma_oracle.py: every 10-bit luma value against a chroma grid, noise
and hard vertical edges in all four matrix / range pairs, a size sweep around the per-thread run and the block width with tight, padded
and offset planes, wide rows with a guarded tail, dirt in every ignored bit and spare slot, what is written into them, and the defining
property: the bytes of libfldr_chroma.so's converters on the same samples as yuv422p10le / yuv444p10le."""
import functools

import numpy as np
import pytest
import torch

import yuv_chroma_oracle as C
import yuv_pack10_oracle as P

pytestmark = pytest.mark.gpu

FORMATS = [(m, r) for m in C.MATRICES for r in C.RANGES]
MARK = 0x5A


def _fmt(c, mat="bt709", rng="limited"):
    import fldr_pack10 as V
    return V.Format(c, mat, rng)


def _dev(plane, dev, pad=0, off=0, fill=MARK, pitch=None):
    """A device copy of a host plane as a view into a byte buffer whose other bytes are `fill`: rows `pad` bytes wider than the row (or of
    `pitch` bytes), starting `off` bytes into the buffer.  -> (frame, (buffer, off, rows, row bytes, pitch))."""
    r, c = plane.shape
    rb = c * plane.itemsize
    pitch = pitch or rb + pad
    buf = torch.full((off + r * pitch + 32,), fill, dtype=torch.uint8, device=dev)
    v = buf[off:off + r * pitch].view(r, pitch)[:, :rb]
    v.copy_(torch.from_numpy(np.ascontiguousarray(plane).view(np.uint8).reshape(r, rb)).to(dev))
    return (v.view(torch.uint16 if plane.itemsize == 2 else torch.uint32),), (buf, off, r, rb, pitch)


def _rows(info, dtype):
    """The rows of a frame made by _dev, from its byte buffer, and whether every other byte of the buffer still has `MARK`."""
    buf, off, r, rb, pitch = info
    b = buf.cpu().numpy()
    keep = np.ones(b.shape, bool)
    rows = np.empty((r, rb), np.uint8)
    for y in range(r):
        rows[y] = b[off + y * pitch:off + y * pitch + rb]
        keep[off + y * pitch:off + y * pitch + rb] = False
    return rows.view(dtype), bool((b[keep] == MARK).all())


def _planar_at(bgr, dev, off=0):
    """A contiguous device copy of a host [.., H, W] uint16 array starting `off` bytes into its buffer."""
    raw = np.ascontiguousarray(bgr).view(np.uint8).reshape(-1)
    buf = torch.full((off + raw.size + 32,), MARK, dtype=torch.uint8, device=dev)
    v = buf[off:off + raw.size]
    v.copy_(torch.from_numpy(raw).to(dev))
    return v.view(torch.uint16).view(bgr.shape), buf


def _noise(c, H, W, seed):
    g = np.random.default_rng(seed)
    cw = C.chroma_width(P.SAMPLING[c], W)
    yuv = tuple(g.integers(0, 1024, sh).astype(np.uint16) for sh in ((H, W), (H, cw), (H, cw)))
    bgr = g.integers(0, 1024, (3, H, W)).astype(np.uint16)
    return yuv, bgr


def _check_both_directions(dev, c, mat, rng, yuv, bgr, dirt=None, **place):
    import fldr_pack10 as V
    fmt = _fmt(c, mat, rng)
    H, W = yuv[0].shape
    s = P.SAMPLING[c]
    frame, _ = _dev(P.pack(*yuv, c, dirt=dirt)[0], dev, **place)
    got = V.to_planar([frame], fmt, W=W).cpu().numpy()[0]
    assert np.array_equal(got, C.yuv_to_bgr(*yuv, s, mat, rng, 10)), ("to_planar", c, mat, rng, H, W, place)
    want = P.pack(*C.bgr_to_yuv(bgr, s, mat, rng, 10), c)[0]
    out, info = _dev(np.zeros_like(want), dev, **place)
    V.from_planar(torch.from_numpy(bgr).to(dev), fmt, out=out)
    rows, clean = _rows(info, want.dtype)
    assert np.array_equal(rows, want), ("from_planar", c, mat, rng, H, W, place)
    assert clean, ("from_planar wrote outside the rows", c, H, W, place)


# ---- every code value ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _grid_planes(W, cw):
    """All 1024 values of the first component (one per row, W columns) against a 33 x 33 grid of the other two (0, 32, .. 992, 1023; cw
    columns: the grid point changes along the row, the first few again when cw > 1089)."""
    grid = np.minimum(np.arange(33) * 32, 1023)
    j = np.arange(cw) % 1089
    a = np.repeat(np.arange(1024)[:, None], W, axis=1)
    b = np.broadcast_to(np.repeat(grid, 33)[j][None, :], (1024, cw))
    c = np.broadcast_to(np.tile(grid, 33)[j][None, :], (1024, cw))
    return tuple(np.ascontiguousarray(p.astype(np.uint16)) for p in (a, b, c))


@pytest.mark.parametrize("c", P.CONTAINERS)
@pytest.mark.parametrize("mat,rng", FORMATS)
def test_every_luma_value_against_a_chroma_grid(dev, mat, rng, c):
    """As YUV: every luma value against the chroma grid (4:2:2: 2184 luma columns = 364 v210 groups, so that the 1092 chroma columns hold
    the whole grid; 4:4:4: 1096 columns).  As BGR: every value of B against the grid of G, R (1096 columns: v210's last group is partial).
    All take the wide form."""
    W = 1096 if P.SAMPLING[c] == "444" else 2184
    yuv = _grid_planes(W, C.chroma_width(P.SAMPLING[c], W))
    bgr = np.stack(_grid_planes(1096, 1096))
    _check_both_directions(dev, c, mat, rng, yuv, bgr, dirt=np.random.default_rng(1))


# ---- noise and edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", P.CONTAINERS)
@pytest.mark.parametrize("mat,rng", FORMATS)
def test_noise_and_vertical_edges(dev, c, mat, rng):
    """Seeded noise at a width of whole v210 groups (the wide form), at a multiple of 8 that is not (the wide form with a guarded last
    group) and at an odd one (the per-sample form); then hard vertical edges at an even and an odd column, low | high and high | low, in the
    YUV planes and in the BGR planes: the horizontal taps (1, 1 on odd columns; 1, 2, 1 around even ones) straddle them, and at columns
    5 / 6 / 7 and 23 / 24 / 25 they straddle the boundary between two v210 groups, i.e. two lanes."""
    full = P.SAMPLING[c] == "444"
    for H, W in ((6, 240), (4, 208), (5, 77)):
        yuv, bgr = _noise(c, H, W, seed=H * W)
        _check_both_directions(dev, c, mat, rng, yuv, bgr, dirt=np.random.default_rng(2))
        for edge in (W // 2 - W // 2 % 2, W // 2 - W // 2 % 2 + 1, 1, 5, 6, 7, 23, 24, 25, W - 1):
            for lo, hi in ((0, 1023), (1023, 0), (255, 767)):
                x = np.arange(W)
                step = np.where(x < edge, lo, hi).astype(np.uint16)
                plane = np.repeat(step[None, :], H, axis=0)
                cstep = plane if full else np.ascontiguousarray(plane[:, 0::2])          # chroma sample i sits on luma column 2 i
                _check_both_directions(dev, c, mat, rng, (plane, cstep, np.ascontiguousarray(cstep[:, ::-1])),
                                       np.stack([plane, np.ascontiguousarray(plane[:, ::-1]), plane]))


@pytest.mark.parametrize("c", P.CONTAINERS)
def test_three_frames_in_one_call_equal_three_calls(dev, c):
    import fldr_pack10 as V
    fmt = _fmt(c)
    frames = [_dev(P.pack(*_noise(c, 4, 48, seed=k)[0], c)[0], dev)[0] for k in range(3)]
    got = V.to_planar(frames, fmt, W=48).cpu().numpy()
    for k in range(3):
        assert np.array_equal(got[k], V.to_planar([frames[k]], fmt, W=48).cpu().numpy()[0]), k
    assert not np.array_equal(got[0], got[2])


# ---- sizes, pitches, alignment ------------------------------------------------------------------------------------------------------
def _sweep_widths(c):
    import fldr_pack10 as V
    run = V.RUN[c]
    block = 64 * run                                                           # luma columns one block covers
    return [1, 2, 5, 6, 7, 11, 12, 13, 23, 24, 25, 47, 48, 49, 64, block - run, block, block + run]


@pytest.mark.parametrize("c", P.CONTAINERS)
def test_size_sweep_with_tight_padded_and_offset_planes(dev, c):
    """H in {1, 2, 4, 5}; W around the group, the run, twice the run, and one run short of, at and one run past a block's 64 runs.  Each
    size: tight rows; rows padded by 12 bytes (the per-sample form) and by 128 (the wide form stays where W allows it); v210 at its
    customary pitch; the plane started 4 and 8 bytes into its buffer (the per-sample form), and the planar BGR frame started 8 bytes into
    its own (the per-sample form of Y210 / Y410; v210 asks 4-byte alignment of it only).  Every variant gives the oracle's bytes, hence the aligned run's, and the output kernel leaves every byte outside the
    rows as it was."""
    import fldr_pack10 as V
    s = P.SAMPLING[c]
    mat, rng = FORMATS[P.CONTAINERS.index(c) + 1]
    fmt = _fmt(c, mat, rng)
    for W in _sweep_widths(c):
        for H in (1, 2, 4, 5):
            yuv, bgr = _noise(c, H, W, seed=1000 * H + W)
            plane = P.pack(*yuv, c, dirt=np.random.default_rng(W))[0]
            want_bgr = C.yuv_to_bgr(*yuv, s, mat, rng, 10)
            want = P.pack(*C.bgr_to_yuv(bgr, s, mat, rng, 10), c)[0]
            variants = [(dict(), 0), (dict(pad=12), 0), (dict(pad=128), 0), (dict(pad=16, off=4), 0), (dict(pad=16, off=8), 0), (dict(pad=16), 8)]
            if c == "v210":
                variants += [(dict(pitch=P.v210_pitch(W)), 0), (dict(), 2)]   # a planar frame at 2 mod 4: v210's per-sample form
            for place, poff in variants:
                tag = (H, W, place, poff)
                frame, _ = _dev(plane, dev, **place)
                dst, dbuf = _planar_at(np.zeros((1, 3, H, W), np.uint16), dev, off=poff)
                V.to_planar([frame], fmt, planar=dst, W=W)
                assert np.array_equal(dst.cpu().numpy()[0], want_bgr), ("to_planar",) + tag
                db = dbuf.cpu().numpy()
                assert (db[:poff] == MARK).all() and (db[poff + want_bgr.nbytes:] == MARK).all(), ("to_planar wrote outside",) + tag
                src, _ = _planar_at(bgr, dev, off=poff)
                out, info = _dev(np.zeros_like(want), dev, **place)
                V.from_planar(src, fmt, out=out)
                rows, clean = _rows(info, want.dtype)
                assert np.array_equal(rows, want), ("from_planar",) + tag
                assert clean, ("from_planar wrote outside the rows",) + tag


@pytest.mark.parametrize("c", P.CONTAINERS)
@pytest.mark.parametrize("W", [4096, 1998])
def test_wide_rows(dev, c, W):
    """4096 = 682 v210 groups and 4 pixels: wide accesses everywhere but on the planar side of each row's last group.  1998 = 333 whole
    groups and no multiple of 8: v210 wide throughout, Y210 / Y410 per sample.  Tight rows and, for v210, the customary pitch."""
    yuv, bgr = _noise(c, 3, W, seed=W)
    places = [dict()] + ([dict(pitch=P.v210_pitch(W))] if c == "v210" else [])
    for place in places:
        _check_both_directions(dev, c, "bt709", "limited", yuv, bgr, dirt=np.random.default_rng(W), **place)


# ---- bits that carry no value --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", P.CONTAINERS)
def test_dirt_is_ignored_and_spare_slots_pad_bits_and_alpha_are_written_by_the_rule(dev, c):
    """Every W % 6 (and both parities) in the wide form's widths and in others: a frame with random bits wherever the container carries no
    value converts like the clean one; a written frame has exactly the oracle's clean bytes — zero pad bits, spare luma slots = luma W - 1,
    spare chroma slots = the row's last chroma sample, alpha 3 — in a buffer that held other bytes before."""
    import fldr_pack10 as V
    fmt = _fmt(c)
    s = P.SAMPLING[c]
    for H, W in [(2, w) for w in range(24, 37)] + [(3, 64), (2, 200), (1, 1), (1, 3)]:
        yuv, bgr = _noise(c, H, W, seed=7 + W)
        clean_host, dirty_host = P.pack(*yuv, c)[0], P.pack(*yuv, c, dirt=np.random.default_rng(8))[0]
        assert not np.array_equal(clean_host, dirty_host)
        a = V.to_planar([_dev(clean_host, dev)[0]], fmt, W=W).cpu().numpy()
        b = V.to_planar([_dev(dirty_host, dev)[0]], fmt, W=W).cpu().numpy()
        assert np.array_equal(a, b) and np.array_equal(a[0], C.yuv_to_bgr(*yuv, s, "bt709", "limited", 10)), (H, W)
        Y, U, Vp = C.bgr_to_yuv(bgr, s, "bt709", "limited", 10)
        for fill in (0x00, 0xFF):
            out, info = _dev(np.zeros_like(clean_host), dev, fill=fill)
            out[0].view(torch.uint8).fill_(fill)
            V.from_planar(torch.from_numpy(bgr).to(dev), fmt, out=out)
            got = out[0].cpu().numpy()
            assert np.array_equal(got, P.pack(Y, U, Vp, c)[0]), (H, W, fill)
            if c == "v210":
                ng = (W + 5) // 6
                Ye, Ue, Ve = P.unpack((got,), c, 6 * ng)                       # the spare slots read as samples
                cw = (W + 1) // 2
                assert not (got >> 30).any()
                assert (Ye[:, W:] == Y[:, W - 1:W]).all() and (Ue[:, cw:] == U[:, cw - 1:cw]).all() and (Ve[:, cw:] == Vp[:, cw - 1:cw]).all()
            elif c == "y210":
                assert not (got & 0x3f).any()
                if W % 2:
                    assert np.array_equal(got[:, -2] >> 6, Y[:, -1])
            else:
                assert ((got >> 30) == 3).all()


# ---- the defining property ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", P.CONTAINERS)
@pytest.mark.parametrize("mat,rng", FORMATS)
def test_converters_give_the_bytes_of_the_planar_library_on_the_same_samples(dev, c, mat, rng):
    """A frame in one of these containers gives the planar BGR that fldr_chroma.to_planar gives on the same samples as yuv422p10le /
    yuv444p10le, and from_planar gives fldr_chroma.from_planar's samples, repacked."""
    import fldr_chroma as K
    import fldr_pack10 as V
    s = P.SAMPLING[c]
    kfmt = K.Format(s, "planar", mat, rng, 10)
    for H, W in ((4, 240), (3, 208), (5, 77)):
        yuv, bgr = _noise(c, H, W, seed=3 * W)
        planar = tuple(torch.from_numpy(p).to(dev) for p in C.pack(*yuv, s, "planar", 10))
        want = K.to_planar([planar], kfmt).cpu().numpy()
        got = V.to_planar([_dev(P.pack(*yuv, c)[0], dev)[0]], _fmt(c, mat, rng), W=W).cpu().numpy()
        assert np.array_equal(got, want), (H, W)
        src = torch.from_numpy(bgr).to(dev)
        samples = [p.cpu().numpy() for p in K.from_planar(src, kfmt)]
        out = V.from_planar(src, _fmt(c, mat, rng))
        assert np.array_equal(out[0].cpu().numpy(), P.pack(*samples, c)[0]), (H, W)
