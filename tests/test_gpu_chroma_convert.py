"""The two converters of libfldr_chroma.so alone (fldr_chroma.to_planar / from_planar) on the GPU, bit for bit against
tests/yuv_chroma_oracle.py: every 8-bit code triple, a 10-bit grid, 4:2:2 noise and edges in all six 4:2:2 containers, a size sweep around
the per-thread run and the block width with tight, padded and misaligned planes, dirt in the unused container bits, and the odd-width rule
of the packed layouts."""
import functools

import numpy as np
import pytest
import torch

import yuv_chroma_oracle as C

pytestmark = pytest.mark.gpu

FORMATS = [(m, r) for m in C.MATRICES for r in C.RANGES]
C422 = [c for c in C.containers() if c[0] == "422"]
MARK = 0x5A


def _fmt(s, l, d, mat="bt709", rng="limited"):
    import fldr_chroma as V
    return V.Format(s, l, mat, rng, d)


def _dev(planes, dev, pad=0, offsets=None, fill=MARK):
    """Device copies of host planes.  pad / offsets (bytes, one offset per plane): each plane a view into a byte buffer `pad` bytes wider
    per row whose other bytes are `fill`, starting offsets[p] bytes into it.  -> (plane views, the buffers)."""
    views, bufs = [], []
    for i, p in enumerate(planes):
        r, c = p.shape
        rb = c * p.itemsize
        pitch, off = rb + pad, (offsets[i] if offsets else 0)
        buf = torch.full((off + r * pitch + 32,), fill, dtype=torch.uint8, device=dev)
        v = buf[off:off + r * pitch].view(r, pitch)[:, :rb]
        v.copy_(torch.from_numpy(np.ascontiguousarray(p).view(np.uint8).reshape(r, rb)).to(dev))
        views.append(v.view(torch.uint16) if p.itemsize == 2 else v)
        bufs.append((buf, off, r, rb, pitch))
    return tuple(views), bufs


def _gaps_untouched(bufs, fill=MARK):
    for buf, off, r, rb, pitch in bufs:
        b = buf.cpu().numpy()
        keep = np.ones(b.shape, bool)
        for y in range(r):
            keep[off + y * pitch:off + y * pitch + rb] = False
        if not (b[keep] == fill).all():
            return False
    return True


def _planar_at(bgr, dev, off=0):
    """A contiguous device copy of a host [.., H, W] array starting `off` bytes into its buffer."""
    raw = np.ascontiguousarray(bgr).view(np.uint8).reshape(-1)
    buf = torch.full((off + raw.size + 32,), MARK, dtype=torch.uint8, device=dev)
    v = buf[off:off + raw.size]
    v.copy_(torch.from_numpy(raw).to(dev))
    return (v.view(torch.uint16) if bgr.itemsize == 2 else v).view(bgr.shape), buf


def _host(frame):
    return tuple(p.cpu().numpy() for p in frame)


def _noise(s, d, H, W, seed):
    g = np.random.default_rng(seed)
    mx, cw = (1 << d) - 1, C.chroma_width(s, W)
    yuv = tuple(g.integers(0, mx + 1, sh).astype(C.dtype_of(d)) for sh in ((H, W), (H, cw), (H, cw)))
    bgr = g.integers(0, mx + 1, (3, H, W)).astype(C.dtype_of(d))
    return yuv, bgr


def _check_both_directions(dev, s, l, d, mat, rng, yuv, bgr, dirt=None):
    import fldr_chroma as V
    fmt = _fmt(s, l, d, mat, rng)
    H, W = yuv[0].shape
    frame, _ = _dev(C.pack(*yuv, s, l, d, dirt=dirt), dev)
    got = V.to_planar([frame], fmt, W=W).cpu().numpy()[0]
    assert np.array_equal(got, C.yuv_to_bgr(*yuv, s, mat, rng, d)), ("to_planar", s, l, d, mat, rng, H, W)
    out = _host(V.from_planar(torch.from_numpy(bgr).to(dev), fmt))
    want = C.pack(*C.bgr_to_yuv(bgr, s, mat, rng, d), s, l, d)
    for p, (a, b) in enumerate(zip(out, want)):
        assert np.array_equal(a, b), ("from_planar", s, l, d, mat, rng, H, W, p)


# ---- every code value ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _all_triples():
    """Every 8-bit triple as three [4096, 4096] planes: plane 0 the slow index."""
    idx = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    return tuple(np.ascontiguousarray(((idx >> sh) & 255).astype(np.uint8)) for sh in (16, 8, 0))


@pytest.mark.parametrize("mat,rng", FORMATS)
def test_every_8_bit_yuv_triple_to_bgr(dev, mat, rng):
    import fldr_chroma as V
    Y, U, Vp = _all_triples()
    frame = tuple(torch.from_numpy(p).to(dev) for p in (Y, U, Vp))
    got = V.to_planar([frame], _fmt("444", "planar", 8, mat, rng)).cpu().numpy()[0]
    R, G, B = C.yuv444_to_rgb(Y, U, Vp, mat, rng)
    for c, w in enumerate((B, G, R)):
        assert np.array_equal(got[c], w), c


@pytest.mark.parametrize("mat,rng", FORMATS)
def test_every_8_bit_bgr_triple_to_yuv(dev, mat, rng):
    import fldr_chroma as V
    B, G, R = _all_triples()
    out = _host(V.from_planar(torch.from_numpy(np.stack([B, G, R])).to(dev), _fmt("444", "planar", 8, mat, rng)))
    for p, w in enumerate(C.rgb_to_yuv444(R, G, B, mat, rng)):
        assert np.array_equal(out[p], w), p


@pytest.mark.parametrize("layout", ["planar", "semiplanar"])
@pytest.mark.parametrize("mat,rng", FORMATS)
def test_10_bit_every_luma_value_against_a_chroma_grid(dev, mat, rng, layout):
    """All 1024 values of the first component against a 33 x 33 grid of the other two (0, 32, .. 992, 1023), as YUV and as BGR, in both
    10-bit 4:4:4 containers.  The frame is 1024 x 1096 (the 1089 grid points and the first 7 again: a multiple of the run, the wide form)."""
    grid = np.minimum(np.arange(33) * 32, 1023)
    j = np.arange(1096) % 1089
    a = np.repeat(np.arange(1024)[:, None], 1096, axis=1)
    b = np.broadcast_to(np.repeat(grid, 33)[j][None, :], a.shape)
    c = np.broadcast_to(np.tile(grid, 33)[j][None, :], a.shape)
    planes = tuple(np.ascontiguousarray(p.astype(np.uint16)) for p in (a, b, c))
    _check_both_directions(dev, "444", layout, 10, mat, rng, planes, np.stack(planes), dirt=np.random.default_rng(1))


# ---- 4:2:2: noise and edges in every container ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,l,d", C422)
@pytest.mark.parametrize("mat,rng", FORMATS)
def test_422_noise_and_vertical_edges(dev, s, l, d, mat, rng):
    """Seeded noise at a width that is a multiple of the run (the wide form) and at an odd one (the per-sample form); then hard vertical
    edges at an even and an odd column, low | high and high | low, in the YUV planes and in the BGR planes: the horizontal taps (1, 1 on
    odd columns; 1, 2, 1 around even ones) straddle them."""
    mx = (1 << d) - 1
    for H, W in ((6, 208), (5, 77)):
        yuv, bgr = _noise(s, d, H, W, seed=H * W + d)
        _check_both_directions(dev, s, l, d, mat, rng, yuv, bgr, dirt=np.random.default_rng(2))
        for edge in (W // 2 - W // 2 % 2, W // 2 - W // 2 % 2 + 1, 1, W - 1):
            for lo, hi in ((0, mx), (mx, 0), (mx // 4, 3 * mx // 4)):
                x = np.arange(W)
                step = np.where(x < edge, lo, hi).astype(C.dtype_of(d))
                full = np.repeat(step[None, :], H, axis=0)
                cstep = np.ascontiguousarray(full[:, 0::2])                    # chroma sample i sits on luma column 2 i
                _check_both_directions(dev, s, l, d, mat, rng, (full, cstep, np.ascontiguousarray(cstep[:, ::-1])),
                                       np.stack([full, np.ascontiguousarray(full[:, ::-1]), full]))


def test_three_frames_in_one_call_equal_three_calls(dev):
    import fldr_chroma as V
    fmt = _fmt("422", "semiplanar", 10)
    frames = [_dev(C.pack(*_noise("422", 10, 4, 24, seed=k)[0], "422", "semiplanar", 10), dev)[0] for k in range(3)]
    got = V.to_planar(frames, fmt).cpu().numpy()
    for k in range(3):
        assert np.array_equal(got[k], V.to_planar([frames[k]], fmt).cpu().numpy()[0]), k
    assert not np.array_equal(got[0], got[2])


# ---- sizes, pitches, alignment ------------------------------------------------------------------------------------------------------
def _sweep_widths(d):
    import fldr_chroma as V
    run = V.RUN[d]
    block = 64 * run                                                           # luma columns one block covers
    return sorted(set(list(range(1, 10)) + [run - 1, run, run + 1, 2 * run - 1, 2 * run, 2 * run + 1, block - 1, block, block + 1, block + run]))


@pytest.mark.parametrize("s,l,d", C.containers())
def test_size_sweep_with_tight_padded_and_misaligned_planes(dev, s, l, d):
    """H in {1, 2, 3, 5}, W from 1 to 9 and around the per-thread run, twice the run and the block width.  Each size: tight pitches; pitches
    padded by 16 bytes (the wide form stays where W allows it) and by an odd / 2 mod 4 amount; then each plane in turn, and the planar BGR
    frame, started at an odd (depth 8) or 2 mod 4 (depth 10) byte offset, which forces the per-sample form.  Every variant gives the
    oracle's bytes, hence the aligned run's, and the output kernel leaves every byte outside the rows as it was."""
    import fldr_chroma as V
    mat, rng = FORMATS[(len(s + l) + d) % 4]
    fmt = _fmt(s, l, d, mat, rng)
    odd = 1 if d == 8 else 2
    for W in _sweep_widths(d):
        for H in (1, 2, 3, 5):
            yuv, bgr = _noise(s, d, H, W, seed=1000 * H + W)
            planes = C.pack(*yuv, s, l, d, dirt=np.random.default_rng(W))
            want_bgr = C.yuv_to_bgr(*yuv, s, mat, rng, d)
            want = C.pack(*C.bgr_to_yuv(bgr, s, mat, rng, d), s, l, d)
            n = len(planes)
            variants = [(0, None, 0), (16, None, 0), (16 + odd, None, 0), (16, [0] * n, odd)]
            variants += [(16, [odd if q == p else 0 for q in range(n)], 0) for p in range(n)]
            for pad, offs, poff in variants:
                tag = (H, W, pad, offs, poff)
                frame, _ = _dev(planes, dev, pad=pad, offsets=offs)
                dst, dbuf = _planar_at(np.zeros((1, 3, H, W), C.dtype_of(d)), dev, off=poff)
                V.to_planar([frame], fmt, planar=dst, W=W)
                assert np.array_equal(dst.cpu().numpy()[0], want_bgr), ("to_planar",) + tag
                db = dbuf.cpu().numpy()
                assert (db[:poff] == MARK).all() and (db[poff + want_bgr.nbytes:] == MARK).all(), ("to_planar wrote outside",) + tag
                src, _ = _planar_at(bgr, dev, off=poff)
                out, bufs = _dev([np.zeros_like(p) for p in want], dev, pad=pad, offsets=offs)
                V.from_planar(src, fmt, out=out)
                for p, (a, b) in enumerate(zip(_host(out), want)):
                    assert np.array_equal(a, b), ("from_planar", p) + tag
                assert _gaps_untouched(bufs), ("from_planar wrote outside the rows",) + tag


# ---- bits that carry no value --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,l,d", [c for c in C.containers() if c[2] == 10])
def test_dirt_in_the_spare_bits_is_ignored_and_never_written(dev, s, l, d):
    import fldr_chroma as V
    fmt = _fmt(s, l, d)
    for H, W in ((4, 64), (3, 21)):
        yuv, bgr = _noise(s, d, H, W, seed=7)
        clean, _ = _dev(C.pack(*yuv, s, l, d), dev)
        dirty_host = C.pack(*yuv, s, l, d, dirt=np.random.default_rng(8))
        assert any(not np.array_equal(a, b) for a, b in zip(dirty_host, C.pack(*yuv, s, l, d)))
        dirty, _ = _dev(dirty_host, dev)
        a, b = V.to_planar([clean], fmt).cpu().numpy(), V.to_planar([dirty], fmt).cpu().numpy()
        assert np.array_equal(a, b) and np.array_equal(a[0], C.yuv_to_bgr(*yuv, s, "bt709", "limited", d))
        spare = 0x003f if l == "semiplanar" else 0xfc00
        for p in _host(V.from_planar(torch.from_numpy(bgr).to(dev), fmt)):
            assert not (p & spare).any() and p.any()


@pytest.mark.parametrize("l", ["uyvy", "yuyv"])
def test_odd_width_packed_frames_ignore_and_copy_the_spare_luma_byte(dev, l):
    import fldr_chroma as V
    fmt = _fmt("422", l, 8)
    spare = -1 if l == "uyvy" else -2                                          # the second luma byte of a row's last group
    for H, W in ((3, 33), (2, 1), (4, 1025)):
        yuv, bgr = _noise("422", 8, H, W, seed=W)
        host = C.pack(*yuv, "422", l, 8)[0]
        outs = []
        for v in (0, 255):
            h = host.copy()
            h[:, spare] = v
            outs.append(V.to_planar([_dev((h,), dev)[0]], fmt, W=W).cpu().numpy()[0])
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], C.yuv_to_bgr(*yuv, "422", "bt709", "limited", 8))
        out = np.full((H, 4 * ((W + 1) // 2)), MARK, np.uint8)
        frame = (torch.from_numpy(out).to(dev),)
        V.from_planar(torch.from_numpy(bgr).to(dev), fmt, out=frame)
        got = frame[0].cpu().numpy()
        Y = C.bgr_to_yuv(bgr, "422", "bt709", "limited", 8)[0]
        assert np.array_equal(got[:, spare], Y[:, -1]) and np.array_equal(C.unpack((got,), "422", l, W)[0], Y)
