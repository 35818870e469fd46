"""The two converters of libfldr_rgb.so alone (fldr_rgb.to_planar / from_planar) on the GPU, bit for bit against the layouts of
tests/rgb_oracle.py: every layout and depth on seeded noise that holds the extreme codes, a size sweep either side of a lane's run, a
wave's width and the condition of the wide form, with tight, padded and offset planes, rows wider than a block, dirt in the ignored bits,
what from_planar writes as alpha, that no byte outside a frame's rows is written, and the alpha pass alone (fldr_rgb.alpha) against the
oracle's two rules at ordinary times, at the ends, outside them and at NaN."""
import numpy as np
import pytest
import torch

import rgb_oracle as R

pytestmark = pytest.mark.gpu

MARK = 0x5A
HEIGHTS = (1, 2, 5)
WIDTHS = list(range(1, 18)) + [31, 32, 33, 63, 64, 65, 70]
IDS = ["%s-%d" % f for f in R.FORMATS]


def _fmt(layout, depth, alpha="opaque"):
    import fldr_rgb as V
    return V.Format(layout, depth, alpha)


def _torch_dtype(a):
    return {1: torch.uint8, 2: torch.uint16, 4: torch.uint32}[a.itemsize]


def _dev(frame, dev, pad=0, off=0, fill=MARK):
    """A device copy of a host frame, every plane a view into a byte buffer of its own whose other bytes are `fill`: rows `pad` bytes
    wider than the row, starting `off` bytes into the buffer.  -> (frame, [(buffer, off, rows, row bytes, pitch)])."""
    planes, infos = [], []
    for plane in frame:
        r, c = plane.shape
        rb = c * plane.itemsize
        pitch = rb + pad
        buf = torch.full((off + r * pitch + 32,), fill, dtype=torch.uint8, device=dev)
        v = buf[off:off + r * pitch].view(r, pitch)[:, :rb]
        v.copy_(torch.from_numpy(np.ascontiguousarray(plane).view(np.uint8).reshape(r, rb)).to(dev))
        planes.append(v.view(_torch_dtype(plane)))
        infos.append((buf, off, r, rb, pitch))
    return tuple(planes), infos


def _rows(infos, like):
    """The frame made by _dev as host planes, from its byte buffers, and whether every other byte of the buffers still has MARK."""
    out, clean = [], True
    for (buf, off, r, rb, pitch), plane in zip(infos, like):
        b = buf.cpu().numpy()
        keep = np.ones(b.shape, bool)
        rows = np.empty((r, rb), np.uint8)
        for y in range(r):
            rows[y] = b[off + y * pitch:off + y * pitch + rb]
            keep[off + y * pitch:off + y * pitch + rb] = False
        clean = clean and bool((b[keep] == MARK).all())
        out.append(rows.view(plane.dtype))
    return tuple(out), clean


def _planar_at(bgr, dev, off=0):
    """A contiguous device copy of a host [.., H, W] array starting `off` bytes into its buffer (the other bytes MARK)."""
    raw = np.ascontiguousarray(bgr).view(np.uint8).reshape(-1)
    buf = torch.full((off + raw.size + 32,), MARK, dtype=torch.uint8, device=dev)
    v = buf[off:off + raw.size]
    v.copy_(torch.from_numpy(raw).to(dev))
    return (v.view(torch.uint16) if bgr.itemsize == 2 else v).view(bgr.shape), buf


def _noise(layout, depth, H, W, seed):
    """(b, g, r, a): seeded noise over the whole code range with the extreme codes at the first and last pixel; a is None for gbrp."""
    g = np.random.default_rng(seed)
    top = (1 << depth) - 1
    b, gr, r = (g.integers(0, top + 1, (H, W)).astype(R.sample_dtype(depth)) for _ in range(3))
    b.flat[0], gr.flat[0], r.flat[0] = top, 0, top
    b.flat[-1], gr.flat[-1], r.flat[-1] = (0, top, 0) if H * W > 1 else (top, 0, top)
    bits = R.alpha_bits(layout, depth)
    a = g.integers(0, 1 << bits, (H, W)) if bits else None
    return b, gr, r, a


def _check_both_directions(dev, layout, depth, H, W, seed, poff=0, **place):
    import fldr_rgb as V
    fmt = _fmt(layout, depth)
    b, g, r, a = _noise(layout, depth, H, W, seed)
    bgr = np.stack([b, g, r])
    tag = (layout, depth, H, W, place, poff)
    # frame -> planar: noise alpha and dirt go nowhere; nothing outside the planar frame is written
    frame, _ = _dev(R.pack(layout, depth, b, g, r, a, dirt=np.random.default_rng(seed + 1)), dev, **place)
    dst, dbuf = _planar_at(np.zeros((1, 3, H, W), R.sample_dtype(depth)), dev, off=poff)
    V.to_planar([frame], fmt, planar=dst)
    assert np.array_equal(dst.cpu().numpy()[0], bgr), ("to_planar",) + tag
    db = dbuf.cpu().numpy()
    assert (db[:poff] == MARK).all() and (db[poff + bgr.nbytes:] == MARK).all(), ("to_planar wrote outside",) + tag
    # planar -> frame: the oracle's frame with opaque alpha; every byte outside the rows keeps what it held
    want = R.pack(layout, depth, b, g, r)
    src, _ = _planar_at(bgr, dev, off=poff)
    out, infos = _dev(tuple(np.zeros_like(p) for p in want), dev, **place)
    V.from_planar(src, fmt, out=out)
    rows, clean = _rows(infos, want)
    for p, (got, exp) in enumerate(zip(rows, want)):
        assert np.array_equal(got, exp), ("from_planar", p) + tag
    assert clean, ("from_planar wrote outside the rows",) + tag
    return rows


@pytest.mark.parametrize("layout,depth", R.FORMATS, ids=IDS)
def test_every_size_with_aligned_planes(dev, layout, depth):
    """Planes and pitches that are multiples of 16 bytes wherever the width allows it (fresh allocations with tight rows; rows padded by
    32 bytes): the wide form where W permits, the per-sample form elsewhere."""
    for H in HEIGHTS:
        for W in WIDTHS:
            _check_both_directions(dev, layout, depth, H, W, seed=100 * H + W)
            _check_both_directions(dev, layout, depth, H, W, seed=100 * H + W, pad=32)


PLACES = {"tight": (0, dict()), "pad12": (0, dict(pad=12)), "offset4": (0, dict(pad=16, off=4)), "planar_offset": (1, dict(pad=16))}


@pytest.mark.parametrize("place", list(PLACES))
@pytest.mark.parametrize("layout,depth", R.FORMATS, ids=IDS)
def test_every_size_with_planes_that_force_the_per_sample_form(dev, layout, depth, place):
    """A tight pitch (no multiple of 16 at most widths), a pitch with 12 spare bytes, a plane that starts 4 bytes into its buffer, and a
    planar BGR frame that starts one sample into its own: each gives the oracle's bytes, hence the aligned run's."""
    samples, kw = PLACES[place]
    for H in HEIGHTS:
        for W in WIDTHS:
            _check_both_directions(dev, layout, depth, H, W, seed=7 * H + W, poff=samples * (2 if depth == 10 else 1), **kw)


@pytest.mark.parametrize("layout,depth", R.FORMATS, ids=IDS)
def test_rows_wider_than_a_block_and_several_blocks_of_rows(dev, layout, depth):
    """2048 and 1100 columns: more than one block along the row in every kernel (a block covers 256 pixels of a word layout, 1024 / 512
    samples of a plane), in the wide and in the per-sample form; 9 and 6 rows: more than one block of rows."""
    _check_both_directions(dev, layout, depth, 6, 2048, seed=1)
    _check_both_directions(dev, layout, depth, 9, 1100, seed=2, pad=16)
    _check_both_directions(dev, layout, depth, 9, 1099, seed=3, pad=12)


@pytest.mark.parametrize("layout,depth", R.FORMATS, ids=IDS)
def test_from_planar_writes_opaque_alpha_whatever_the_policy_and_masks_depth_10(dev, layout, depth):
    import fldr_rgb as V
    H, W = 3, 20
    b, g, r, _ = _noise(layout, depth, H, W, seed=11)
    bgr = np.stack([b, g, r])
    want = R.pack(layout, depth, b, g, r)
    for policy in ("opaque", "nearer", "blend"):
        for fill in (0x00, 0xFF):
            out, _ = _dev(tuple(np.zeros_like(p) for p in want), dev, fill=fill)
            for p in out:
                p.view(torch.uint8).fill_(fill)
            V.from_planar(torch.from_numpy(bgr).to(dev), _fmt(layout, depth, policy), out=out)
            got = tuple(p.cpu().numpy() for p in out)
            assert all(np.array_equal(x, y) for x, y in zip(got, want)), (layout, depth, policy, fill)
            alpha = R.unpack(layout, depth, got)[3]
            if R.alpha_bits(layout, depth):
                assert (alpha == {8: 255, 10: 1023, 2: 3}[R.alpha_bits(layout, depth)]).all()
            else:
                assert alpha is None and len(got) == 3
    if depth == 10:                                                            # bits above the code value never reach a frame
        dirty = bgr | (np.random.default_rng(5).integers(0, 64, bgr.shape).astype(np.uint16) << 10)
        out = V.from_planar(torch.from_numpy(dirty).to(dev), _fmt(layout, depth))
        assert all(np.array_equal(p.cpu().numpy(), y) for p, y in zip(out, want)), (layout, depth)


@pytest.mark.parametrize("layout,depth", [("bgra", 8), ("x2bgr10", 10), ("gbrap", 10)])
def test_three_frames_in_one_call_equal_three_calls(dev, layout, depth):
    import fldr_rgb as V
    fmt = _fmt(layout, depth)
    host = [R.pack(layout, depth, *_noise(layout, depth, 4, 48, seed=k)) for k in range(3)]
    frames = [_dev(f, dev)[0] for f in host]
    got = V.to_planar(frames, fmt).cpu().numpy()
    for k in range(3):
        assert np.array_equal(got[k], V.to_planar([frames[k]], fmt).cpu().numpy()[0]), k
        assert np.array_equal(got[k], R.planar_bgr(layout, depth, host[k])), k
    assert not np.array_equal(got[0], got[2])


def test_an_hwc_tensor_is_a_byte_frame(dev):
    """[H, W, 4] bytes as image libraries hold them are taken as they are."""
    import fldr_rgb as V
    b, g, r, a = _noise("rgba", 8, 6, 20, seed=9)
    hwc = torch.from_numpy(R.pack("rgba", 8, b, g, r, a)[0].reshape(6, 20, 4)).to(dev)
    assert np.array_equal(V.to_planar([(hwc,)], _fmt("rgba", 8)).cpu().numpy()[0], np.stack([b, g, r]))


# ---- the alpha pass alone -----------------------------------------------------------------------------------------------------------
ALPHA_PAIRS = [(("bgra", 8), ("bgra", 8)), (("argb", 8), ("rgba", 8)), (("abgr", 8), ("gbrap", 8)), (("gbrap", 8), ("argb", 8)),
               (("gbrap", 8), ("gbrap", 8)), (("gbrap", 10), ("gbrap", 10)), (("x2rgb10", 10), ("x2bgr10", 10))]
# ordinary times; the ends; just below one half; outside [0, 1]; NaN and infinity (BLEND: w = 0 and w = 65536)
TIMES = [0.25, 0.5, 0.75, 0.0, 1.0, float(np.nextafter(np.float32(0.5), np.float32(0))), 1.0 / 3.0, -0.25, 7.0, float("nan"), float("inf")]


def _check_alpha(dev, fin, fout, policy, H, W, times, seed, **place):
    import fldr_rgb as V
    ins = [_noise(*fin, H, W, seed + i) for i in range(2)]
    frames = [_dev(R.pack(*fin, *c), dev, **place)[0] for c in ins]
    b, g, r, _ = _noise(*fout, H, W, seed + 2)
    opaque = R.pack(*fout, b, g, r)                                            # what from_planar leaves
    outs, infos = zip(*[_dev(opaque, dev, **place) for _ in times])
    t = torch.tensor(times, dtype=torch.float32, device=dev)
    V.alpha(frames, _fmt(*fin), list(outs), _fmt(*fout, policy), t)
    for k, tv in enumerate(times):
        rows, clean = _rows(infos[k], opaque)
        want = R.pack(*fout, b, g, r, R.alpha_of(policy, ins[0][3], ins[1][3], tv))
        assert all(np.array_equal(x, y) for x, y in zip(rows, want)), (fin, fout, policy, H, W, place, k, tv)
        assert clean, ("the alpha pass wrote outside the rows", fin, fout, H, W, place)


@pytest.mark.parametrize("policy", ["nearer", "blend"])
@pytest.mark.parametrize("fin,fout", ALPHA_PAIRS, ids=["%s%d-%s%d" % (a + b) for a, b in ALPHA_PAIRS])
def test_alpha_pass_alone_at_every_kind_of_time(dev, fin, fout, policy):
    """Only alpha changes, by the oracle's rule, in the wide form (W % 4 == 0, aligned planes) and in the per-pixel form (odd widths, a
    pitch with 12 spare bytes, planes 4 bytes into their buffers), with rows longer than one pass of a block (1030 > 1024)."""
    for H, W in ((1, 1), (2, 3), (5, 16), (3, 17), (2, 64), (5, 70), (3, 1028), (2, 1030)):
        _check_alpha(dev, fin, fout, policy, H, W, TIMES, seed=H * W)
    _check_alpha(dev, fin, fout, policy, 5, 64, TIMES[:3], seed=1, pad=32)
    _check_alpha(dev, fin, fout, policy, 5, 64, TIMES[:3], seed=2, pad=12)
    _check_alpha(dev, fin, fout, policy, 5, 64, TIMES[:3], seed=3, pad=16, off=4)


def test_alpha_pass_takes_more_outputs_than_one_launch_serves(dev):
    """70 outputs: one launch for 64, one for 6."""
    times = [float(k) / 69.0 for k in range(70)]
    _check_alpha(dev, ("bgra", 8), ("gbrap", 8), "blend", 3, 20, times, seed=5)
    _check_alpha(dev, ("rgba", 8), ("rgba", 8), "nearer", 3, 21, times, seed=6)


def test_alpha_pass_leaves_opaque_frames_alone(dev):
    import fldr_rgb as V
    fin, fout = ("bgra", 8), ("argb", 8)
    frames = [_dev(R.pack(*fin, *_noise(*fin, 4, 12, i)), dev)[0] for i in range(2)]
    b, g, r, _ = _noise(*fout, 4, 12, 2)
    host = R.pack(*fout, b, g, r)
    out, infos = _dev(host, dev)
    V.alpha(frames, _fmt(*fin), [out], _fmt(*fout, "opaque"), torch.tensor([0.5], device=dev))
    rows, clean = _rows(infos, host)
    assert np.array_equal(rows[0], host[0]) and clean
