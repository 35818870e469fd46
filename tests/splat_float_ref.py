"""The forward splat (FunctionSoftsplat: summation, average, linear, softmax) in float64, written from its definition and not from the
kernels or the oracle: plain numpy, no shared code with oracle/fldr_oracle.py and no call into it.  It is what the fp32 oracle
(tests/test_splat_ref_cpu.py) and fldr_softsplat_acc64 (tests/test_gpu_splat_ops.py) are held to.  Next to it: the error bound of a
kernel that forms the operator's fp32 products and sums them exactly, the exact flow bounds per source block in the layout the
kernels read, a model of the kernel's candidate search on those bounds, and the statement with one fault at a time (the mutants).

  The operation.  Source pixel (x, y) of sample n moves to o = (x + fx, y + fy).  That sum is formed in fp32: the rounding belongs to
  the operator's definition (the position, not the flow, decides which cells a source touches).  Everything after it is float64.
  With x0 = floor(ox), ax = ox - x0 (and the same in y) the source adds  value * weight  to the four cells (x0, y0), (x0 + 1, y0),
  (x0, y0 + 1), (x0 + 1, y0 + 1) with weights (1 - ax)(1 - ay), ax (1 - ay), (1 - ax) ay, ax ay; corners outside the frame add nothing.
  The modes differ in what is added: summation v = img; average v = img and 1 into a normaliser; linear v = img m and m; softmax
  v = ((img + 1) / 2) exp(m) and exp(m) (m = 0 without a metric).  Output: (A / S - 1/2) 2, A the cell's sum, S its normaliser with
  S == 0 -> 1 (summation: S = 1): a cell that nothing reaches is exactly -1, a hole.

  Holes.  The hole set of this statement equals the fp32 operator's whenever no fp32 product underflows: x1 - ox with x1 = x0 + 1 is
  exact in fp32 (both lie within one unit of each other, Sterbenz), so are ox - x0 and the y factors; a weight is the product of two
  such factors and is zero in fp32 exactly when one factor is zero, which is exactly when it is zero in float64; and a positive
  metric weight times a positive corner weight is positive unless it underflows.  The CPU test asserts that no nonzero product of
  any case lies below 2^-100.

  The bound (per element; u = 2^-24, the unit roundoff of fp32).  A kernel that forms the operator's fp32 products commits, per
  contribution to the numerator, relative errors of at most
      d_pre  u            the sum img + 1 of softmax (the halving is exact), 0 otherwise;
      d_g    2 u E        exp(m) of softmax, E = the allowed distance in ulps (an ulp is at most 2 u of the value), 0 otherwise;
      d_v    u            the product pre * g, where one is formed (linear, softmax with a metric);
      d_w    u            the corner weight, one product of two exact factors;
      d_t    u            the product value * weight;
  r_num = their sum, and per contribution to the normaliser r_den = d_g + d_w + (u where g is not the constant 1).  With
  Aabs = sum |terms| >= |A| and every normaliser term positive:
      eA = (r_num + n 2^-53) Aabs, then + u (|A| + eA) for the cast of the fp64 sum to fp32   (n contributions: their fp64 additions),
      eS = (r_den + n 2^-53) S,    then + u (S + eS),
      Q  = A / S:  |A_f / S_f - Q| <= (eA + |Q| eS) / (S - eS) =: eQ0,   the quotient within one ulp (st_div): eQ = eQ0 + 2 u (|Q| + eQ0),
      output (q - 1/2) 2: one rounding of the difference, an exact doubling:  bound = 2 (eQ + u (|Q - 1/2| + eQ)).
  Summation has no quotient: bound = 2 (eA + u (|A - 1/2| + eA)).  Second-order terms are covered by a factor 1 + 2^-20 on r_num and
  r_den.  A hole is exact: bound 0.  E is not fixed here: the CPU test measures it (exp_ulp_distance) and passes it in."""
import numpy as np

U32 = 2.0 ** -24
MODES = ("summation", "average", "linear", "softmax")
BW, BH, SBX, SBY = 64, 4, 4, 16                  # source block, blocks per super-block
SB_BLOCKS = SBX * SBY
Q_BLOCKS, Q_SUPER, WHOLE_PIXELS = 512, 64, 2304
FAULTS = ("east_tile", "column_w", "trunc", "tiny", "norm_floor", "queue_512", "nw_left")
WALKS = ("whole", "none", "rect", "queue", "rect_overflow", "whole_sb_overflow")


def positions(flow):
    """fp32 flow [N,2,H,W] -> (ox, oy) float64 [N,H,W]: the fp32 sums index + flow, widened."""
    f = np.asarray(flow, np.float32)
    N, _, H, W = f.shape
    ox = np.arange(W, dtype=np.float32)[None, None, :] + f[:, 0]
    oy = np.arange(H, dtype=np.float32)[None, :, None] + f[:, 1]
    assert ox.dtype == np.float32 and oy.dtype == np.float32
    return ox.astype(np.float64), oy.astype(np.float64)


def corners(flow, fault=None):
    """The four corners of every source: [(flat cell index [N,HW] (0 where outside), weight [N,HW], inside [N,HW], tx, ty)]."""
    f = np.asarray(flow)
    N, _, H, W = f.shape
    ox, oy = positions(f)
    rnd = np.trunc if fault == "trunc" else np.floor
    x0, y0 = rnd(ox), rnd(oy)
    ax, ay = ox - x0, oy - y0
    out = []
    for dy, wy in ((0, 1.0 - ay), (1, ay)):
        for dx, wx in ((0, 1.0 - ax), (1, ax)):
            tx, ty = x0 + dx, y0 + dy
            wt = wx * wy
            if fault == "column_w":                                  # column W counts as inside: the flat index runs into the next row
                inside = (tx >= 0) & (tx <= W) & (ty >= 0) & (ty < H) & (ty * W + tx < H * W)
            else:
                inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
            if fault == "east_tile" and dx == 1:
                inside &= (np.mod(tx, 64) != 0) | (tx == 0)             # (column 0 belongs to no next tile)
            if fault == "tiny":
                inside &= wt >= 1e-6
            idx = np.where(inside, ty * W + tx, 0).astype(np.int64)
            out.append((idx.reshape(N, -1), wt.reshape(N, -1), inside.reshape(N, -1), np.where(inside, tx, -9).reshape(N, -1),
                        np.where(inside, ty, -9).reshape(N, -1), dx))
    return out


def _pre_and_g(img, metric, mode):
    img = np.asarray(img, np.float64)
    N, C, H, W = img.shape
    m = None if metric is None else np.asarray(metric, np.float64).reshape(N, 1, H * W)
    pre = img.reshape(N, C, H * W)
    g = np.ones((N, 1, H * W))
    if mode == "linear":
        g = m
    elif mode == "softmax":
        pre = (pre + 1.0) / 2.0
        if m is not None:
            g = np.exp(m)
    return pre, g


def _dropped_by_queue(flow, geom):
    """Fault queue_512: per sample, [(source mask [HW], tx0, tx1, ty0, ty1)] of the tile columns with more than 512 matching blocks."""
    N, _, H, W = np.asarray(flow).shape
    TW, TH, K = geom
    blk, sbt = block_bounds(flow)
    model = search_model(blk, sbt, H, W, TW, TH, K, want_blocks=True)
    out = []
    for n in range(N):
        cols = []
        for col in model[n]:
            if col["n_match"] <= Q_BLOCKS or col["sb_over"]:
                continue
            mask = np.zeros((H, W), bool)
            for bx, by in col["blocks"][Q_BLOCKS:]:
                mask[by * BH:(by + 1) * BH, bx * BW:(bx + 1) * BW] = True
            cols.append((mask.reshape(-1), col["tx0"], col["tx0"] + TW - 1, col["sy0"], col["sy0"] + K * TH - 1))
        out.append(cols)
    return out


def splat(img, flow, metric, mode, fault=None, geom=None):
    """img [N,C,H,W], flow [N,2,H,W] fp32, metric [N,1,H,W] or None -> (out [N,C,H,W], norm [N,1,H,W]) float64; norm is the
    normaliser before 0 -> 1 (the sum of the corner weights times the metric weights; for summation, the same with weight 1: its
    zeros are the cells nothing reaches).  fault / geom: one of FAULTS and (TW, TH, K) of the configuration, for the mutants."""
    assert mode in MODES and (fault is None or fault in FAULTS)
    N, C, H, W = np.asarray(img).shape
    pre, g = _pre_and_g(img, metric, mode)
    queue = _dropped_by_queue(flow, geom) if fault == "queue_512" else None
    A = np.zeros((N, C, H * W))
    S = np.zeros((N, 1, H * W))
    for idx, wt, inside, tx, ty, dx in corners(flow, fault):
        if fault == "nw_left" and dx == 1:                           # the source's north-west corner is the last column of the tile to the left
            inside = inside & (np.mod(tx, geom[0]) != 0)
        for n in range(N):
            keep = inside[n]
            if queue is not None:
                keep = keep.copy()
                for mask, cx0, cx1, cy0, cy1 in queue[n]:
                    keep &= ~(mask & (tx[n] >= cx0) & (tx[n] <= cx1) & (ty[n] >= cy0) & (ty[n] <= cy1))
            w = np.where(keep, wt[n], 0.0)
            S[n, 0] += np.bincount(idx[n], weights=g[n, 0] * w, minlength=H * W)
            for c in range(C):
                A[n, c] += np.bincount(idx[n], weights=(pre[n, c] * g[n, 0]) * w, minlength=H * W)
    if mode == "summation":
        out = A
    elif fault == "norm_floor":
        out = A / np.maximum(S, 1e-7)
    else:
        out = A / np.where(S == 0.0, 1.0, S)
    return ((out - 0.5) * 2.0).reshape(N, C, H, W), S.reshape(N, 1, H, W)


def reach(flow):
    """[N,1,H,W]: +1 where a cell is reached by a nonzero weight, -1 where not: the `average` splat of an all-ones image."""
    N, _, H, W = np.asarray(flow).shape
    out, _ = splat(np.ones((N, 1, H, W)), flow, None, "average")
    return out


def max_weight(flow):
    """[N,H,W]: the largest corner weight that reaches each cell (0 where none does)."""
    N, _, H, W = np.asarray(flow).shape
    best = np.zeros((N, H * W))
    for idx, wt, inside, _, _, _ in corners(flow):
        for n in range(N):
            np.maximum.at(best[n], idx[n][inside[n]], wt[n][inside[n]])
    return best.reshape(N, H, W)


def smallest_product(img, flow, metric, mode):
    """The smallest nonzero magnitude among the products the operator forms: pre * g, g * weight, (pre * g) * weight (in-frame corners)."""
    N, C = np.asarray(img).shape[:2]
    pre, g = _pre_and_g(img, metric, mode)
    vals = [np.abs(pre * g)]
    for idx, wt, inside, _, _, _ in corners(flow):
        w = np.where(inside, wt, 0.0)[:, None]
        vals += [np.abs(g * w), np.abs(pre * g) * w]
    lo = np.inf
    for v in vals:
        nz = v[v > 0]
        if nz.size:
            lo = min(lo, float(nz.min()))
    return lo


def exp_ulp_distance(m32, e32):
    """The largest distance, in fp32 ulps of the true value, between an fp32 implementation's exp (e32 = exp(m32) as it computed it)
    and float64 exp of the same fp32 arguments."""
    ref = np.exp(np.asarray(m32, np.float32).astype(np.float64))
    ulp = np.exp2(np.floor(np.log2(ref)) - 23)
    return float((np.abs(np.asarray(e32, np.float32).astype(np.float64) - ref) / ulp).max())


def bound(img, flow, metric, mode, exp_ulps):
    """The per-element error bound [N,C,H,W] derived in the module docstring, for exp within `exp_ulps` ulps."""
    N, C, H, W = np.asarray(img).shape
    pre, g = _pre_and_g(img, metric, mode)
    has_metric = mode == "linear" or (mode == "softmax" and metric is not None)
    d_pre = U32 if mode == "softmax" else 0.0
    d_g = 2 * U32 * exp_ulps if (mode == "softmax" and metric is not None) else 0.0
    d_v = U32 if has_metric else 0.0
    second = 1.0 + 2.0 ** -20
    r_num = (d_pre + d_g + d_v + U32 + U32) * second
    r_den = (d_g + U32 + (U32 if has_metric else 0.0)) * second
    A = np.zeros((N, C, H * W))
    Aabs = np.zeros((N, C, H * W))
    S = np.zeros((N, 1, H * W))
    cnt = np.zeros((N, 1, H * W))
    for idx, wt, inside, _, _, _ in corners(flow):
        for n in range(N):
            w = np.where(inside[n], wt[n], 0.0)
            S[n, 0] += np.bincount(idx[n], weights=g[n, 0] * w, minlength=H * W)
            cnt[n, 0] += np.bincount(idx[n], weights=(w > 0).astype(np.float64), minlength=H * W)
            for c in range(C):
                t = (pre[n, c] * g[n, 0]) * w
                A[n, c] += np.bincount(idx[n], weights=t, minlength=H * W)
                Aabs[n, c] += np.bincount(idx[n], weights=np.abs(t), minlength=H * W)
    s64 = cnt * 2.0 ** -53
    eA = (r_num + s64) * Aabs
    eA = eA + U32 * (np.abs(A) + eA)
    if mode == "summation":
        b = 2.0 * (eA + U32 * (np.abs(A - 0.5) + eA))
        return b.reshape(N, C, H, W)
    eS = (r_den + s64) * S
    eS = eS + U32 * (S + eS)
    hole = S == 0.0
    Ss = np.where(hole, 1.0, S)
    Q = A / Ss
    eQ = (eA + np.abs(Q) * eS) / (Ss - eS)
    eQ = eQ + 2 * U32 * (np.abs(Q) + eQ)
    b = 2.0 * (eQ + U32 * (np.abs(Q - 0.5) + eQ))
    return np.where(hole, 0.0, b).reshape(N, C, H, W)


def violations(got, ref, norm, bnd):
    """The comparison of the GPU test, as a list of findings (empty: the result passes): every element finite and within the bound
    of the statement, and exactly -1.0 where the statement's normaliser is 0."""
    got = np.asarray(got, np.float64)
    found = []
    if got.shape != ref.shape:
        return ["shape %s, expected %s" % (got.shape, ref.shape)]
    if not np.isfinite(got).all():
        found.append("%d non-finite values" % int((~np.isfinite(got)).sum()))
    hole = np.broadcast_to(norm == 0.0, ref.shape)
    wrong = hole & (got != -1.0)
    if wrong.any():
        found.append("%d hole elements are not exactly -1.0" % int(wrong.sum()))
    with np.errstate(invalid="ignore"):
        over = ~(np.abs(got - ref) <= bnd)
    if over.any():
        k = np.unravel_index(np.argmax(np.where(over, np.abs(got - ref) - bnd, -np.inf)), ref.shape)
        found.append("%d elements beyond the bound, worst at %s: got %.9g, statement %.9g, bound %.3g" % (int(over.sum()), k, got[k], ref[k], bnd[k]))
    return found


def share_of_bound(got, ref, bnd):
    """max |got - ref| / bound over the elements with a positive bound (0 if there are none)."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    pos = bnd > 0
    return float((err[pos] / bnd[pos]).max()) if pos.any() else 0.0


# ---- exact flow bounds in the layout the kernels read ------------------------------------------------------------------------------
def table_geometry(H, W):
    """(nsb_x, nsb_y) super-blocks of an H x W map."""
    return -(-W // (SBX * BW)), -(-H // (SBY * BH))


def block_bounds(flow):
    """fp32 flow [N,2,H,W] -> (blk [N,nsb,64,4], sbt [N,nsb,4]) fp32: the exact (xmin, xmax, ymin, ymax) of the flow per 64 x 4
    block and per 256 x 64 super-block; block b of a super-block sits at column b % 4, row b // 4; blocks and super-blocks outside the
    map are (+inf, -inf, +inf, -inf)."""
    f = np.asarray(flow, np.float32)
    N, _, H, W = f.shape
    nsb_x, nsb_y = table_geometry(H, W)
    Hp, Wp = nsb_y * SBY * BH, nsb_x * SBX * BW
    lo = np.full((N, 2, Hp, Wp), np.inf, np.float32)
    hi = np.full((N, 2, Hp, Wp), -np.inf, np.float32)
    lo[:, :, :H, :W] = f
    hi[:, :, :H, :W] = f
    # [N,2,sby,block row,BH,sbx,block column,BW] -> reduce the pixels of a block
    shape = (N, 2, nsb_y, SBY, BH, nsb_x, SBX, BW)
    bmin = lo.reshape(shape).min(axis=(4, 7))                          # [N,2,sby,SBY,sbx,SBX]
    bmax = hi.reshape(shape).max(axis=(4, 7))
    blk = np.stack([bmin[:, 0], bmax[:, 0], bmin[:, 1], bmax[:, 1]], -1)       # [N,sby,SBY,sbx,SBX,4]
    blk = blk.transpose(0, 1, 3, 2, 4, 5).reshape(N, nsb_y * nsb_x, SB_BLOCKS, 4)
    sbt = np.stack([blk[..., 0].min(2), blk[..., 1].max(2), blk[..., 2].min(2), blk[..., 3].max(2)], -1)
    return np.ascontiguousarray(blk, np.float32), np.ascontiguousarray(sbt, np.float32)


def table_workspace(blk, sbt):
    """The flat fp32 workspace fldr_softsplat_acc64 reads a caller-filled table from: all block entries, then all super-block entries."""
    return np.concatenate([blk.reshape(-1), sbt.reshape(-1)]).astype(np.float32)


def split_workspace(ws, tables, H, W):
    """A flat workspace of `tables` tables (samples, or problems x samples for the pair form) -> (blk [tables,nsb,64,4], sbt [tables,nsb,4])."""
    nsb_x, nsb_y = table_geometry(H, W)
    nsb = nsb_x * nsb_y
    ws = np.asarray(ws, np.float32).reshape(-1)
    nb = tables * nsb * SB_BLOCKS * 4
    assert ws.size == nb + tables * nsb * 4, (ws.size, tables, nsb)
    return ws[:nb].reshape(tables, nsb, SB_BLOCKS, 4), ws[nb:].reshape(tables, nsb, 4)


# ---- the kernel's candidate search, restated on a table ----------------------------------------------------------------------------
def _match(b, rx0, rx1, ry0, ry1, tx0, tx1, ty0, ty1):
    """st_match in fp32: can sources of the region [rx0, rx1] x [ry0, ry1] with flow bounds b[..., 4] touch the tile?  Conservative by
    one cell."""
    f = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        return ((f(rx1) + b[..., 1] >= f(tx0) - f(2)) & (f(rx0) + b[..., 0] <= f(tx1) + f(1)) &
                (f(ry1) + b[..., 3] >= f(ty0) - f(2)) & (f(ry0) + b[..., 2] <= f(ty1) + f(1)))


def search_model(blk, sbt, H, W, TW, TH, K, whole=None, want_blocks=False):
    """What fldr_softsplat_acc64's search does with a table, per sample and per column of K tiles (row-major over the columns):
    dict(tx0, sy0, n_sb (matching super-blocks; all of them when there are at most 64), n_match (matching blocks), sb_over,
    walks (one per tile of the column that lies in the map)).  Walks: `whole` (maps of at most 2304 pixels, or whole=True),
    `whole_sb_overflow` (more than 64 matching super-blocks), `none` (no block matches), `rect` (the rectangle the joint bounds
    allow), `queue` (the queued blocks, when the rectangle would visit more pixels), `rect_overflow` (more than 512 matching
    blocks: the rectangle, whatever its size)."""
    f = np.float32
    blk, sbt = np.asarray(blk, np.float32), np.asarray(sbt, np.float32)
    N = blk.shape[0]
    nsb_x, nsb_y = table_geometry(H, W)
    nsb = nsb_x * nsb_y
    if whole is None:
        whole = H * W <= WHOLE_PIXELS
    s = np.arange(nsb)
    sbx0, sby0 = (s % nsb_x) * SBX * BW, (s // nsb_x) * SBY * BH
    b = np.arange(SB_BLOCKS)
    bx = (s[:, None] % nsb_x) * SBX + b[None, :] % SBX                  # [nsb,64] block coordinates
    by = (s[:, None] // nsb_x) * SBY + b[None, :] // SBX
    out = []
    for n in range(N):
        cols = []
        for sty in range(-(-H // (K * TH))):
            for stx in range(-(-W // TW)):
                tx0, sy0 = stx * TW, sty * K * TH
                tx1, sy1 = tx0 + TW - 1, min(sy0 + K * TH, H) - 1
                tiles = [sy0 + k * TH for k in range(K) if sy0 + k * TH < H]
                col = dict(tx0=tx0, sy0=sy0, n_sb=0, n_match=0, sb_over=False, walks=[])
                cols.append(col)
                if whole:
                    col["walks"] = ["whole"] * len(tiles)
                    continue
                if nsb <= Q_SUPER:
                    listed = np.ones(nsb, bool)
                else:
                    listed = _match(sbt[n], sbx0, sbx0 + SBX * BW - 1, sby0, sby0 + SBY * BH - 1, tx0, tx1, sy0, sy1)
                col["n_sb"] = int(listed.sum())
                if col["n_sb"] > Q_SUPER:
                    col["sb_over"] = True
                    col["walks"] = ["whole_sb_overflow"] * len(tiles)
                    continue
                hit = _match(blk[n], bx * BW, bx * BW + BW - 1, by * BH, by * BH + BH - 1, tx0, tx1, sy0, sy1) & listed[:, None]
                col["n_match"] = n_match = int(hit.sum())
                if want_blocks:
                    col["blocks"] = list(zip(bx[hit].tolist(), by[hit].tolist()))       # super-block order, then block order
                if n_match == 0:
                    col["walks"] = ["none"] * len(tiles)
                    continue
                hb = blk[n][hit]
                rxmin, rxmax, rymin, rymax = hb[:, 0].min(), hb[:, 1].max(), hb[:, 2].min(), hb[:, 3].max()
                cx0, cx1 = int(bx[hit].min()) * BW, int(bx[hit].max()) * BW + BW - 1
                cy0, cy1 = int(by[hit].min()) * BH, int(by[hit].max()) * BH + BH - 1
                bounded = all(abs(float(v)) < 1.0e6 for v in (rxmin, rxmax, rymin, rymax))
                for ty0 in tiles:
                    X0, X1, Y0, Y1 = cx0, min(cx1, W - 1), cy0, min(cy1, H - 1)
                    if bounded:
                        X0 = max(X0, int(np.floor(f(tx0) - f(2) - rxmax)))
                        X1 = min(X1, int(np.ceil(f(tx1) + f(1) - rxmin)))
                        Y0 = max(Y0, int(np.floor(f(ty0) - f(2) - rymax)))
                        Y1 = min(Y1, int(np.ceil(f(ty0 + TH - 1) + f(1) - rymin)))
                    area = max(X1 - X0 + 1, 0) * max(Y1 - Y0 + 1, 0)
                    if n_match > Q_BLOCKS:
                        col["walks"].append("rect_overflow")
                    else:
                        col["walks"].append("rect" if area <= 256 * n_match else "queue")
        out.append(cols)
    return out


def walks_of(model):
    """The set of walks a search model takes, over all samples, columns and tiles."""
    return {w for cols in model for col in cols for w in col["walks"]}
