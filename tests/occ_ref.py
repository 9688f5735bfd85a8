"""float32 numpy restatement of the warp rasteriser and of its optional outputs (DESIGN.md "Backward flow and
occlusion"): warped RGB / mask, backward flow B, backward occlusion OccBwd and forward occlusion Occ.

`warp_ref` is vectorised (every (triangle, cell) pair the rasteriser visits at once); `warp_brute` is a plain
sequential Python statement of the definitions, for tiny grids only.  Both evaluate every float expression in the
rasteriser's order, one IEEE float32 operation at a time, so they agree with the GPU bit for bit.
"""
import numpy as np

F = np.float32


def field_from_flow(flow):
    """warp position of the ArapFlow_Warp path: (float)x + flow.x, (float)y + flow.y"""
    H, W = flow.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W]
    return np.stack([xs.astype(F) + flow[..., 0].astype(F), ys.astype(F) + flow[..., 1].astype(F)], -1)


def _bary(p0x, p0y, p1x, p1y, p2x, p2y, sx, sy):
    """the rasteriser's inside test and barycentrics (b0, b1, b2) at (sx, sy); arrays of float32"""
    with np.errstate(all="ignore"):
        one = F(1.0)
        X0, X1, X2 = p0x - sx * one, p1x - sx * one, p2x - sx * one
        Y0, Y1, Y2 = p0y - sy * one, p1y - sy * one, p2y - sy * one
        d01 = X0 * Y1 - Y0 * X1
        d12 = X1 * Y2 - Y1 * X2
        d20 = X2 * Y0 - Y2 * X0
        skip = (d01 < 0) & (d12 < 0) & (d20 < 0)
        ood = one / ((d01 + d12) + d20)
        d01, d12, d20 = d01 * ood, d12 * ood, d20 * ood
        ok = ~skip & (d01 >= 0) & (d12 >= 0) & (d20 >= 0)
    return ok, d12, d20, d01


def _triangles(field, mask):
    """every rasterised triangle in index order: index, corner grid coordinates (int) and warp positions"""
    H, W = mask.shape
    obj = mask == 0
    q = np.zeros((H, W), bool)
    if W > 1 and H > 1:
        q[:-1, :-1] = obj[:-1, :-1] & obj[:-1, 1:] & obj[1:, :-1] & obj[1:, 1:]
    u = np.flatnonzero(q.ravel())
    ux, uy = u % W, u // W
    t = np.stack([2 * u, 2 * u + 1], 1).ravel()
    # 2u = (p00, p01, p10), 2u+1 = (p10, p01, p11)
    ax = np.stack([ux, ux], 1).ravel(); ay = np.stack([uy, uy + 1], 1).ravel()
    bx = np.stack([ux + 1, ux + 1], 1).ravel(); by = np.stack([uy, uy], 1).ravel()
    cx = np.stack([ux, ux + 1], 1).ravel(); cy = np.stack([uy + 1, uy + 1], 1).ravel()
    P = field.reshape(-1, 2)
    pa, pb, pc = P[ax + W * ay], P[bx + W * by], P[cx + W * cy]
    return t, (ax, ay, bx, by, cx, cy), (pa, pb, pc)


def _cell_ranges(W, H, pa, pb, pc):
    """raster_tri's loop: x = xa .. while x < W and x <= maxx (y likewise); empty for a NaN corner"""
    with np.errstate(invalid="ignore"):
        mnx = np.floor(np.minimum(pa[:, 0], np.minimum(pb[:, 0], pc[:, 0])))
        mny = np.floor(np.minimum(pa[:, 1], np.minimum(pb[:, 1], pc[:, 1])))
        mxx = np.ceil(np.maximum(pa[:, 0], np.maximum(pb[:, 0], pc[:, 0])))
        mxy = np.ceil(np.maximum(pa[:, 1], np.maximum(pb[:, 1], pc[:, 1])))
    nan = np.isnan(mnx) | np.isnan(mny) | np.isnan(mxx) | np.isnan(mxy)
    mnx, mny, mxx, mxy = [np.where(nan, 0, a) for a in (mnx, mny, mxx, mxy)]
    xa = np.clip(mnx, 0, W).astype(np.int64)
    ya = np.clip(mny, 0, H).astype(np.int64)
    xb = np.clip(mxx, -1, W - 1).astype(np.int64)
    yb = np.clip(mxy, -1, H - 1).astype(np.int64)
    nx = np.where(nan, 0, np.maximum(xb - xa + 1, 0))
    ny = np.where(nan, 0, np.maximum(yb - ya + 1, 0))
    return xa, ya, nx, ny


def _pairs(xa, ya, nx, ny):
    """flat list of (triangle row, cell x, cell y) of every cell every triangle visits"""
    n = nx * ny
    k = np.repeat(np.arange(len(n)), n)
    off = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
    return k, xa[k] + off // np.maximum(ny[k], 1), ya[k] + off % np.maximum(ny[k], 1)


def own_max_tri(mask):
    """m(v): the largest index of a rasterised triangle with v as a corner, -1 if none"""
    H, W = mask.shape
    obj = mask == 0
    q = np.zeros((H + 1, W + 1), bool)          # q[y+1, x+1] = quad (x, y) rasterised
    if W > 1 and H > 1:
        q[1:H, 1:W] = obj[:-1, :-1] & obj[:-1, 1:] & obj[1:, :-1] & obj[1:, 1:]
    ys, xs = np.mgrid[0:H, 0:W]
    u = xs + W * ys
    m = np.full((H, W), -1, np.int64)
    for on, val in ((q[:H, :W], 2 * (u - W - 1) + 1), (q[:H, 1:], 2 * (u - W) + 1), (q[1:, :W], 2 * (u - 1) + 1),
                    (q[1:, 1:], 2 * u)):          # increasing order: the last one set wins
        m = np.where(on, val, m)
    return m


def warp_ref(rgb, mask, field):
    """-> dict(warped_rgb, warped_mask, backward_flow, occlusion_bwd, occlusion); rgb may be None"""
    H, W = mask.shape
    N = W * H
    field = np.ascontiguousarray(field, F)
    t, (ax, ay, bx, by, cx, cy), (pa, pb, pc) = _triangles(field, mask)
    xa, ya, nx, ny = _cell_ranges(W, H, pa, pb, pc)
    k, x, y = _pairs(xa, ya, nx, ny)
    ok, b0, b1, b2 = _bary(pa[k, 0], pa[k, 1], pb[k, 0], pb[k, 1], pc[k, 0], pc[k, 1], x.astype(F), y.astype(F))
    k, x, y, b0, b1, b2 = k[ok], x[ok], y[ok], b0[ok], b1[ok], b2[ok]
    key = (t[k].astype(np.uint64) + np.uint64(1)) << np.uint64(32)
    if rgb is not None:
        img = rgb.reshape(-1, 3)
        v = np.zeros(len(k), np.uint64)
        for c in range(3):
            c0, c1, c2 = (img[a + W * b, c].astype(F) for a, b in ((ax[k], ay[k]), (bx[k], by[k]), (cx[k], cy[k])))
            s = (c0 * b0 + c1 * b1) + c2 * b2
            v = (v << np.uint64(8)) | (s.astype(np.uint64) & np.uint64(0xff))
        key |= v
    keys = np.zeros(N, np.uint64)
    np.maximum.at(keys, x + W * y, key)
    covered = keys != 0
    out = dict(warped_mask=np.where(covered, 255, 0).astype(np.uint8).reshape(H, W))
    out["warped_rgb"] = None if rgb is None else np.stack(
        [(keys >> np.uint64(s)) & np.uint64(0xff) for s in (16, 8, 0)], -1).astype(np.uint8).reshape(H, W, 3)
    # backward flow: T(q)'s barycentrics at q, the source point from the corners' grid coordinates
    q = np.flatnonzero(covered)
    tq = ((keys[q] >> np.uint64(32)) - np.uint64(1)).astype(np.int64)
    r = np.searchsorted(t, tq)
    qx, qy = (q % W).astype(F), (q // W).astype(F)
    ok, b0, b1, b2 = _bary(pa[r, 0], pa[r, 1], pb[r, 0], pb[r, 1], pc[r, 0], pc[r, 1], qx, qy)
    assert ok.all()
    B = np.zeros((N, 2), F)
    for d, (A, Bc, Cc) in enumerate(((ax, bx, cx), (ay, by, cy))):
        s = (A[r].astype(F) * b0 + Bc[r].astype(F) * b1) + Cc[r].astype(F) * b2
        B[q, d] = s - (qx if d == 0 else qy)
    out["backward_flow"] = B.reshape(H, W, 2)
    obj = (mask == 0).ravel()
    out["occlusion_bwd"] = np.where(~covered & obj, 255, 0).astype(np.uint8).reshape(H, W)
    # forward occlusion: object vertices binned by the cell of P(v), tested by the triangles visiting that cell
    P = field.reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        inside = (P[:, 0] >= 0) & (P[:, 0] <= F(W - 1)) & (P[:, 1] >= 0) & (P[:, 1] <= F(H - 1))
    occ = np.where(obj, np.where(inside, 0, 255), np.where(covered, 255, 0)).astype(np.uint8)
    vs = np.flatnonzero(obj & inside)
    cell = np.floor(P[vs, 0]).astype(np.int64) + W * np.floor(P[vs, 1]).astype(np.int64)
    order = np.argsort(cell, kind="stable")
    vs, cell = vs[order], cell[order]
    start = np.searchsorted(cell, np.arange(N + 1))
    m = own_max_tri(mask).ravel()
    k, x, y = _pairs(xa, ya, nx, ny)
    c = x + W * y
    cnt = start[c + 1] - start[c]
    kk = np.repeat(k, cnt)
    off = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    v = vs[np.repeat(start[c], cnt) + off]
    later = t[kk] > m[v]
    kk, v = kk[later], v[later]
    ok = _bary(pa[kk, 0], pa[kk, 1], pb[kk, 0], pb[kk, 1], pc[kk, 0], pc[kk, 1], P[v, 0], P[v, 1])[0]
    occ[v[ok]] = 255
    out["occlusion"] = occ.reshape(H, W)
    return out


def warp_brute(rgb, mask, field):
    """the definitions, sequentially: the reference's quad loop with later writes winning, then every pixel and vertex
    on its own.  Tiny grids only."""
    H, W = mask.shape
    field = np.ascontiguousarray(field, F)
    one = F(1.0)

    def bary(p0, p1, p2, sx, sy):
        with np.errstate(all="ignore"):
            X0, X1, X2 = p0[0] - sx * one, p1[0] - sx * one, p2[0] - sx * one
            Y0, Y1, Y2 = p0[1] - sy * one, p1[1] - sy * one, p2[1] - sy * one
            d01, d12, d20 = X0 * Y1 - Y0 * X1, X1 * Y2 - Y1 * X2, X2 * Y0 - Y2 * X0
            if d01 < 0 and d12 < 0 and d20 < 0:
                return None
            ood = one / ((d01 + d12) + d20)
            d01, d12, d20 = d01 * ood, d12 * ood, d20 * ood
        if not (d01 >= 0 and d12 >= 0 and d20 >= 0):
            return None
        return d12, d20, d01

    def visits(p0, p1, p2, x, y):
        """does raster_tri's loop visit cell (x, y) for this triangle"""
        xs, ys = [p[0] for p in (p0, p1, p2)], [p[1] for p in (p0, p1, p2)]
        if any(np.isnan(a) for a in xs + ys):
            return False
        mnx, mny = np.floor(min(xs)), np.floor(min(ys))      # clamped as floats first: +-Inf has no int
        xa = 0 if mnx < 0 else W if mnx > W else int(mnx)
        ya = 0 if mny < 0 else H if mny > H else int(mny)
        return xa <= x < W and x <= np.ceil(max(xs)) and ya <= y < H and y <= np.ceil(max(ys))

    tris = []                                     # (index, [corner (gx, gy)]) in index order
    for uy in range(H - 1):
        for ux in range(W - 1):
            if all(mask[y, x] == 0 for x, y in ((ux, uy), (ux + 1, uy), (ux, uy + 1), (ux + 1, uy + 1))):
                u = ux + W * uy
                tris.append((2 * u, [(ux, uy), (ux + 1, uy), (ux, uy + 1)]))
                tris.append((2 * u + 1, [(ux, uy + 1), (ux + 1, uy), (ux + 1, uy + 1)]))
    win = np.full((H, W), -1, np.int64)
    wrgb = np.zeros((H, W, 3), np.uint8)
    for ti, cs in tris:
        p = [field[gy, gx] for gx, gy in cs]
        for y in range(H):
            for x in range(W):
                if not visits(*p, x, y):
                    continue
                b = bary(*p, F(x), F(y))
                if b is None:
                    continue
                win[y, x] = ti                    # later triangles overwrite
                if rgb is not None:
                    for ch in range(3):
                        c = [F(rgb[gy, gx, ch]) for gx, gy in cs]
                        wrgb[y, x, ch] = int((c[0] * b[0] + c[1] * b[1]) + c[2] * b[2]) & 0xff
    byidx = dict(tris)
    B = np.zeros((H, W, 2), F)
    obwd = np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            if win[y, x] < 0:
                obwd[y, x] = 255 if mask[y, x] == 0 else 0
                continue
            cs = byidx[int(win[y, x])]
            b = bary(*[field[gy, gx] for gx, gy in cs], F(x), F(y))
            for d in range(2):
                s = (F(cs[0][d]) * b[0] + F(cs[1][d]) * b[1]) + F(cs[2][d]) * b[2]
                B[y, x, d] = s - F((x, y)[d])
    occ = np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            if mask[y, x] != 0:
                occ[y, x] = 255 if win[y, x] >= 0 else 0
                continue
            P = field[y, x]
            if not (P[0] >= 0 and P[0] <= F(W - 1) and P[1] >= 0 and P[1] <= F(H - 1)):
                occ[y, x] = 255
                continue
            own = [ti for ti, cs in tris if (x, y) in cs]
            m = max(own) if own else -1
            cx, cy = int(np.floor(P[0])), int(np.floor(P[1]))
            for ti, cs in tris:
                if (x, y) in cs or ti <= m:
                    continue
                p = [field[gy, gx] for gx, gy in cs]
                if visits(*p, cx, cy) and bary(*p, P[0], P[1]) is not None:
                    occ[y, x] = 255
                    break
    return dict(warped_rgb=None if rgb is None else wrgb, warped_mask=np.where(win >= 0, 255, 0).astype(np.uint8),
                backward_flow=B, occlusion_bwd=obwd, occlusion=occ)


def folded_case(W, H, amp, seed=None):
    """test_gpu_warp.py's random folded flows: rgb, 10 % background, normal flow of amplitude `amp`"""
    rng = np.random.default_rng(W * H if seed is None else seed)
    rgb = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    mask = np.where(rng.random((H, W)) < 0.1, 255, 0).astype(np.uint8)
    fl = (rng.normal(size=(H, W, 2)) * amp).astype(np.float32)
    fl[mask != 0] = 0
    return rgb, mask, fl
