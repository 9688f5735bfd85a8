"""float32 numpy restatement of the point tracks (DESIGN.md "Point tracks"): the position of caller-given sub-pixel
points of frame 1 in every state of a layered sequence, and whether they are hidden there.  On top of occ_ref
(triangles, cell ranges, `_bary`, `own_max_tri`) and layers_step_ref (`_tables`, `_in_frame`, cases).

`track_ref` is vectorised; `track_brute` is a plain sequential Python statement of the definitions, for tiny grids only.
Both take `masks` [n][H][W], `fields` [T][n][H][W][2], the layers' positions in the T states, and `points` [P][2], and
evaluate every float expression in the kernels' order, one IEEE float32 operation at a time.
"""
import numpy as np

import layers_step_ref as sref
import occ_ref
from occ_ref import F

CLASSES = ("visible", "out", "same", "higher", "bg_hit", "bg_free")


def locate(masks, points):
    """the owner of every point: layer (-1: background, -2: outside the frame or NaN), triangle, barycentrics [P,3],
    M, and the three corner indices [P,3]"""
    masks = np.asarray(masks)
    n, H, W = masks.shape
    pts = np.ascontiguousarray(points, F)
    P = len(pts)
    valid = sref._in_frame(pts, W, H)
    layer = np.where(valid, -1, -2).astype(np.int64)
    tri = np.full(P, -1, np.int64)
    bary = np.zeros((P, 3), F)
    M = np.full(P, -1, np.int64)
    corners = np.zeros((P, 3), np.int64)
    v = np.flatnonzero(valid)
    px, py = pts[v, 0], pts[v, 1]
    ix, iy = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
    for l in range(n):                              # increasing (layer, triangle): the last to pass is the largest
        obj = masks[l] == 0
        on = np.zeros((H, W), bool)
        if W > 1 and H > 1:
            on[:-1, :-1] = obj[:-1, :-1] & obj[:-1, 1:] & obj[1:, :-1] & obj[1:, 1:]
        m = occ_ref.own_max_tri(masks[l]).ravel()
        for b, a in ((1, 1), (1, 0), (0, 1), (0, 0)):
            qx, qy = ix - a, iy - b
            inside = (qx >= 0) & (qy >= 0) & (qx + 1 < W) & (qy + 1 < H)
            ok_q = inside & on[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]
            for odd in (0, 1):                      # 2u = (p00, p01, p10), 2u+1 = (p10, p01, p11)
                cx = np.stack([qx, qx + 1, qx + odd], -1)
                cy = np.stack([qy + odd, qy, qy + 1], -1)
                ok, b0, b1, b2 = occ_ref._bary(cx[:, 0].astype(F), cy[:, 0].astype(F), cx[:, 1].astype(F),
                                               cy[:, 1].astype(F), cx[:, 2].astype(F), cy[:, 2].astype(F), px, py)
                hit = np.flatnonzero(ok & ok_q)
                k = v[hit]
                layer[k] = l
                tri[k] = 2 * (qx[hit] + W * qy[hit]) + odd
                bary[k] = np.stack([b0[hit], b1[hit], b2[hit]], -1)
                ci = cx[hit] + W * cy[hit]
                corners[k] = ci
                M[k] = m[ci].max(-1)
    return layer, tri, bary, M, corners


def track_ref(masks, fields, points, parts=False):
    """-> dict(pos f32[T,P,2], occ u8[T,P]).  With `parts` also the flags by cause, bool[T,P]: `out` (an owned point
    leaves the frame), `same` (a hit with l' == l), `higher` (a hit with l' > l, background points included), and
    `owned`, `valid` bool[P]"""
    masks = np.asarray(masks)
    n, H, W = masks.shape
    N = W * H
    fields = np.ascontiguousarray(fields, F)
    T = fields.shape[0]
    pts = np.ascontiguousarray(points, F)
    P = len(pts)
    layer, tri, bary, M, corners = locate(masks, pts)
    owned = layer >= 0
    pos = np.zeros((T, P, 2), F)
    occ = np.zeros((T, P), np.uint8)
    flags = {k: np.zeros((T, P), bool) for k in ("out", "same", "higher")}
    for s in range(T):
        d = pts.copy()
        for l in range(n):
            k = np.flatnonzero(layer == l)
            Pb = fields[s, l].reshape(-1, 2)
            i0, i1, i2 = corners[k, 0], corners[k, 1], corners[k, 2]
            with np.errstate(invalid="ignore", over="ignore"):
                for c in range(2):
                    d[k, c] = (Pb[i0, c] * bary[k, 0] + Pb[i1, c] * bary[k, 1]) + Pb[i2, c] * bary[k, 2]
        pos[s] = d
        inside = sref._in_frame(d, W, H)
        same, higher = np.zeros(P, bool), np.zeros(P, bool)
        wl = np.maximum(layer, -1)                  # a background point asks from below every layer
        vs = np.flatnonzero(inside)
        cell = np.floor(d[vs, 0]).astype(np.int64) + W * np.floor(d[vs, 1]).astype(np.int64)
        order = np.argsort(cell, kind="stable")
        vs, cell = vs[order], cell[order]
        start = np.searchsorted(cell, np.arange(N + 1))
        for lp, (t, _, (pa, pb, pc), (k, x, y)) in enumerate(sref._tables(masks, fields[s])):
            c = x + W * y
            cnt = start[c + 1] - start[c]
            kk = np.repeat(k, cnt)
            off = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
            v = vs[np.repeat(start[c], cnt) + off]
            rule = (lp > wl[v]) | ((lp == wl[v]) & (t[kk] > M[v]))
            kk, v = kk[rule], v[rule]
            ok = occ_ref._bary(pa[kk, 0], pa[kk, 1], pb[kk, 0], pb[kk, 1], pc[kk, 0], pc[kk, 1], d[v, 0], d[v, 1])[0]
            v = v[ok]
            same[v[wl[v] == lp]] = True
            higher[v[wl[v] < lp]] = True
        occ[s] = np.where(~inside | same | higher, 255, 0)
        flags["out"][s], flags["same"][s], flags["higher"][s] = owned & ~inside, same, higher
    out = dict(pos=pos, occ=occ)
    if parts:
        out.update(flags, owned=owned, valid=layer >= -1)
    return out


def class_counts(r, s):
    """the six classes of state s from track_ref(.., parts=True), in the order of CLASSES.  `same` and `higher` are the
    flags of layers_step_ref: a point may carry both, and `higher` counts every hit with l' > l, the background points
    (which ask from below every layer) included; bg_hit / bg_free split the in-frame background points"""
    owned, bg = r["owned"], r["valid"] & ~r["owned"]
    hit = r["out"][s] | r["same"][s] | r["higher"][s]
    return [int((owned & ~hit).sum()), int(r["out"][s].sum()), int(r["same"][s].sum()), int(r["higher"][s].sum()),
            int((bg & r["higher"][s]).sum()), int((bg & ~r["higher"][s]).sum())]


def track_brute(masks, fields, points):
    """the definitions, sequentially: every point on its own against every triangle.  -> dict(pos, occ)"""
    masks = np.asarray(masks)
    n, H, W = masks.shape
    fields = np.ascontiguousarray(fields, F)
    T = fields.shape[0]
    pts = np.ascontiguousarray(points, F)
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

    def visits(p, x, y):
        xs, ys = [c[0] for c in p], [c[1] for c in p]
        if any(np.isnan(v) for v in xs + ys):
            return False
        mnx, mny = np.floor(min(xs)), np.floor(min(ys))      # clamped as floats first: +-Inf has no int
        xa = 0 if mnx < 0 else W if mnx > W else int(mnx)
        ya = 0 if mny < 0 else H if mny > H else int(mny)
        return xa <= x < W and x <= np.ceil(max(xs)) and ya <= y < H and y <= np.ceil(max(ys))

    def in_frame(p):
        return bool(p[0] >= 0 and p[0] <= F(W - 1) and p[1] >= 0 and p[1] <= F(H - 1))

    tris = []                                     # (layer, index, quad, [corner (gx, gy)]) in (layer, index) order
    for l in range(n):
        for uy in range(H - 1):
            for ux in range(W - 1):
                if all(masks[l, y, x] == 0 for x, y in ((ux, uy), (ux + 1, uy), (ux, uy + 1), (ux + 1, uy + 1))):
                    u = ux + W * uy
                    tris.append((l, 2 * u, (ux, uy), [(ux, uy), (ux + 1, uy), (ux, uy + 1)]))
                    tris.append((l, 2 * u + 1, (ux, uy), [(ux, uy + 1), (ux + 1, uy), (ux + 1, uy + 1)]))
    pos = np.zeros((T, len(pts), 2), F)
    occ = np.zeros((T, len(pts)), np.uint8)
    for k, p in enumerate(pts):
        if not in_frame(p):
            pos[:, k], occ[:, k] = p, 255
            continue
        fx, fy = int(np.floor(p[0])), int(np.floor(p[1]))
        own = None
        for l, ti, quad, cs in tris:              # the last to pass is the largest (layer, triangle)
            if quad not in ((fx, fy), (fx - 1, fy), (fx, fy - 1), (fx - 1, fy - 1)):
                continue
            b = bary(*[(F(gx), F(gy)) for gx, gy in cs], p[0], p[1])
            if b is not None:
                own = (l, cs, b)
        for s in range(T):
            if own is None:
                l, m, d = -1, -1, (p[0], p[1])
            else:
                l, cs, b = own
                pb = [fields[s, l, gy, gx] for gx, gy in cs]
                with np.errstate(all="ignore"):
                    d = tuple((pb[0][c] * b[0] + pb[1][c] * b[1]) + pb[2][c] * b[2] for c in range(2))
                m = max(tj for lt, tj, _, cj in tris if lt == l and any(c in cj for c in cs))
            pos[s, k] = d
            if not in_frame(d):
                occ[s, k] = 255
                continue
            cx, cy = int(np.floor(d[0])), int(np.floor(d[1]))
            for lt, tj, _, cj in tris:
                if not (lt > l or (lt == l and tj > m)):
                    continue
                q = [fields[s, lt, gy, gx] for gx, gy in cj]
                if visits(q, cx, cy) and bary(*q, d[0], d[1]) is not None:
                    occ[s, k] = 255
                    break
    return dict(pos=pos, occ=occ)


def pixel_points(W, H):
    """the N integer pixels in index order"""
    ys, xs = np.mgrid[0:H, 0:W]
    return np.stack([xs.ravel(), ys.ravel()], -1).astype(F)


def case_points(W, H, seed):
    """the point set of a GPU case: the N integer pixels; 300 seeded sub-pixel points, a quarter of them on the quarter
    lattice; points with px = W - 1 and with py = H - 1; three points outside the frame and a NaN point; one point
    repeated five times.  P > N"""
    rng = np.random.default_rng(seed + 9000)
    sub = np.stack([rng.uniform(0, W - 1, 300), rng.uniform(0, H - 1, 300)], -1).astype(F)
    sub[:75] = np.minimum(np.round(sub[:75] * 4) / 4, [W - 1, H - 1]).astype(F)
    right = np.stack([np.full(6, W - 1), rng.uniform(0, H - 1, 6)], -1).astype(F)
    bottom = np.stack([rng.uniform(0, W - 1, 6), np.full(6, H - 1)], -1).astype(F)
    corner = np.array([[W - 1, H - 1], [0, 0]], F)
    outside = np.array([[-0.25, 1.0], [W - 0.5, 0.5], [1.0, H + 3.0], [np.nan, 0.5]], F)
    rep = np.repeat(sub[100:101], 5, 0)
    return np.concatenate([pixel_points(W, H), sub, right, bottom, corner, outside, rep]).astype(F)


def rectangle_points():
    """quarter-lattice points of sref.rectangles_case's 16 x 12 frame"""
    ys, xs = np.mgrid[0:4 * 11 + 1, 0:4 * 15 + 1]
    return np.stack([xs.ravel() / 4.0, ys.ravel() / 4.0], -1).astype(F)
