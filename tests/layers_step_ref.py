"""float32 numpy restatement of the layered in-between frames (DESIGN.md "Layered in-between frames"): `step`, the flow
from the layered composite of a state a of all layers to a second state b, and `OccStep`, the forward occlusion of that
link in the composite's pixel domain.  On top of occ_ref (triangles, cell ranges, `_bary`, `own_max_tri`),
occ_layers_ref (fields, cases) and mid_ref.

`layers_step_ref` is vectorised; `layers_step_brute` is a plain sequential Python statement of the definitions, for
tiny grids only.  Both take `fields_a`, `fields_b` [n][H][W][2], the layers' positions in the two states, and evaluate
every float expression in the kernels' order, one IEEE float32 operation at a time.
"""
import numpy as np

import mid_ref
import occ_layers_ref as lref
import occ_ref
from occ_ref import F


def _tables(masks, fields):
    """per layer: occ_ref's triangle table and every (triangle row, cell) pair raster_tri's loop visits"""
    n, H, W = masks.shape
    out = []
    for l in range(n):
        t, corners, (pa, pb, pc) = occ_ref._triangles(fields[l], masks[l])
        out.append((t, corners, (pa, pb, pc), occ_ref._pairs(*occ_ref._cell_ranges(W, H, pa, pb, pc))))
    return out


def winners(masks, fields):
    """the composite's winner per pixel: (layer, triangle), -1 where nothing is drawn; and the layers' tables"""
    n, H, W = masks.shape
    tabs = _tables(masks, fields)
    wl, wt = np.full(W * H, -1, np.int64), np.full(W * H, -1, np.int64)
    for l, (t, _, (pa, pb, pc), (k, x, y)) in enumerate(tabs):
        ok = occ_ref._bary(pa[k, 0], pa[k, 1], pb[k, 0], pb[k, 1], pc[k, 0], pc[k, 1], x.astype(F), y.astype(F))[0]
        win = np.full(W * H, -1, np.int64)
        np.maximum.at(win, (x + W * y)[ok], t[k[ok]])
        wl, wt = np.where(win >= 0, l, wl), np.where(win >= 0, win, wt)     # the higher layer on top
    return wl, wt, tabs


def _in_frame(d, W, H):
    with np.errstate(invalid="ignore"):
        return (d[:, 0] >= 0) & (d[:, 0] <= F(W - 1)) & (d[:, 1] >= 0) & (d[:, 1] <= F(H - 1))


def layers_step_ref(masks, fields_a, fields_b, parts=False):
    """-> dict(step f32[H,W,2], occlusion_step u8[H,W], warped_mask u8[H,W]).  With `parts` also the flags by cause:
    `out` (d leaves the frame), `same` (a hit with l' == l), `higher` (a hit with l' > l, uncovered pixels included)"""
    masks = np.asarray(masks)
    n, H, W = masks.shape
    N = W * H
    fields_a, fields_b = np.ascontiguousarray(fields_a, F), np.ascontiguousarray(fields_b, F)
    wl, wt, tabs = winners(masks, fields_a)
    covered = wl >= 0
    idx = np.arange(N)
    d = np.stack([(idx % W).astype(F), (idx // W).astype(F)], -1)      # an uncovered pixel asks at d = q
    M = np.full(N, -1, np.int64)
    for l in range(n):
        t, (ax, ay, bx, by, cx, cy), (pa, pb, pc), _ = tabs[l]
        q = np.flatnonzero(wl == l)
        r = np.searchsorted(t, wt[q])
        qx, qy = (q % W).astype(F), (q // W).astype(F)
        ok, b0, b1, b2 = occ_ref._bary(pa[r, 0], pa[r, 1], pb[r, 0], pb[r, 1], pc[r, 0], pc[r, 1], qx, qy)
        assert ok.all()
        Pb = fields_b[l].reshape(-1, 2)
        i0, i1, i2 = ax[r] + W * ay[r], bx[r] + W * by[r], cx[r] + W * cy[r]
        with np.errstate(invalid="ignore", over="ignore"):
            for c in range(2):
                d[q, c] = (Pb[i0, c] * b0 + Pb[i1, c] * b1) + Pb[i2, c] * b2
        m = occ_ref.own_max_tri(masks[l]).ravel()
        M[q] = np.maximum(m[i0], np.maximum(m[i1], m[i2]))
    step = np.zeros((N, 2), F)
    with np.errstate(invalid="ignore", over="ignore"):
        step[covered, 0] = d[covered, 0] - (idx[covered] % W).astype(F)
        step[covered, 1] = d[covered, 1] - (idx[covered] // W).astype(F)
    inside = _in_frame(d, W, H)
    out_f = covered & ~inside
    same, higher = np.zeros(N, bool), np.zeros(N, bool)
    # the query: in-frame points binned by the cell of d, tested by every triangle of every layer placed by b
    vs = np.flatnonzero(inside)
    cell = np.floor(d[vs, 0]).astype(np.int64) + W * np.floor(d[vs, 1]).astype(np.int64)
    order = np.argsort(cell, kind="stable")
    vs, cell = vs[order], cell[order]
    start = np.searchsorted(cell, np.arange(N + 1))
    for lp, (t, _, (pa, pb, pc), (k, x, y)) in enumerate(_tables(masks, fields_b)):
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
    occ = np.where(out_f | same | higher, 255, 0).astype(np.uint8)
    out = dict(step=step.reshape(H, W, 2), occlusion_step=occ.reshape(H, W),
               warped_mask=np.where(covered, 255, 0).astype(np.uint8).reshape(H, W))
    if parts:
        out.update(out=out_f.reshape(H, W), same=same.reshape(H, W), higher=higher.reshape(H, W))
    return out


def layers_step_brute(masks, fields_a, fields_b):
    """the definitions, sequentially: layer after layer in the quad loop under a, later writes winning; then every pixel
    on its own against every triangle placed by b.  -> dict(step, occlusion_step, warped_mask)"""
    masks = np.asarray(masks)
    n, H, W = masks.shape
    A, B = np.ascontiguousarray(fields_a, F), np.ascontiguousarray(fields_b, F)
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

    tris = []                                     # (layer, index, [corner (gx, gy)]) in (layer, index) order
    for l in range(n):
        for uy in range(H - 1):
            for ux in range(W - 1):
                if all(masks[l, y, x] == 0 for x, y in ((ux, uy), (ux + 1, uy), (ux, uy + 1), (ux + 1, uy + 1))):
                    u = ux + W * uy
                    tris.append((l, 2 * u, [(ux, uy), (ux + 1, uy), (ux, uy + 1)]))
                    tris.append((l, 2 * u + 1, [(ux, uy + 1), (ux + 1, uy), (ux + 1, uy + 1)]))
    win = {}
    for l, ti, cs in tris:
        p = [A[l, gy, gx] for gx, gy in cs]
        for y in range(H):
            for x in range(W):
                if visits(p, x, y) and bary(*p, F(x), F(y)) is not None:
                    win[(x, y)] = (l, ti, cs)     # later triangles, then later layers, overwrite
    step = np.zeros((H, W, 2), F)
    occ = np.zeros((H, W), np.uint8)
    wmask = np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            if (x, y) not in win:
                l, m, d = -1, -1, (F(x), F(y))    # below every layer, at d = q
            else:
                wmask[y, x] = 255
                l, ti, cs = win[(x, y)]
                b = bary(*[A[l, gy, gx] for gx, gy in cs], F(x), F(y))
                pb = [B[l, gy, gx] for gx, gy in cs]
                with np.errstate(all="ignore"):
                    d = tuple((pb[0][c] * b[0] + pb[1][c] * b[1]) + pb[2][c] * b[2] for c in range(2))
                    step[y, x] = (d[0] - F(x), d[1] - F(y))
                # M(t): over the corners of t, the largest triangle of layer l with that corner
                m = max(tj for lt, tj, cj in tris if lt == l and any(c in cj for c in cs))
            if not (d[0] >= 0 and d[0] <= F(W - 1) and d[1] >= 0 and d[1] <= F(H - 1)):
                occ[y, x] = 255
                continue
            cx, cy = int(np.floor(d[0])), int(np.floor(d[1]))
            for lt, tj, cj in tris:
                if not (lt > l or (lt == l and tj > m)):
                    continue
                p = [B[lt, gy, gx] for gx, gy in cj]
                if visits(p, cx, cy) and bary(*p, d[0], d[1]) is not None:
                    occ[y, x] = 255
                    break
    return dict(step=step, occlusion_step=occ, warped_mask=wmask)


def union_of_single(masks, fields_a, fields_b):
    """what n separate one-layer step occlusions give, merged as the composite is: a covered pixel takes the map of its
    winner's layer alone, an uncovered one is 255 where any layer alone flags it.  OccStep differs from this exactly
    where layers interact."""
    masks = np.asarray(masks)
    n, H, W = masks.shape
    wl = winners(masks, np.ascontiguousarray(fields_a, F))[0].reshape(H, W)
    single = np.stack([layers_step_ref(masks[l][None], fields_a[l][None], fields_b[l][None])["occlusion_step"]
                       for l in range(n)])
    occ = np.where(wl < 0, single.max(0), 0).astype(np.uint8)
    for l in range(n):
        occ[wl == l] = single[l][wl == l]
    return occ


def merged_single_steps(masks, fields_a, fields_b):
    """the host merge of n per-layer mid_ref.step_ref results by pipeline.merge_backward's selection: the last layer
    whose own warped mask covers q wins"""
    from arap_flow_amd import pipeline
    masks = np.asarray(masks)
    n = masks.shape[0]
    steps = [mid_ref.step_ref(masks[l], fields_a[l], fields_b[l]) for l in range(n)]
    covers = [mid_ref.winners(masks[l], fields_a[l])[0].reshape(masks.shape[1:]) >= 0 for l in range(n)]
    return pipeline.merge_backward(steps, covers, masks == 0)[0]


def two_state_layers(W, H, n, seed, overlap=False):
    """(rgb, masks, flows_a, flows_b): lref.layered_case for state a; state b is another folded draw with other
    whole-pixel shifts, so the layers pass over each other and partly leave the frame between a and b"""
    rgb, masks, fa = lref.layered_case(W, H, n, seed, overlap=overlap)
    rng = np.random.default_rng(seed + 5000)
    fb = fa + (rng.normal(size=fa.shape) * 0.8).astype(np.float32)
    for l in range(n):
        fb[l] += np.array([rng.integers(-max(W // n, 1), max(W // n, 1) + 1), rng.integers(-2, 3)], np.float32)
        fb[l][masks[l] != 0] = 0
    return rgb, masks, fa, fb


def rectangles_case():
    """closed form: two rectangles, the lower at rest in both states, the upper translated by whole pixels between a and
    b.  Returns masks, flows_a, flows_b and the expected OccStep set: the lower-layer and background pixels of the
    composite of a that the upper rectangle newly covers in b."""
    W, H = 16, 12
    masks = np.full((2, H, W), 255, np.uint8)
    masks[0, 2:10, 1:9] = 0                       # lower, at rest: x 1..8, y 2..9
    masks[1, 3:9, 10:15] = 0                      # upper: x 10..14, y 3..8
    fa = np.zeros((2, H, W, 2), np.float32)
    fb = np.zeros((2, H, W, 2), np.float32)
    fa[1][masks[1] == 0] = (-2.0, 0.0)            # state a: x 8..12, y 3..8
    fb[1][masks[1] == 0] = (-6.0, -2.0)           # state b: x 4..8,  y 1..6 (row 1 is background)
    ys, xs = np.mgrid[0:H, 0:W]
    in_a = (xs >= 8) & (xs <= 12) & (ys >= 3) & (ys <= 8)
    in_b = (xs >= 4) & (xs <= 8) & (ys >= 1) & (ys <= 6)
    return masks, fa, fb, in_b & ~in_a


# (W, H, layers, seed, overlapping masks): the shapes of the layered warp's tests; they cross block, tile and cell
# edges.
# The seeds are fixed so that every multi-layer case meets exercised() below (test_layers_step_host.py shows it).
MULTI = [(10, 8, 3, 3, False), (12, 7, 4, 1, False), (10, 8, 3, 2, True), (70, 50, 3, 1, False), (129, 65, 5, 1, True),
         (64, 4, 2, 6, False)]
# one quad; one column and one row, no rasterised quad: every pixel is an uncovered query at its own cell
SINGLE = [(2, 2, 1, 8, False), (1, 5, 1, 9, False), (5, 1, 1, 10, False)]


def exercised(masks, fields_a, fields_b):
    """the conditions on a multi-layer input, from the restatement alone: OccStep is not the union of the layers' own
    step occlusions (the cross-layer rule acts), a pixel is flagged by the same-layer rule t' > M(t), one by !in_frame,
    and step is non-zero on covered pixels.  -> dict of bools"""
    r = layers_step_ref(masks, fields_a, fields_b, parts=True)
    covered = r["warped_mask"] != 0
    return dict(cross=bool((r["occlusion_step"] != union_of_single(masks, fields_a, fields_b)).any()),
                same=bool(r["same"].any()), out=bool(r["out"].any()), moves=bool((r["step"][covered] != 0).any()))
