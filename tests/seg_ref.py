"""float32 numpy twin of DESIGN.md "Segment maps" (arap_flow_amd/csrc/arap_seg.h).

`seg_ref` is vectorised: the frame-2 winner and backward flow come from occ_layers_ref.layers_ref, the background's flow
from bg_ref.apply_map, the jump test is the stated float32 operators in their order, and the distance is an explicit
minimum over ALL boundary pixels of the frame (no separable passes, no window).  `seg_loops` states the same per pixel in
plain Python loops, on occ_layers_ref.layers_brute, for tiny frames only.  The point maps G / Ginv are an input (the tests
take them from ArapFlow_BackgroundMaps or bg_ref.maps_f64), None for a static background.
"""
import numpy as np

import bg_ref
import occ_layers_ref
from bg_ref import F

FAR = 65535
OUTPUTS = ("idx1", "idx2", "mb1", "mb2", "dist1", "dist2")


def full_flow(obj_flow, has, Gmap):
    """the object-side flow where `has`, elsewhere the background's: G(x, y) - (x, y), or exactly 0 without a map"""
    H, W = has.shape
    bgf = np.zeros((H, W, 2), F)
    if Gmap is not None:
        ys, xs = np.mgrid[0:H, 0:W]
        px, py = bg_ref.apply_map(Gmap, W, H)
        bgf = np.stack([px - xs.astype(F), py - ys.astype(F)], -1).astype(F)
    return np.where(has[..., None], obj_flow, bgf).astype(F)


def boundaries(flow, tau):
    """mb: 255 where !(dx * dx + dy * dy <= tau * tau) against a 4-neighbour inside the frame, float32 throughout"""
    flow = np.asarray(flow, F)
    H, W = flow.shape[:2]
    with np.errstate(all="ignore"):
        tau2 = F(tau) * F(tau)
        mb = np.zeros((H, W), bool)
        for a, b in ((np.s_[:, 1:], np.s_[:, :-1]), (np.s_[1:, :], np.s_[:-1, :])):
            d = flow[a] - flow[b]
            jump = ~(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] <= tau2)
            mb[a] |= jump
            mb[b] |= jump
    return np.where(mb, 255, 0).astype(np.uint8)


def nearest2(mb):
    """the squared distance of every pixel to the nearest pixel of mb, the minimum over every boundary pixel of the
    frame, in integers; a huge value in a frame without boundary"""
    H, W = mb.shape
    by, bx = (a.astype(np.int32) for a in np.nonzero(mb))
    best = np.full(H * W, np.iinfo(np.int32).max, np.int32)
    ys, xs = (a.ravel().astype(np.int32)[:, None] for a in np.mgrid[0:H, 0:W])
    for k in range(0, len(by), 128):
        best = np.minimum(best, ((xs - bx[k:k + 128]) ** 2 + (ys - by[k:k + 128]) ** 2).min(-1))
    return best.reshape(H, W)


def distances(mb, radius, near=None):
    """dist: nearest2 where <= radius^2, else FAR (`near`: nearest2(mb), if the caller has it)"""
    near = nearest2(mb) if near is None else near
    return np.where(near <= radius * radius, near, FAR).astype(np.uint16)


def seg_ref(masks, flows, tau, radius, G=None, Ginv=None):
    """-> dict of OUTPUTS plus the full flows F1, B2"""
    masks = np.asarray(masks, np.uint8)
    flows = np.ascontiguousarray(flows, F)
    n, H, W = masks.shape
    own = occ_layers_ref.owner_of(masks)
    out = dict(idx1=(own + 1).astype(np.uint8))
    fields = occ_layers_ref.fields_from_flows(flows)
    lay = occ_layers_ref.layers_ref(None, masks, fields)
    idx2 = np.zeros((H, W), np.uint8)
    for l in range(n):                      # what a layer covers does not depend on the others; the largest layer wins
        alone = occ_layers_ref.layers_ref(None, masks[l:l + 1], fields[l:l + 1])["warped_mask"]
        idx2[alone != 0] = l + 1
    assert ((idx2 != 0) == (lay["warped_mask"] != 0)).all()
    out["idx2"] = idx2
    ys, xs = np.mgrid[0:H, 0:W]
    out["F1"] = full_flow(flows[np.maximum(own, 0), ys, xs], own >= 0, G)
    out["B2"] = full_flow(lay["backward_flow"], idx2 != 0, Ginv)
    for f, key in (("1", "F1"), ("2", "B2")):
        out["mb" + f] = boundaries(out[key], tau)
        out["dist" + f] = distances(out["mb" + f], radius)
    return out


def seg_loops(masks, flows, tau, radius, G=None, Ginv=None):
    """the definitions, pixel by pixel (tiny frames only) -> dict of OUTPUTS"""
    masks = np.asarray(masks, np.uint8)
    flows = np.ascontiguousarray(flows, F)
    n, H, W = masks.shape
    fields = occ_layers_ref.fields_from_flows(flows)
    lay = occ_layers_ref.layers_brute(None, masks, fields)
    alone = [occ_layers_ref.layers_brute(None, masks[l:l + 1], fields[l:l + 1])["warped_mask"] for l in range(n)]

    def bg(m, x, y):
        if m is None:
            return F(0), F(0)
        m = np.asarray(m, F)
        fx, fy = F(x), F(y)
        px = bg_ref.fma(m[0], fx, bg_ref.fma(m[1], fy, m[2]))
        py = bg_ref.fma(m[3], fx, bg_ref.fma(m[4], fy, m[5]))
        return F(px - fx), F(py - fy)

    idx1, idx2 = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    F1, B2 = np.zeros((H, W, 2), F), np.zeros((H, W, 2), F)
    for y in range(H):
        for x in range(W):
            for l in range(n):
                if masks[l, y, x] == 0:
                    idx1[y, x] = l + 1              # the largest such l stays
            F1[y, x] = flows[idx1[y, x] - 1, y, x] if idx1[y, x] else bg(G, x, y)
            if lay["warped_mask"][y, x]:
                for l in range(n):                  # the winner's layer: the largest one that covers (x, y) on its own
                    if alone[l][y, x]:
                        idx2[y, x] = l + 1
                B2[y, x] = lay["backward_flow"][y, x]
            else:
                B2[y, x] = bg(Ginv, x, y)
    out = dict(idx1=idx1, idx2=idx2)
    with np.errstate(all="ignore"):
        tau2 = F(tau) * F(tau)
        for f, flow in (("1", F1), ("2", B2)):
            mb = np.zeros((H, W), np.uint8)
            for y in range(H):
                for x in range(W):
                    for qx, qy in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)):
                        if not (0 <= qx < W and 0 <= qy < H):
                            continue
                        dx, dy = F(flow[y, x, 0] - flow[qy, qx, 0]), F(flow[y, x, 1] - flow[qy, qx, 1])
                        d2 = F(F(dx * dx) + F(dy * dy))
                        if not d2 <= tau2:
                            mb[y, x] = 255
            dist = np.full((H, W), FAR, np.uint16)
            marks = [(x, y) for y in range(H) for x in range(W) if mb[y, x]]
            for y in range(H):
                for x in range(W):
                    d = min([(x - bx) ** 2 + (y - by) ** 2 for bx, by in marks], default=None)
                    if d is not None and d <= radius * radius:
                        dist[y, x] = d
            out["mb" + f], out["dist" + f] = mb, dist
    return out


def seg_case(W, H, n, seed=0):
    """n overlapping layers for the tests: vertical bands two pixels into their right neighbour, a few background holes,
    per-layer whole-pixel shifts that throw the layers over each other, a smooth flow on layer 0 with a fold strictly
    inside it (a patch of vertices thrown across their neighbours), and a NaN vertex inside the last layer"""
    rng = np.random.default_rng(seed)
    masks = np.full((n, H, W), 255, np.uint8)
    edges = np.linspace(0, W, n + 1).astype(int)
    flows = np.zeros((n, H, W, 2), F)
    for l in range(n):
        a, b = edges[l], min(edges[l + 1] + (2 if l + 1 < n else 0), W)
        masks[l, :, a:b] = 0
        masks[l][rng.random((H, W)) < 0.03] = 255
        flows[l] += np.array([(-1) ** l * max(1, (b - a) // 3), l % 2], F)
    ys, xs = np.mgrid[0:H, 0:W]
    flows[0, ..., 0] += (0.125 * np.sin(ys / 3.0)).astype(F)           # smooth: far below tau = 1 between neighbours
    fy, fx = H // 2, max(1, (edges[1] - edges[0]) // 2)
    masks[0, max(fy - 2, 0):fy + 3, max(fx - 2, 0):fx + 3] = 0
    flows[0, fy, fx] += np.array([-2.5, 0.0], F)                       # the fold: one vertex across its left neighbour
    ny, nx = H // 3, min(edges[n - 1] + max(2, (W - edges[n - 1]) // 2), W - 1)
    masks[n - 1, max(ny - 1, 0):ny + 2, max(nx - 1, 0):nx + 2] = 0
    flows[n - 1, ny, nx, 0] = np.nan
    for l in range(n):
        flows[l][masks[l] != 0] = 0
    return masks, flows, (fx, fy), (nx, ny)
