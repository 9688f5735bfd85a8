"""Hostile warp fields (DESIGN.md "Hostile fields"): the inputs the warp family must survive in production and that no
smooth or normally distributed flow ever reaches -- NaN corners, +-Inf and 1e30 positions, finite giant triangles,
zero-area and collinear triangles, exact ties on vertices and shared edges, thousands of vertices in one cell,
positions on and one ulp outside the frame's edge, products in the subnormal range.

Every family is built as a FLOW, the form the entry points take; its field is occ_ref.field_from_flow of that flow, so
`field = (float)x + flow` holds bit for bit and the restatements see exactly the positions the kernels compute.  Two
consequences of IEEE addition, kept as they are: a position is never -0.0 ((+0) + (-0) = +0; `edges` passes the -0.0 as
a flow value), and a position below 1 ulp of its vertex's grid coordinate exists only where that coordinate is 0, so
`tiny` leaves column 0 and row 0 with positions of about 1e-20 and collapses every other coordinate to exactly 0.

`case` gives one (family, mask) input with the restatement's answer and the probe the `exercised` and `defined`
conditions read, computed once per process.  The conditions come from the restatement alone.
"""
import functools

import numpy as np

import occ_ref
from occ_ref import F

NAMES = ("int", "half", "naninf", "huge30", "huge6", "tiny", "fewpoints", "line", "rot180", "edges")
QUADRATIC = ("fewpoints", "line", "tiny")       # all vertices in a few cells: the numpy query is quadratic in N
MASKS = ("random", "strip")
SHAPES = ((12, 9), (67, 9), (129, 65))          # one block; W no multiple of 64, H none of 4; three scan chunks, N % 4 = 1
SCAN_SHAPES = ((65, 63), (64, 64), (241, 17))   # N = 4095, 4096, 4097 around the scan's chunk of 4096 counts
SCAN_CHUNK = 4096
KEYS = ("warped_rgb", "warped_mask", "backward_flow", "occlusion_bwd", "occlusion")
# every family at every shape, but the quadratic ones at the largest
CASES = [(W, H, name) for W, H in SHAPES for name in NAMES if not ((W, H) == SHAPES[-1] and name in QUADRATIC)]


def grid(W, H):
    ys, xs = np.mgrid[0:H, 0:W]
    return np.stack([xs, ys], -1).astype(F)


def _pick(rng, N, frac, groups):
    """`groups` disjoint random index sets of max(2, round(frac N)) vertices each"""
    k = max(2, int(round(frac * N)))
    p = rng.permutation(N)
    return [p[g * k:(g + 1) * k] for g in range(groups)]


def _edge_flow(W, H):
    """the grid with chosen vertices on, and one ulp outside, the frame's edge: per row one vertex's x, per column one
    vertex's y, the variant by the row / column number modulo 6.  Every target is reached exactly (asserted)."""
    f = np.zeros((H, W, 2), F)
    want = []
    for axis, (n_other, size) in enumerate(((H, W), (W, H))):
        last = F(size - 1)
        below, above = np.nextafter(F(0), F(-np.inf)), np.nextafter(last, F(np.inf))
        variants = [(0, F(-0.0), F(0)),                     # a -0.0 flow at coordinate 0: the position is +0
                    (0, below, below),                      # one ulp below 0: outside
                    (2, F(-2), F(0)),                       # exactly 0 from inside
                    (size - 3, F(2), last),                 # exactly size - 1 from inside
                    (size - 1, above - last, above),        # one ulp above size - 1: outside
                    (1, F(size - 2), last)]                 # exactly size - 1 from the far side: a long thin triangle
        for o in range(n_other):
            at, val, target = variants[o % 6]
            idx = (o, at, 0) if axis == 0 else (at, o, 1)
            f[idx] = val
            want.append((idx, target))
    field = occ_ref.field_from_flow(f)
    for idx, target in want:
        assert field[idx].tobytes() == F(target).tobytes(), (idx, field[idx], target)
    return f


def flows(W, H, seed, few=None):
    """{name: flow f32[H,W,2]}, deterministic in (W, H, seed).  `few`: the points `fewpoints` collapses onto, as
    [(x, y, weight)]; by default the four points (W//2 + {0,1}, H//2 + {0,1}) alike."""
    rng = np.random.default_rng([W, H, seed])
    N = W * H
    g = grid(W, H)
    out = {}
    out["int"] = rng.integers(-3, 4, (H, W, 2)).astype(F)
    out["half"] = (rng.integers(-6, 7, (H, W, 2)) * 0.5).astype(F)
    f = rng.normal(size=(H, W, 2)).astype(F)
    a, b, c = _pick(rng, N, 0.03, 3)
    f.reshape(-1, 2)[a, 0] = np.nan
    f.reshape(-1, 2)[b, 1] = np.inf
    f.reshape(-1, 2)[c, 0] = -np.inf
    out["naninf"] = f
    for name, scale in (("huge30", 1e30), ("huge6", 1e6)):
        noise = rng.normal(size=(H, W, 2)).astype(F)
        f = noise.copy()
        sel, = _pick(rng, N, 0.02, 1)
        sign = rng.choice(np.array([-1, 1], F), (len(sel), 2))
        f.reshape(-1, 2)[sel] = (g + noise).reshape(-1, 2)[sel] * sign * F(scale)
        out[name] = f
    out["tiny"] = (g + rng.normal(size=(H, W, 2)).astype(F)) * F(1e-20) - g
    if few is None:
        few = [(W // 2 + a, H // 2 + b, 1.0) for b in (0, 1) for a in (0, 1)]
    pts = np.array([(x, y) for x, y, _ in few], F)
    w = np.array([q for _, _, q in few], np.float64)
    out["fewpoints"] = pts[rng.choice(len(pts), (H, W), p=w / w.sum())] - g
    f = rng.normal(size=(H, W, 2)).astype(F)
    f[..., 1] = F(H // 2 + 0.5) - g[..., 1]
    out["line"] = f
    out["rot180"] = np.stack([F(W - 1) - 2 * g[..., 0], F(H - 1) - 2 * g[..., 1]], -1).astype(F)
    out["edges"] = _edge_flow(W, H)
    assert tuple(out) == NAMES and all(v.dtype == F and v.shape == (H, W, 2) for v in out.values())
    return out


def families(W, H, seed, few=None):
    """{name: field f32[H,W,2]}: the positions of `flows`, field = (float)x + flow bit for bit"""
    with np.errstate(all="ignore"):
        return {k: occ_ref.field_from_flow(v) for k, v in flows(W, H, seed, few).items()}


def masks(W, H, seed):
    """a 10 % random background; a one-vertex-wide strip of object: vertices without a triangle, m(v) = -1"""
    rng = np.random.default_rng([W, H, seed, 1])
    strip = np.full((H, W), 255, np.uint8)
    strip[H // 2, :] = 0
    return dict(random=np.where(rng.random((H, W)) < 0.1, 255, 0).astype(np.uint8), strip=strip)


def colours(W, H, seed):
    return np.random.default_rng([W, H, seed, 2]).integers(0, 256, (H, W, 3)).astype(np.uint8)


def scan_few(W, H):
    """`fewpoints` for the scan shapes: the collapse points in the first cells, so that the start of every later cell is
    a carry of about N, and -- else no later start would ever be read -- one point in twenty on the last cell"""
    return [(0, 0, 1.0), (1, 0, 1.0), (0, 1, 1.0), (1, 1, 1.0), (W - 1, H - 1, 0.2)]


def probe(rgb, mask, field):
    """what the conditions read, from occ_ref's own pieces: the (triangle, cell) pairs the rasteriser accepts, their
    barycentrics and colour mixes, the triangles skipped for a NaN corner, the most cells one triangle visits, and the
    binning of the in-frame object vertices"""
    H, W = mask.shape
    field = np.ascontiguousarray(field, F)
    t, (ax, ay, bx, by, cx, cy), (pa, pb, pc) = occ_ref._triangles(field, mask)
    nan_tri = np.isnan(pa).any(1) | np.isnan(pb).any(1) | np.isnan(pc).any(1)
    xa, ya, nx, ny = occ_ref._cell_ranges(W, H, pa, pb, pc)
    k, x, y = occ_ref._pairs(xa, ya, nx, ny)
    ok, b0, b1, b2 = occ_ref._bary(pa[k, 0], pa[k, 1], pb[k, 0], pb[k, 1], pc[k, 0], pc[k, 1], x.astype(F), y.astype(F))
    k, bary = k[ok], np.stack([b0[ok], b1[ok], b2[ok]], -1)
    img = rgb.reshape(-1, 3).astype(F)
    with np.errstate(all="ignore"):
        s = np.stack([(img[ax[k] + W * ay[k], c] * bary[:, 0] + img[bx[k] + W * by[k], c] * bary[:, 1]) +
                      img[cx[k] + W * cy[k], c] * bary[:, 2] for c in range(3)], -1)
    P = field.reshape(-1, 2)
    obj = (mask == 0).ravel()
    with np.errstate(invalid="ignore"):
        inside = (P[:, 0] >= 0) & (P[:, 0] <= F(W - 1)) & (P[:, 1] >= 0) & (P[:, 1] <= F(H - 1))
    vs = np.flatnonzero(obj & inside)
    cell = np.floor(P[vs, 0]).astype(np.int64) + W * np.floor(P[vs, 1]).astype(np.int64)
    return dict(accepted=int(ok.sum()), zero_bary=int((bary == 0).any(1).sum()), bary_finite=bool(np.isfinite(bary).all()),
                colour_defined=bool(((s >= 0) & (s < 256)).all()), nan_triangles=int(nan_tri.sum()),
                most_cells=int((nx * ny).max()) if len(nx) else 0,
                cell_counts=np.bincount(cell, minlength=W * H), inside=inside, object=obj)


def exercised(name, case):
    """does the input still do its family's job?  Conditions on the restatement, asserted before any GPU result is
    looked at.  They are stated for the random mask (the strip has no triangle)."""
    p, ref, field, mask = case["probe"], case["ref"], case["field"], case["mask"]
    H, W = mask.shape
    N = W * H
    covered = int((ref["warped_mask"] != 0).sum())
    occluded = int(((ref["occlusion"] == 255) & (mask == 0)).sum())
    if name in ("int", "half"):
        return p["accepted"] > 0 and 10 * p["zero_bary"] >= p["accepted"]
    if name == "naninf":
        return p["nan_triangles"] >= 1 and covered > 0
    if name == "huge30":
        big = np.abs(field.reshape(-1, 2)[p["object"]]) > 1e29
        return bool(big.any()) and covered > 0
    if name == "huge6":
        return 2 * p["most_cells"] >= N
    if name == "fewpoints":
        return 8 * int(p["cell_counts"].max()) >= N and occluded >= 1
    if name == "tiny":
        v = np.abs(field.reshape(-1, 2)[p["object"]])
        sub = [a[(a > 0) & (a < 1e-19)] for a in (v[:, 0], v[:, 1])]       # their products are subnormal in float32
        return p["accepted"] == 0 and all(len(a) for a in sub) and 0 < float(sub[0].min()) * float(sub[1].min()) < 1.2e-38
    if name == "line":
        return p["accepted"] == 0
    if name == "rot180":
        return covered > 0
    if name == "edges":
        P = field.reshape(-1, 2)[p["object"]]
        ok = True
        for axis, size in ((0, W), (1, H)):
            last = F(size - 1)
            for on, off in ((F(0), np.nextafter(F(0), F(-np.inf))), (last, np.nextafter(last, F(np.inf)))):
                ok = ok and bool((P[:, axis] == on).any()) and bool((P[:, axis] == off).any())
        return ok and bool(p["inside"][p["object"]].any()) and bool((~p["inside"][p["object"]]).any())
    raise KeyError(name)


def defined(case):
    """the definedness guard: every accepted pair has finite barycentrics and every colour mix s has 0 <= s < 256, so the
    reference's float -> byte conversion is defined on the whole family"""
    return case["probe"]["bary_finite"] and case["probe"]["colour_defined"]


def scan_exercised(case):
    """fewpoints on a scan shape: the start of the last cell is a carry of at least 0.9 of the binned points, at least
    N / 2 of them, and -- where N has a second chunk -- points are binned behind the first"""
    c = case["probe"]["cell_counts"]
    total = int(c.sum())
    later = int(c[SCAN_CHUNK:].sum())
    return 2 * total >= len(c) and 10 * int(c[:-1].sum()) >= 9 * total and int(c[-1]) > 0 and (len(c) <= SCAN_CHUNK or later > 0)


@functools.lru_cache(maxsize=None)
def case(W, H, name, mask_name, seed=0, scan=False):
    """one input and the restatement's answer: dict(rgb, mask, flow, field, ref, probe); shared, leave it unchanged"""
    few = scan_few(W, H) if scan else None
    flow = flows(W, H, seed, few)[name]
    with np.errstate(all="ignore"):
        field = occ_ref.field_from_flow(flow)
    rgb, mask = colours(W, H, seed), masks(W, H, seed)[mask_name]
    return dict(rgb=rgb, mask=mask, flow=flow, field=field, ref=occ_ref.warp_ref(rgb, mask, field),
                probe=probe(rgb, mask, field))


def same_float(a, b):
    """bit for bit but for a NaN's sign and payload: NaNs in the same places, equal bits everywhere else"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


# ---- the inputs of the routes that take more than one field --------------------------------------------------------------
def benign_flow(W, H, seed, amp=1.5):
    """a folded normal flow of a few pixels: the kind of input every other test of the family uses"""
    return (np.random.default_rng([W, H, seed, 3]).normal(size=(H, W, 2)) * amp).astype(F)


def band_mask(W, H, seed, lo, hi):
    """object on the columns lo <= x < hi, with 8 % background holes"""
    m = np.full((H, W), 255, np.uint8)
    m[:, lo:hi] = 0
    m[np.random.default_rng([W, H, seed, 4]).random((H, W)) < 0.08] = 255
    return m


def step_inputs(W, H, name, mask_name, seed=0):
    """[(tag, mask, flow_a, flow_b)]: the hostile field once as state a and once as state b, the other state `int`"""
    c = case(W, H, name, mask_name, seed)
    other = flows(W, H, seed + 1)["int"]
    return [("a", c["mask"], c["flow"], other), ("b", c["mask"], other, c["flow"])]


def layer_inputs(W, H, name, mask_name, seed=0):
    """[(tag, masks, flows)]: two layers with the hostile one below and above a benign band (x >= W/3), and three with
    it between that band and an `int` band (x < W/2).  The hostile layer keeps the family's whole mask."""
    c = case(W, H, name, mask_name, seed)
    right, left = band_mask(W, H, seed, W // 3, W), band_mask(W, H, seed + 1, 0, W // 2 + 1)
    ben, other = benign_flow(W, H, seed), flows(W, H, seed + 1)["int"]
    return [("below", np.stack([c["mask"], right]), np.stack([c["flow"], ben])),
            ("above", np.stack([right, c["mask"]]), np.stack([ben, c["flow"]])),
            ("between", np.stack([left, c["mask"], right]), np.stack([other, c["flow"], ben]))]


def layers_step_inputs(W, H, name, mask_name, seed=0):
    """[(tag, masks, flows_a, flows_b)]: a benign band below the hostile layer; the hostile field as the upper layer's
    state a, as its state b, and (another draw of the family) as both; `int` where it is not hostile"""
    c = case(W, H, name, mask_name, seed)
    masks_ = np.stack([band_mask(W, H, seed, W // 3, W), c["mask"]])
    ben_a, ben_b = benign_flow(W, H, seed), benign_flow(W, H, seed + 1, 2.0)
    other, again = flows(W, H, seed + 1)["int"], flows(W, H, seed + 1)[name]
    return [("a", masks_, np.stack([ben_a, c["flow"]]), np.stack([ben_b, other])),
            ("b", masks_, np.stack([ben_a, other]), np.stack([ben_b, c["flow"]])),
            ("both", masks_, np.stack([ben_a, c["flow"]]), np.stack([ben_b, again]))]


def track_inputs(W, H, name, mask_name, seed=0):
    """(masks [1,H,W], flows [2,1,H,W,2], points): one layer, the states (hostile, `int`), and track_ref's point set --
    the integer pixels, sub-pixel and quarter-lattice points, the frame's edge, points outside it and a NaN point"""
    import track_ref
    c = case(W, H, name, mask_name, seed)
    fl = np.stack([c["flow"], flows(W, H, seed + 1)["int"]])[:, None]
    return c["mask"][None], fl, track_ref.case_points(W, H, seed)


def fields_of(flows_):
    """the positions of a stack of flows [..., H, W, 2]"""
    flows_ = np.asarray(flows_, F)
    with np.errstate(all="ignore"):
        return np.stack([occ_ref.field_from_flow(f) for f in flows_.reshape((-1,) + flows_.shape[-3:])]).reshape(flows_.shape)
