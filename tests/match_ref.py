"""Stage-by-stage checks of the matcher (arap_flow_amd/csrc_dm/arapmatch.hip) against oracle/dm_oracle.py.

Every stage after the bottom-level correlation is comparisons and float32 additions in a fixed order, so GIVEN THE SAME
MAPS the restatement and the kernels agree exactly.  Each helper therefore takes what the matcher produced for stage k,
runs the oracle for stage k + 1 only, and returns (or checks) what the matcher must have produced for stage k + 1:

  descriptors --level0_f64--> level-0 maps --level_up_ref--> level l + 1 maps --backtrack_on--> match rows

No near-tie slack is needed anywhere: the only inexact steps (the 144-term sums of level 0 and the power x^1.4) are
bounded against a float64 reference, cell by cell.  `chain` runs all of it on anything with the surface of
match.Matcher (descriptors, levels, level_maps) -- the HIP matcher on the GPU, `OracleMatcher` on the CPU.
"""
import numpy as np

from oracle import dm_oracle as dm

F = np.float32
U = 2.0 ** -24                     # unit roundoff of float32
LEVEL0_TERMS = dm.PATCH * dm.PATCH * 9


def clamped_r(ngh_rad):
    """search radius of ArapMatch_Create: ngh_rad >> 1, at least 1, at most 96 (the LDS ring of k_corr0)"""
    return min(max(int(ngh_rad) >> 1, 1), 96)


# ---- stage 1: descriptors -> level-0 maps ----------------------------------------------------------------------------
def level0_f64(d1, d2, r):
    """dm.level0 in float64 on float32 descriptors: [gh][gw][2r+1][2r+1], exact to ~1e-14 relative.  Per vertical
    displacement one matrix product gives <d1(y, x), d2(y + dy, x')> for every pair of columns; the band
    x' = x + dx, |dx| <= r, summed over each patch's 4 x 4 pixels, is the cell (dy, dx)."""
    h, w = d1.shape[:2]
    P = dm.PATCH
    gh, gw = h // P, w // P
    S = 2 * r + 1
    out = np.zeros((gh, gw, S, S), np.float64)
    pad = np.zeros((h + 2 * r, w + 2 * r, 9), np.float64)
    pad[r:r + h, r:r + w] = d2
    a = d1[:gh * P, :gw * P].astype(np.float64)
    for dy in range(-r, r + 1):
        b = pad[r + dy:r + dy + gh * P]                                   # [gh P][w + 2r][9]
        D = np.ascontiguousarray(np.matmul(a, b.transpose(0, 2, 1)))    # [gh P][gw P][w + 2r]
        s0, s1, s2 = D.strides
        band = np.lib.stride_tricks.as_strided(D, (gh * P, gw * P, S), (s0, s1 + s2, s2), writeable=False)   # [y][x][dx + r] = D[y][x][x + dx + r]
        out[:, :, dy + r, :] = band.reshape(gh, P, gw, P, S).sum((1, 3)) / 16.0
    return out


def in_padding(h, w, r):
    """bool [gh][gw][S][S]: the cell's 4x4 placement in frame 2 lies entirely outside the h x w frame"""
    gh, gw = h // dm.PATCH, w // dm.PATCH
    d = np.arange(-r, r + 1)
    x0 = dm.PATCH * np.arange(gw)[:, None] + d[None, :]                  # [gw][S] first pixel column of the placement
    y0 = dm.PATCH * np.arange(gh)[:, None] + d[None, :]
    outx = (x0 + dm.PATCH - 1 < 0) | (x0 >= w)
    outy = (y0 + dm.PATCH - 1 < 0) | (y0 >= h)
    return outy[:, None, :, None] | outx[None, :, None, :]


def check_level0(got, d1, d2, r):
    """Every cell of the matcher's level-0 maps against the float64 sum of the same 144 products.

    All 144 terms are >= 0 (rectified descriptors, zero padding), so for ANY summation order -- sequential, pairwise or
    the MFMA's -- the float32 result s satisfies |s - ref| <= gamma_144 * ref with gamma_n = n u / (1 - n u), u = 2^-24
    (Higham, Accuracy and Stability of Numerical Algorithms, eq. 3.5 with the product roundings folded in: 1 rounding
    per product + at most 143 per addition chain).  gamma_144 < 144.002 u; one more u for comparing against a rounded
    reference gives 145 u.  The scaling by 1/16 is exact.  Underflow cannot break the relative bound: a cell with one
    pixel inside the frame is at least (0.3 / |d|)^2 / 16 >= 6.9e-4 (the ninth channel, |d|^2 <= 8.09), its bound
    >= 6e-9, while 144 flushed products are below 144 * 2^-126.
    Cells entirely in the zero padding are sums of +0 and must be exactly 0."""
    h, w = d1.shape[:2]
    S = 2 * r + 1
    assert got.shape == (h // dm.PATCH, w // dm.PATCH, S, S) and got.dtype == F, (got.shape, got.dtype)
    assert (d1 >= 0).all() and (d2 >= 0).all()
    ref = level0_f64(d1, d2, r)
    pad = in_padding(h, w, r)
    assert (ref[pad] == 0).all() and (ref[~pad] > 0).all()
    nz = np.flatnonzero(got[pad])
    assert nz.size == 0, "level 0: %d cells in the zero padding are not 0.0 (first: %r)" % (nz.size, np.argwhere(pad)[nz[0]])
    err = np.abs(got.astype(np.float64) - ref)
    bad = err > (LEVEL0_TERMS + 1) * U * ref
    if bad.any():
        k = np.unravel_index(np.argmax(np.where(bad, err, 0)), err.shape)
        raise AssertionError("level 0: %d of %d cells outside 145 u relative; first patch column %d; worst cell %r: got %.9g, "
                             "float64 %.9g" % (bad.sum(), bad.size, np.argwhere(bad)[:, 1].min(), k, got[k], ref[k]))
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.nanmax(np.where(ref > 0, err / ref, 0.0)) / U)                # worst error in units of u * ref


# ---- stage 2: level l -> level l + 1 ---------------------------------------------------------------------------------
def ulp_distance(a, b):
    """distance in float32 steps between arrays of non-negative finite float32"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    assert (a >= 0).all() and (b >= 0).all() and np.isfinite(a).all() and np.isfinite(b).all()
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def level_up_ref(below, level, c):
    """dm.level_up on the matcher's own maps of level `level`: (pre, ref, kids, o, c') or None when no level follows.
    pre = 0.25 * (((0 + p0) + p1) + p2) + p3 of the pooled children, float32, bit-reproducible (maxima and four
    additions in the oracle's order); ref = float32(float64(pre) ** 1.4), the correctly rounded power."""
    gh, gw, S, _ = below.shape
    nh, nw, kids = dm.children_of(level, gh, gw)
    if kids is None:
        return None
    o, S2, c2 = dm.pool_geometry(S, c)
    if S2 < 1:
        return None
    pooled = dm.maxpool(below, o)
    acc = np.zeros((nh, nw, S2, S2), F)
    for q in range(4):
        acc = acc + pooled[kids[q][..., 0], kids[q][..., 1]]
    pre = np.maximum(acc * F(0.25), F(0.0)).astype(F)
    ref = np.power(pre.astype(np.float64), np.float64(dm.LAMBDA)).astype(F)
    return pre, ref, kids, o, c2


def check_level_up(got, below, level, c, max_ulp):
    """the matcher's level `level` + 1 within max_ulp float32 steps of the correctly rounded power, exact where the
    pre-power value is 0 or 1; returns the largest distance seen"""
    up = level_up_ref(below, level, c)
    assert up is not None, "level %d exists but the oracle builds no level on level %d" % (level + 1, level)
    pre, ref, _, _, _ = up
    assert got.shape == ref.shape and got.dtype == F, (level + 1, got.shape, ref.shape)
    assert np.isfinite(got).all() and (got >= 0).all(), "level %d: negative or non-finite cells" % (level + 1)
    exact = (pre == 0) | (pre == 1)
    assert np.array_equal(got[exact], pre[exact]), "level %d: x^1.4 of an exact 0 or 1 is not exact" % (level + 1)
    d = ulp_distance(got, ref)
    if d.max() > max_ulp:
        k = np.unravel_index(np.argmax(d), d.shape)
        raise AssertionError("level %d: %d of %d cells more than %d ulp from the float64 power; worst cell %r: got %.9g, want %.9g "
                             "(%d ulp), pre-power %.9g" % (level + 1, (d > max_ulp).sum(), d.size, max_ulp, k, got[k], ref[k], d[k], pre[k]))
    return int(d.max())


# ---- stage 3: maps -> matches ----------------------------------------------------------------------------------------
def levels_from_maps(maps, cs):
    """the `levels` list dm.backtrack expects, from downloaded maps and the centres of Matcher.levels()"""
    levels = [dict(maps=maps[0], c=cs[0], kids=None, o=None)]
    for l in range(1, len(maps)):
        gh, gw, S, _ = maps[l - 1].shape
        nh, nw, kids = dm.children_of(l - 1, gh, gw)
        o, S2, c2 = dm.pool_geometry(S, cs[l - 1])
        assert maps[l].shape == (nh, nw, S2, S2) and cs[l] == c2, (l, maps[l].shape, (nh, nw, S2, S2), cs[l], c2)
        levels.append(dict(maps=maps[l], c=c2, kids=kids, o=o))
    return levels


def merge(best, cell, c0, h2, w2):
    """the merging half of dm.matches: one match per 4x4 cell of frame 2 (h2 x w2 at half resolution); the better score
    wins, ties -> the smaller atomic patch index; rows x1 y1 x2 y2 score index in the order of the atomic patches"""
    gh, gw = best.shape
    win = {}
    for j in range(gh):
        for i in range(gw):
            if best[j, i] <= 0:
                continue
            x2 = dm.PATCH * i + 2 + int(cell[j, i, 1]) - c0
            y2 = dm.PATCH * j + 2 + int(cell[j, i, 0]) - c0
            if not (0 <= x2 < w2 and 0 <= y2 < h2):
                continue
            key = (y2 // dm.PATCH, x2 // dm.PATCH)
            cand = (float(best[j, i]), -(j * gw + i))
            if key not in win or cand > win[key][0]:
                win[key] = (cand, (j, i, x2, y2))
    out = []
    for (_, (j, i, x2, y2)) in sorted(win.values(), key=lambda t: -t[0][1]):
        out.append((2 * (dm.PATCH * i + 2), 2 * (dm.PATCH * j + 2), 2 * x2, 2 * y2, best[j, i], len(out)))
    return np.asarray(out, F).reshape(-1, 6)


def backtrack_on(maps, cs, h2, w2):
    """dm.backtrack + merge on the matcher's own maps: the rows Matcher.run must have returned, bit for bit"""
    best, cell = dm.backtrack(levels_from_maps(maps, cs))
    return merge(best, cell, cs[0], h2, w2)


def check_matches(got, maps, cs, h2, w2):
    want = backtrack_on(maps, cs, h2, w2)
    assert got.dtype == F and got.ndim == 2 and got.shape[1] == 6, (got.dtype, got.shape)
    if got.shape != want.shape or not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        n = min(len(got), len(want))
        diff = np.flatnonzero((got[:n].view(np.uint32) != want[:n].view(np.uint32)).any(1))
        k = int(diff[0]) if diff.size else n
        raise AssertionError("matches: %d rows, want %d; %d of the common rows differ; first at row %d: got %r, want %r"
                             % (len(got), len(want), diff.size, k, got[k].tolist() if k < len(got) else None,
                                want[k].tolist() if k < len(want) else None))
    return len(want)


# ---- stage 4: geometry -----------------------------------------------------------------------------------------------
def pyramid_geometry(h2, w2, r):
    """[(nh, nw, S, c)] per level: the loop of dm.pyramid on shapes alone (dm.children_of, dm.pool_geometry)"""
    geo = [(h2 // dm.PATCH, w2 // dm.PATCH, 2 * r + 1, r)]
    while True:
        gh, gw, S, c = geo[-1]
        nh, nw, kids = dm.children_of(len(geo) - 1, gh, gw)
        if kids is None:
            break
        _, S2, c2 = dm.pool_geometry(S, c)
        if S2 < 1:
            break
        geo.append((nh, nw, S2, c2))
        if S2 == 1:
            break
    return geo


def check_geometry(geo, h2, w2, ngh_rad):
    r = clamped_r(ngh_rad)
    assert geo[0][3] == r, "search radius %d, want %d (ngh_rad %d)" % (geo[0][3], r, ngh_rad)
    want = pyramid_geometry(h2, w2, r)
    assert list(geo) == want, "pyramid geometry %r, want %r" % (geo, want)


# ---- all of it -------------------------------------------------------------------------------------------------------
def chain(g, rows, ngh_rad, max_ulp):
    """every stage of matcher `g` (after a run that returned `rows`) against the stage before it.  All stages are
    checked even when an earlier one fails; returns (failures, stats): the assertion messages, and the figures worth
    printing (worst level-0 error in units of u * ref, largest ulp distance of the power, rows)."""
    failures, stats = [], {}
    d1, d2 = g.descriptors(0), g.descriptors(1)
    h2, w2 = d1.shape[:2]
    geo = g.levels()
    maps = [g.level_maps(k) for k in range(len(geo))]
    cs = [q[3] for q in geo]

    def stage(name, fn, *a):
        try:
            stats[name] = fn(*a)
        except AssertionError as e:
            failures.append("%s: %s" % (name, e))

    stage("geometry", check_geometry, geo, h2, w2, ngh_rad)
    stage("level0", check_level0, maps[0], d1, d2, cs[0])
    for l in range(1, len(maps)):
        stage("level%d" % l, check_level_up, maps[l], maps[l - 1], l - 1, cs[l - 1], max_ulp)
    stage("matches", check_matches, rows, maps, cs, h2, w2)
    return failures, stats


class OracleMatcher:
    """the oracle with the surface of match.Matcher, to run `chain` without a GPU"""

    def __init__(self, W, H, ngh_rad=100):
        self.W, self.H, self.r = int(W), int(H), clamped_r(ngh_rad)
        self.lv = None

    def pyramid(self, d1, d2):
        return dm.pyramid(d1, d2, self.r)

    def backtrack(self, levels):
        return dm.backtrack(levels)

    def merge(self, best, cell, c0, h2, w2):
        return merge(best, cell, c0, h2, w2)

    def run(self, a, b):
        self.d = [dm.descriptors(a), dm.descriptors(b)]
        self.lv = self.pyramid(*self.d)
        best, cell = self.backtrack(self.lv)
        return self.merge(best, cell, self.lv[0]["c"], *self.d[1].shape[:2])

    def descriptors(self, which):
        return self.d[which]

    def levels(self):
        return [l["maps"].shape[:3] + (l["c"],) for l in self.lv]

    def level_maps(self, k):
        return self.lv[k]["maps"]

    def close(self):
        pass
