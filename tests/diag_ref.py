"""Fold diagnostics (DESIGN.md "Fold diagnostics"), restated twice: `diag`, vectorised float32 numpy -- the twin the GPU
must equal bit for bit -- and `diag_sequential`, the definitions read out one vertex and one triangle at a time in
plain Python, for tiny grids.  Both take the mask's red channel u8[H,W] (0 = object) and the vertex positions
P f32[H,W,2]; `flow_pos` makes the positions of a flow.  No tolerance anywhere: counts, flags and extrema in the total
order of the IEEE bit patterns (-0 < +0)."""
import numpy as np

KEYS = ("vertices", "outside", "triangles", "folded", "nonfinite", "det_min", "det_max", "disp2_max")
FLOAT_KEYS = KEYS[5:]
F32 = np.float32


def grid_field(W, H):
    ys, xs = np.mgrid[0:H, 0:W]
    return np.stack([xs, ys], -1).astype(F32)


def flow_pos(flow):
    """P = ((float)x + flow.x, (float)y + flow.y), one float32 addition per coordinate"""
    flow = np.asarray(flow, F32)
    H, W = flow.shape[:2]
    with np.errstate(all="ignore"):
        return grid_field(W, H) + flow


def order_key(a):
    """float32 -> uint32, monotone in the total order of the bit patterns"""
    u = np.ascontiguousarray(a, F32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def _extreme(values, largest, none):
    values = np.asarray(values, F32).reshape(-1)
    if values.size == 0:
        return F32(none)
    k = order_key(values)
    return values[np.argmax(k) if largest else np.argmin(k)]


def _det(p0, p1, p2):
    e1x, e1y = p1[..., 0] - p0[..., 0], p1[..., 1] - p0[..., 1]
    e2x, e2y = p2[..., 0] - p0[..., 0], p2[..., 1] - p0[..., 1]
    return (e1x * e2y) - (e1y * e2x)


def diag(mask_red, P):
    """-> (stats: {key: int or np.float32} over KEYS, fold u8[H,W])"""
    mask_red, P = np.asarray(mask_red), np.ascontiguousarray(P, F32)
    H, W = mask_red.shape
    assert P.shape == (H, W, 2) and P.dtype == F32
    obj = mask_red == 0
    grid = grid_field(W, H)
    with np.errstate(all="ignore"):
        on = obj[:-1, :-1] & obj[:-1, 1:] & obj[1:, :-1] & obj[1:, 1:]
        p00, p01, p10, p11 = P[:-1, :-1], P[:-1, 1:], P[1:, :-1], P[1:, 1:]
        det = np.stack([_det(p00, p01, p10), _det(p10, p01, p11)])          # triangles 2u, 2u + 1
        assert det.dtype == F32
        on2 = np.stack([on, on])
        fin = on2 & np.isfinite(det)
        folded = fin & (det <= 0)
        bad = on2 & ~(np.isfinite(det) & (det > 0))
        inside = (P[..., 0] >= 0) & (P[..., 0] <= F32(W - 1)) & (P[..., 1] >= 0) & (P[..., 1] <= F32(H - 1))
        both = obj & np.isfinite(P[..., 0]) & np.isfinite(P[..., 1])
        d = P - grid
        disp2 = (d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])
        assert disp2.dtype == F32
    stats = dict(vertices=int(obj.sum()), outside=int((obj & ~inside).sum()), triangles=int(on2.sum()),
                 folded=int(folded.sum()), nonfinite=int((on2 & ~fin).sum()),
                 det_min=_extreme(det[fin], False, np.inf), det_max=_extreme(det[fin], True, -np.inf),
                 disp2_max=_extreme(disp2[both], True, 0.0))
    fold = np.zeros((H, W), bool)
    fold[:-1, :-1] |= bad[0]                    # p00: triangle 2u
    fold[:-1, 1:] |= bad[0] | bad[1]            # p01: both
    fold[1:, :-1] |= bad[0] | bad[1]            # p10: both
    fold[1:, 1:] |= bad[1]                      # p11: triangle 2u + 1
    return stats, np.where(fold & obj, 255, 0).astype(np.uint8)


def diag_sequential(mask_red, P):
    """the definitions, one at a time (tiny grids)"""
    import math
    import struct
    mask_red, P = np.asarray(mask_red), np.asarray(P, F32)
    H, W = mask_red.shape
    bits = lambda v: struct.unpack("<I", struct.pack("<f", float(v)))[0]
    key = lambda v: (bits(v) ^ 0xffffffff) if bits(v) >> 31 else (bits(v) | 0x80000000)
    st = dict(vertices=0, outside=0, triangles=0, folded=0, nonfinite=0)
    dets, disps = [], []
    fold = np.zeros((H, W), np.uint8)
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                if mask_red[y, x] != 0:
                    continue
                st["vertices"] += 1
                px, py = P[y, x]
                if not (px >= 0 and px <= F32(W - 1) and py >= 0 and py <= F32(H - 1)):
                    st["outside"] += 1
                if math.isfinite(px) and math.isfinite(py):
                    dx, dy = F32(px - F32(x)), F32(py - F32(y))
                    disps.append(F32(F32(dx * dx) + F32(dy * dy)))
        for y in range(H - 1):
            for x in range(W - 1):
                c = [(x, y), (x + 1, y), (x, y + 1), (x + 1, y + 1)]                # p00 p01 p10 p11
                if any(mask_red[b, a] != 0 for a, b in c):
                    continue
                for tri in ((c[0], c[1], c[2]), (c[2], c[1], c[3])):
                    p0, p1, p2 = (P[b, a] for a, b in tri)
                    e1x, e1y = F32(p1[0] - p0[0]), F32(p1[1] - p0[1])
                    e2x, e2y = F32(p2[0] - p0[0]), F32(p2[1] - p0[1])
                    det = F32(F32(e1x * e2y) - F32(e1y * e2x))
                    st["triangles"] += 1
                    if not math.isfinite(det):
                        st["nonfinite"] += 1
                    elif det <= 0:
                        st["folded"] += 1
                    if math.isfinite(det):
                        dets.append(det)
                    if not math.isfinite(det) or det <= 0:
                        for a, b in tri:
                            fold[b, a] = 255
    st["det_min"] = min(dets, key=key) if dets else F32(np.inf)
    st["det_max"] = max(dets, key=key) if dets else F32(-np.inf)
    st["disp2_max"] = max(disps, key=key) if disps else F32(0)
    return st, fold


def stats_bytes(stats):
    """the struct's bytes without `reserved`: equal bytes = equal bit for bit (NaN-proof, -0 != +0)"""
    return b"".join(np.asarray(stats[k], F32 if k in FLOAT_KEYS else np.uint32).tobytes() for k in KEYS)


def same(a, b):
    """two (stats, fold) results, bit for bit"""
    return stats_bytes(a[0]) == stats_bytes(b[0]) and np.array_equal(a[1], b[1])


# ---- the cases both test files use -----------------------------------------------------------------------------------
W0, H0 = 67, 9            # W no multiple of 64, H no multiple of 4, 2 x 3 blocks of (64, 4)


def masks(W=W0, H=H0):
    """all object; a 30 % random background; a one-pixel-wide strip of object (vertices, no triangle); all background"""
    rnd = np.where(np.random.default_rng(3).random((H, W)) < 0.3, 255, 0).astype(np.uint8)
    strip = np.full((H, W), 255, np.uint8)
    strip[H // 2, :] = 0
    return dict(all=np.zeros((H, W), np.uint8), random=rnd, strip=strip, none=np.full((H, W), 255, np.uint8))


def fields(W=W0, H=H0):
    """{name: flow f32[H,W,2]}: the flows of the issue's list; every position is grid + flow (flow_pos)"""
    g = grid_field(W, H)
    z = np.zeros((H, W, 2), F32)
    out = dict(zero=z)
    mirror = z.copy()
    mirror[..., 0] = F32(W - 1) - 2 * g[..., 0]                            # x -> (W - 1) - x, exact
    out["mirror"] = mirror
    shift = z.copy()
    shift[..., 0], shift[..., 1] = 3, -2
    out["translation"] = shift
    out["noise_a"] = np.random.default_rng(7).normal(0, 0.35, (H, W, 2)).astype(F32)
    out["noise_b"] = np.random.default_rng(3).normal(0, 0.5, (H, W, 2)).astype(F32)
    bad = out["noise_a"].copy()
    bad[H // 2, W // 3, 0] = np.nan
    bad[2, 2 * W // 3, 1] = np.inf
    out["nan_inf"] = bad
    for x, y in spikes(W, H):
        s = z.copy()
        s[y, x] = (-1.5, -1.25) if x > 0 else (1.5, 1.25)                  # across its neighbours: folds triangles at it
        out["spike_%d_%d" % (x, y)] = s
    return out


def spikes(W=W0, H=H0):
    """single displaced vertices: first lane of the first block, last lane of its last wave, first lane of a block
    diagonally next to it, and one inside the last partial block"""
    return [(0, 0), (63, 3), (64, 4), (W - 2, H - 2)]


def translation_outside(W, H, dx, dy):
    """object vertices an all-object W x H grid moves out of the frame under the integer translation (dx, dy)"""
    inx, iny = max(0, W - abs(dx)), max(0, H - abs(dy))
    return W * H - inx * iny
