"""The numpy twin of ArapFlow_LabelScore and ArapFlow_MapScore (DESIGN.md "Map scoring"): counts by boolean sums, bmap by
shifted arrays, hits by an explicit squared-distance minimum over the other set's pixels, the same file text; beside it
the definitions once more as plain loops over pixels.  Test helper; no GPU."""
import numpy as np

from arap_flow_amd import pipeline

U64 = np.uint64


def _maps(gt, est, skip):
    gt, est = np.asarray(gt, np.uint8), np.asarray(est, np.uint8)
    if gt.ndim == 2:
        gt, est = gt[None], est[None]
    assert gt.ndim == 3 and gt.shape == est.shape
    skip = np.zeros(gt.shape, bool) if skip is None else np.asarray(skip).reshape(gt.shape) != 0
    return gt, est, skip


def bmap(m):
    """the DAVIS toolkit's seg2bmap at equal size, of a boolean map [..., H, W]: a pixel differs from its right, lower or
    lower-right neighbour; the last row looks right only, the last column down only, the last pixel is 0"""
    m = np.asarray(m, bool)
    b = np.zeros(m.shape, bool)
    b[..., :, :-1] |= m[..., :, :-1] != m[..., :, 1:]
    b[..., :-1, :] |= m[..., :-1, :] != m[..., 1:, :]
    b[..., :-1, :-1] |= m[..., :-1, :-1] != m[..., 1:, 1:]
    return b


def hits(A, B, radius):
    """the pixels of A with a pixel of B within `radius`: the squared distance to every pixel of B, its minimum"""
    pa, pb = np.argwhere(A).astype(np.int64), np.argwhere(B).astype(np.int64)
    if len(pa) == 0 or len(pb) == 0:
        return 0
    count = 0
    for lo in range(0, len(pa), 512):
        d = pa[lo:lo + 512, None, :] - pb[None, :, :]
        count += int(((d * d).sum(axis=2).min(axis=1) <= radius * radius).sum())
    return count


def match(A, B, skip, radius):
    """(a, b, a_hit, b_hit) of the boundary match of two boolean sets under a boolean skip plane"""
    A, B = A & ~skip, B & ~skip
    return [int(A.sum()), int(B.sum()), hits(A, B, radius), hits(B, A, radius)]


def label_ref(gt, est, L, radius, skip=None):
    """opt.label_score's twin -> {"table": u64[n,L+1,8]}"""
    gt, est, skip = _maps(gt, est, skip)
    table = np.zeros((len(gt), L + 1, 8), U64)
    for i, (g, e, s) in enumerate(zip(gt, est, skip)):
        c = ~s
        table[i, 0, :5] = [c.sum(), s.sum(), (c & (g == e)).sum(), (c & (g > L)).sum(), (c & (e > L)).sum()]
        for k in range(1, L + 1):
            table[i, k, :3] = [(c & (g == k)).sum(), (c & (e == k)).sum(), (c & (g == k) & (e == k)).sum()]
            table[i, k, 3:7] = match(bmap(g == k), bmap(e == k), s, radius)
    return {"table": table}


def map_ref(gt, est, skip=None, thr=(), radius=0):
    """opt.map_score's twin -> {"hist": u64[n,2,256], "match": u64[n,m,4]}"""
    gt, est, skip = _maps(gt, est, skip)
    hist, mt = np.zeros((len(gt), 2, 256), U64), np.zeros((len(gt), len(thr), 4), U64)
    for i, (g, e, s) in enumerate(zip(gt, est, skip)):
        for c in (0, 1):
            hist[i, c] = np.bincount(e[~s & ((g != 0) == bool(c))], minlength=256)
        for j, t in enumerate(thr):
            mt[i, j] = match(g != 0, e >= t, s, radius)
    return {"hist": hist, "match": mt}


def label_text(gt, est, L, radius, skip=None):
    """the file an `lscore` line writes for one map"""
    return pipeline.format_label_score(label_ref(gt, est, L, radius, skip)["table"][0])


def map_text(gt, est, skip=None, thr=(), radius=0):
    """the file an `mscore` line writes for one map"""
    r = map_ref(gt, est, skip, thr, radius)
    return pipeline.format_map_score(dict(hist=r["hist"][0], thr=tuple(thr), match=r["match"][0]))


# ---- the definitions as plain loops ----------------------------------------------------------------------------------------
def bmap_loops(m):
    H, W = len(m), len(m[0])
    b = [[False] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            if x < W - 1 and y < H - 1:
                b[y][x] = m[y][x] != m[y][x + 1] or m[y][x] != m[y + 1][x] or m[y][x] != m[y + 1][x + 1]
            elif x < W - 1:
                b[y][x] = m[y][x] != m[y][x + 1]
            elif y < H - 1:
                b[y][x] = m[y][x] != m[y + 1][x]
    return b


def match_loops(A, B, skip, radius):
    H, W = len(A), len(A[0])
    pa = [(x, y) for y in range(H) for x in range(W) if A[y][x] and not skip[y][x]]
    pb = [(x, y) for y in range(H) for x in range(W) if B[y][x] and not skip[y][x]]
    near = lambda p, qs: any((p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2 <= radius * radius for q in qs)
    return [len(pa), len(pb), sum(near(p, pb) for p in pa), sum(near(q, pa) for q in pb)]


def label_loops(gt, est, L, radius, skip=None):
    """one map [H,W] -> the table as nested lists [L+1][8]"""
    gt, est = np.asarray(gt).tolist(), np.asarray(est).tolist()
    H, W = len(gt), len(gt[0])
    skip = [[False] * W for _ in range(H)] if skip is None else (np.asarray(skip) != 0).tolist()
    t = [[0] * 8 for _ in range(L + 1)]
    for y in range(H):
        for x in range(W):
            g, e = gt[y][x], est[y][x]
            if skip[y][x]:
                t[0][1] += 1
                continue
            t[0][0] += 1
            t[0][2] += g == e
            t[0][3] += g > L
            t[0][4] += e > L
            if 1 <= g <= L:
                t[g][0] += 1
            if 1 <= e <= L:
                t[e][1] += 1
            if 1 <= g <= L and g == e:
                t[g][2] += 1
    for k in range(1, L + 1):
        A = bmap_loops([[v == k for v in row] for row in gt])
        B = bmap_loops([[v == k for v in row] for row in est])
        t[k][3:7] = match_loops(A, B, skip, radius)
    return t


def map_loops(gt, est, skip=None, thr=(), radius=0):
    """one map [H,W] -> (hist [2][256], match [m][4]) as nested lists"""
    gt, est = np.asarray(gt).tolist(), np.asarray(est).tolist()
    H, W = len(gt), len(gt[0])
    skip = [[False] * W for _ in range(H)] if skip is None else (np.asarray(skip) != 0).tolist()
    hist = [[0] * 256 for _ in range(2)]
    for y in range(H):
        for x in range(W):
            if not skip[y][x]:
                hist[int(gt[y][x] != 0)][est[y][x]] += 1
    mt = [match_loops([[v != 0 for v in row] for row in gt], [[v >= t for v in row] for row in est], skip, radius) for t in thr]
    return hist, mt
