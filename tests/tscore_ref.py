"""The numpy twins of ArapFlow_TrackScore and ArapFlow_ChainFlows (DESIGN.md "Track scoring"): float32 arithmetic operator
by operator, an integer table.  An fmaf is a float64 product and sum rounded once to float32, the way bg_ref.py does it:
the product of two float32 is exact in float64; the float64 sum is exact for the dyadic data most tests use and within a
double rounding of probability ~2^-29 per operation otherwise.  Test helper; no GPU."""
import numpy as np

F = np.float32
FRAMES_MAX, CLASSES, FIELDS = 64, 3, 16
CAP = 1 << 24                       # q of a capped point-frame: 4096 px in units of 2^-12
X = (1, 2, 4, 8, 16)                # the thresholds, in pixels
COUNT, GT_VIS, EST_VIS, AGREE, WITHIN, TP, SUM, MAX = 0, 1, 2, 3, 4, 9, 14, 15


def fma(a, b, c):
    with np.errstate(all="ignore"):
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def point_terms(gt_pos, est_pos, scale=(1, 1)):
    """(e2, q) of every point-frame, each operator one float32 operation"""
    g, s = np.asarray(gt_pos, F), np.asarray(est_pos, F)
    sx, sy = F(scale[0]), F(scale[1])
    with np.errstate(all="ignore"):
        dx, dy = (s[..., 0] - g[..., 0]) * sx, (s[..., 1] - g[..., 1]) * sy
        e2 = dx * dx + dy * dy
        e = np.sqrt(e2)
        ec = np.where(e <= F(4096), e, F(4096)).astype(F)
        q = (ec * F(4096) + F(0.5)).astype(np.uint32)           # truncation
    assert e2.dtype == e.dtype == F
    return e2, q


def track_score_ref(gt_pos, gt_occ, est_pos, est_occ, scale=(1, 1)):
    """opt.track_score's twin: gt_pos, est_pos f32[F,P,2]; gt_occ, est_occ u8[F,P] -> u64[F,3,16]"""
    gt_occ, est_occ = np.asarray(gt_occ, np.uint8), np.asarray(est_occ, np.uint8)
    nf = gt_occ.shape[0]
    e2, q = point_terms(gt_pos, est_pos, scale)
    valid = gt_occ[0] == 0
    gv, ev = gt_occ == 0, est_occ == 0
    table = np.zeros((nf, CLASSES, FIELDS), np.uint64)
    table[0, 0, 0], table[0, 0, 1] = valid.sum(), (~valid).sum()
    hb = np.zeros(valid.shape, bool)                          # hidden in one of the frames 1 .. f-1
    for f in range(1, nf):
        with np.errstate(invalid="ignore"):
            inx = [gv[f] & (e2[f] < F(x * x)) for x in X]
        for c, m in enumerate((valid, valid & gv[f] & ~hb, valid & gv[f] & hb)):
            qm = np.where(m & gv[f], q[f], 0).astype(np.uint64)
            row = [m.sum(), (m & gv[f]).sum(), (m & ev[f]).sum(), (m & (gv[f] == ev[f])).sum()]
            row += [(m & i).sum() for i in inx] + [(m & i & ev[f]).sum() for i in inx] + [qm.sum(), qm.max()]
            table[f, c] = np.array([int(v) for v in row], np.uint64)
        hb |= ~gv[f]
    return table


def in_frame(p, W, H):
    with np.errstate(invalid="ignore"):
        return (p[..., 0] >= 0) & (p[..., 0] <= F(W - 1)) & (p[..., 1] >= 0) & (p[..., 1] <= F(H - 1))


def sample(A, a):
    """S(A, a) at the points a f32[P,2] inside the frame of A f32[H,W,2] -> f32[P,2]"""
    H, W = A.shape[:2]
    x0, y0 = np.floor(a[:, 0]).astype(np.int64), np.floor(a[:, 1]).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    fx, fy = (a[:, 0] - x0.astype(F))[:, None], (a[:, 1] - y0.astype(F))[:, None]
    assert fx.dtype == F
    with np.errstate(all="ignore"):
        c00, c01, c10, c11 = A[y0, x0], A[y0, x1], A[y1, x0], A[y1, x1]
        top, bot = fma(fx, c01 - c00, c00), fma(fx, c11 - c10, c10)
        return fma(fy, bot - top, top)


def chain_ref(flows, points, bwd=None):
    """opt.chain_flows' twin: flows f32[L,H,W,2], bwd the same or None, points f32[P,2] -> (pos f32[L+1,P,2], occ u8[L+1,P])"""
    flows, p = np.asarray(flows, F), np.asarray(points, F).copy()
    L, H, W = flows.shape[:3]
    pos, occ = np.zeros((L + 1,) + p.shape, F), np.zeros((L + 1, p.shape[0]), np.uint8)
    lost = ~in_frame(p, W, H)
    pos[0], occ[0] = p, np.where(lost, 255, 0)
    for j in range(L):
        live = np.nonzero(~lost)[0]
        o = np.full(p.shape[0], 255, np.uint8)
        with np.errstate(all="ignore"):
            f = sample(flows[j], p[live])
            b = p[live] + f
            p[live] = b
            inside = in_frame(b, W, H)
            lost[live[~inside]] = True
            o[live[inside]] = 0
            if bwd is not None and inside.any():
                fi, bi = f[inside], b[inside]
                g = sample(np.asarray(bwd, F)[j], bi)
                s = fi + g
                d2 = s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]
                m2 = (fi[:, 0] * fi[:, 0] + fi[:, 1] * fi[:, 1]) + (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1])
                assert d2.dtype == m2.dtype == F
                o[live[inside]] = np.where(~(d2 <= fma(F(0.01), m2, F(0.5))), 255, 0)
        pos[j + 1], occ[j + 1] = p, o
    return pos, occ


def ulp(x, k):
    """the float32 k steps from x in the order of the positive bit patterns"""
    return (np.asarray(x, F).view(np.uint32) + np.uint32(k) if k >= 0 else np.asarray(x, F).view(np.uint32) - np.uint32(-k)).view(F)


def threshold_offsets(x, scale, seed=11):
    """two offsets (est - gt) f32[2] under `scale`: one whose e2 is exactly x * x, one whose e2 is one ulp below it; found by
    a seeded search on the circle of radius x, with the twin's own arithmetic"""
    rng = np.random.default_rng(seed + x)
    sx, sy = F(scale[0]), F(scale[1])
    want = (F(x * x), ulp(F(x * x), -1))
    found = [None, None]
    while found[0] is None or found[1] is None:
        ang = rng.uniform(0.1, 1.4, 100000)
        d = np.stack([(F(x) * np.cos(ang).astype(F)) / sx, (F(x) * np.sin(ang).astype(F)) / sy], -1).astype(F)
        for k in (-1, 0, 1):
            dk = np.stack([d[:, 0], ulp(d[:, 1], k) if k else d[:, 1]], -1)
            e2, _ = point_terms(np.zeros_like(dk), dk, scale)
            for w in range(2):
                hit = np.nonzero(e2 == want[w])[0]
                if found[w] is None and hit.size:
                    found[w] = dk[hit[0]]
    return found


TAPVID_854x480 = (F(256) / F(854), F(256) / F(480))          # a non-dyadic scale: the benchmark's raster of an 854 x 480 frame


def crafted_case(scale=(1, 1)):
    """(gt_pos, gt_occ, est_pos, est_occ), F = 4: for every threshold x a point-frame with e2 exactly x * x and one an ulp
    below, among the tracked and among the reappeared; NaN and inf estimates; every gv / ev combination in both classes;
    hidden-then-visible ground truth; invalid queries (with NaN positions) -- every field of every class is non-zero"""
    nf = 4
    rows = []                                                   # (offset f32[2], gt_occ[4], est_occ[4])
    vis, hid = 0, 255
    for x in X:
        for d in threshold_offsets(x, scale):
            rows.append((d, (vis, vis, vis, vis), (vis, vis, vis, vis)))          # tracked
            rows.append((d, (vis, hid, vis, vis), (vis, vis, vis, hid)))          # reappeared in frames 2 and 3
            rows.append((d, (vis, vis, vis, vis), (vis, hid, 7, vis)))            # tracked, the estimate hidden
    for bad in ((np.nan, 0), (np.inf, 3), (-np.inf, np.nan), (1e30, 0)):
        rows.append((np.array(bad, F), (vis, vis, hid, vis), (vis, vis, vis, vis)))
        rows.append((np.array(bad, F), (vis, 1, vis, vis), (vis, vis, hid, vis)))
    for g1 in (vis, hid):                                       # every gv / ev combination, before and after a hidden frame
        for g in (vis, 3):
            for e in (vis, 200):
                rows.append((np.array([0.25, -0.5], F), (vis, g1, g, g), (vis, e, e, e)))
    rows.append((np.array([0.5, 0.5], F), (hid, vis, vis, vis), (vis, vis, vis, vis)))          # invalid queries
    rows.append((np.array([np.nan, np.nan], F), (1, hid, vis, hid), (hid, hid, vis, vis)))
    P = len(rows)
    rng = np.random.default_rng(3)
    gt_pos = np.zeros((nf, P, 2), F)
    gt_pos[:, -1] = np.nan                                      # (the last invalid query has no position at all)
    est_pos = np.stack([np.stack([gt_pos[f, k] + r[0] for k, r in enumerate(rows)]) for f in range(nf)]).astype(F)
    est_pos[0] = rng.uniform(-5, 5, (P, 2)).astype(F)           # frame 0 of the estimate is never read into a count
    gt_occ = np.array([r[1] for r in rows], np.uint8).T.copy()
    est_occ = np.array([r[2] for r in rows], np.uint8).T.copy()
    return gt_pos, gt_occ, est_pos, est_occ


def random_case(nf, P, seed, invalid=0.1, hidden=0.2):
    """a random track pair: errors spread over all thresholds, some far beyond the cap, some non-finite"""
    rng = np.random.default_rng(seed)
    gt_pos = rng.uniform(0, 100, (nf, P, 2)).astype(F)
    mag = (F(2) ** rng.uniform(-3, 6, (nf, P, 1))).astype(F)
    est_pos = (gt_pos + mag * rng.standard_normal((nf, P, 2)).astype(F)).astype(F)
    wild = rng.random((nf, P)) < 0.02
    est_pos[wild] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e9], F), (int(wild.sum()), 2))
    gt_occ = np.where(rng.random((nf, P)) < hidden, 255, 0).astype(np.uint8)
    gt_occ[0] = np.where(rng.random(P) < invalid, 255, 0)
    est_occ = np.where(rng.random((nf, P)) < hidden, rng.integers(1, 256, (nf, P)), 0).astype(np.uint8)
    return gt_pos, gt_occ, est_pos, est_occ
