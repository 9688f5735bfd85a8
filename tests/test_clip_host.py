"""CPU-only: training clips (DESIGN.md "Training clips") around the kernels.  The numpy twin tests/clip_ref.py against
tests/aug_ref.py byte for byte where a clip is a pair, against numpy slicing and closed forms on the consequences the
definition names, on a crafted case that shows every reason for a hidden point, on the rounding edge of `erased`, on used
and unused bad taps and the guard of a from-first link; the flow of a link and the tracks of its two frames against each
other within a bound derived here; ArapFlow_ClipTables (host only) through ctypes."""
import ctypes as C

import numpy as np
import pytest

import aug_cases
import aug_ref
import clip_ref
from aug_cases import AFFINE_G, AFFINE_g, EPS, SECOND_ORDER

F = np.float32
D = np.float64
ID = (1, 0, 0, 0, 1, 0)


def frame(T=ID, gain=(1, 1, 1), gamma=1.0, erase=(), fill=(0, 0, 0)):
    from arap_flow_amd import opt
    return opt.ClipFrame(T, gain, gamma, erase, fill)


def clip(W, H, T, L, P, seed=0, B=1):
    """frames of random bytes, flows on the 2^-6 lattice with a few NaN / inf / 1e9 pixels, a random skip, points around
    the source and a random hidden flag"""
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (B, T, H, W, 3)).astype(np.uint8)
    flows = (rng.integers(-640, 641, (B, L, H, W, 2)) / 64.0).astype(F)
    for k, v in enumerate((np.nan, np.inf, -np.inf, 1e9)):
        flows[:, :, (k * 3 + 1) % H, (k * 5 + 2) % W, k % 2] = v
    skip = np.where(rng.random((B, L, H, W)) < 0.1, rng.integers(1, 256, (B, L, H, W)), 0).astype(np.uint8)
    pos = (np.stack([rng.integers(-64, 64 * (W + 1), (B, T, P)), rng.integers(-64, 64 * (H + 1), (B, T, P))], -1) / 64.0).astype(F)
    occ = np.where(rng.random((B, T, P)) < 0.2, 255, 0).astype(np.uint8)
    return frames, flows, skip, pos, occ


def planar(a):
    return np.moveaxis(a, -1, -3).astype(F)


def bad_of(flow, skip):
    return (skip != 0) | ~np.isfinite(flow).all(-1)


def in_crop(p, w, h):
    from arap_flow_amd import trk
    return trk.in_frame(p, w, h)


# ---- a clip of two frames and one link is a pair ---------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(48, 8), (65, 9), (3, 2)], ids=lambda s: "%dx%d" % s)
def test_pair_equivalence(size):
    """T = 2, L = 1, links = (0, 1), no rectangle on frame 0: video[:,0], video[:,1], flows[:,0], valid[:,0] are
    aug_ref.augment's img1, img2, flow, valid byte for byte, at every transform of tests/aug_cases.py"""
    W, H = 70, 9
    w, h = size
    ts = aug_cases.transforms(W, H, w, h)
    frames, flows, skips, _, _ = clip(W, H, 2, 1, 1, seed=5, B=len(ts))
    rgb1, rgb2, flow, skip = frames[:, 0], frames[:, 1], flows[:, 0], skips[:, 0]
    scale, bias = (1 / 58.395, 1 / 57.12, 1 / 57.375), (-2.1179, -2.0357, -1.8044)
    want = aug_ref.augment(rgb1, rgb2, flow, ts, (w, h), skip=skip, scale=scale, bias=bias, tau=1.0)
    samples = [[frame(s.T1, s.gain1, s.gamma1, (), s.fill), frame(s.T2, s.gain2, s.gamma2, s.erase, s.fill)] for s in ts]
    got = clip_ref.augment(frames, samples, (w, h), links=[(0, 1)], flows=flows, skip=skips,
                           scale=scale, bias=bias, tau=1.0)
    assert got["video"][:, 0].tobytes() == want["img1"].tobytes() and got["video"][:, 1].tobytes() == want["img2"].tobytes()
    assert got["flows"][:, 0].tobytes() == want["flow"].tobytes() and got["valid"][:, 0].tobytes() == want["valid"].tobytes()


# ---- the consequences of the definition, against numpy slicing and closed forms ----------------------------------------------
def test_identity_maps():
    W, H, T, P = 70, 9, 3, 200
    frames, flows, skip, pos, occ = clip(W, H, T, 2, P, seed=1, B=2)
    r = clip_ref.augment(frames, [[frame()] * T] * 2, (W, H), links=[(0, 1), (0, 2)], flows=flows, skip=skip, pos=pos, occ=occ)
    assert np.array_equal(r["video"], planar(frames))
    assert np.array_equal(r["tracks"], pos)
    want = (occ == 0) & in_crop(pos, W, H)
    assert np.array_equal(r["vis"], np.where(want, 255, 0)) and 0.2 < want.mean() < 0.9
    # from-first links under identity maps return their input flow wherever it is valid
    bad = bad_of(flows, skip)
    assert np.array_equal(r["valid"], np.where(bad, 0, 255))
    assert np.array_equal(r["flows"], np.where(bad[:, :, None], F(0), planar(flows)))


def test_integer_translation():
    W, H, w, h, T, P = 70, 9, 48, 5, 3, 200
    shifts = [(13, 3), (0, 0), (22, 4)]
    frames, flows, skip, pos, occ = clip(W, H, T, 1, P, seed=2)
    samples = [[frame((1, 0, sx, 0, 1, sy)) for sx, sy in shifts]]
    r = clip_ref.augment(frames, samples, (w, h), pos=pos, occ=occ)
    for t, (sx, sy) in enumerate(shifts):
        assert np.array_equal(r["video"][0, t], planar(frames[0, t, sy:sy + h, sx:sx + w]))
        assert np.array_equal(r["tracks"][0, t], pos[0, t] - np.asarray([sx, sy], F))
        want = (occ[0, t] == 0) & in_crop(pos[0, t] - np.asarray([sx, sy], F), w, h)
        assert np.array_equal(r["vis"][0, t], np.where(want, 255, 0))


def test_mirror_and_zoom_maps():
    W, H, P = 70, 9, 200
    frames, _, _, pos, occ = clip(W, H, 2, 0, P, seed=3)
    r = clip_ref.augment(None, [[frame((-1, 0, W - 1, 0, 1, 0)), frame((2, 0, 0, 0, 2, 0))]], (W, H), pos=pos, occ=occ)
    assert np.array_equal(r["tracks"][0, 0, :, 0], F(W - 1) - pos[0, 0, :, 0]) and np.array_equal(r["tracks"][0, 0, :, 1], pos[0, 0, :, 1])
    assert np.array_equal(r["tracks"][0, 1], F(0.5) * pos[0, 1])
    assert np.array_equal(r["vis"][0, 1], np.where((occ[0, 1] == 0) & in_crop(F(0.5) * pos[0, 1], W, H), 255, 0))


def test_from_first_link_under_a_translated_target():
    """a link (0, j) with T_j a translation by (2, 1) returns flow - (2, 1)"""
    W, H = 70, 9
    frames, flows, skip, _, _ = clip(W, H, 3, 2, 1, seed=4)
    samples = [[frame(), frame((1, 0, 5, 0, 1, 3)), frame((1, 0, 2, 0, 1, 1))]]
    r = clip_ref.augment(None, samples, (W, H), links=[(0, 2), (0, 1)], flows=flows, skip=skip)
    bad = bad_of(flows, skip)
    assert np.array_equal(r["valid"], np.where(bad, 0, 255))
    for l, shift in enumerate(((2, 1), (5, 3))):
        want = planar(flows[0, l]) - np.asarray(shift, F)[:, None, None]
        assert np.array_equal(r["flows"][0, l], np.where(bad[0, l][None], F(0), want))


# ---- every reason for a hidden point --------------------------------------------------------------------------------------
def crafted():
    """70x9 -> 48x8, T = 3, P = 96: a rotation with scale, the same with a relative motion, a translation; points spread
    a fifth of the crop beyond each of its sides, three that overflow; rectangles on every frame"""
    W, H, w, h, T, P = 70, 9, 48, 8, 3, 96
    s = aug_cases.transforms(W, H, w, h)[5]
    maps = [s.T1, s.T2, (1, 0, 11, 0, 1, 1)]
    rng = np.random.default_rng(7)
    o = rng.uniform(-0.2, 1.2, (T, P, 2)) * [w - 1, h - 1]
    pos = np.empty((T, P, 2), F)
    for t, M in enumerate(maps):
        A = np.asarray(M, D).reshape(2, 3)
        pos[t] = (o[t] @ A[:, :2].T + A[:, 2]).astype(F)
    pos[0, 5], pos[1, 6], pos[2, 7] = (np.nan, 3), (np.inf, 1), (3e38, -3e38)
    occ = np.where(rng.random((T, P)) < 0.15, 255, 0).astype(np.uint8)
    rects = [((10, 1, 22, 6),), ((0, 0, 6, 8), (30, 2, 40, 5)), ((20, 0, 30, 8), (-5, -5, 3, 3), (40, 6, 60, 20), (44, 0, 48, 2))]
    samples = [[frame(M, (1.1, 0.9, 1.0), 0.9, rects[t], (0.25, 0.5, 0.75)) for t, M in enumerate(maps)]]
    frames, flows, skip, _, _ = clip(W, H, T, 2, 1, seed=8)
    return dict(frames=frames, samples=samples, size=(w, h), links=[(0, 1), (1, 2)], flows=flows, skip=skip, pos=pos[None], occ=occ[None])


def test_crafted_case_shows_every_reason_for_a_hidden_point():
    c = crafted()
    r = clip_ref.augment(c["frames"], c["samples"], c["size"], links=c["links"], flows=c["flows"], skip=c["skip"], pos=c["pos"],
                         occ=c["occ"], reasons=True)
    why = r["reasons"][0]
    for k in ("occ", "left", "right", "above", "below", "erased", "nonfinite"):
        assert any(f[k].any() for f in why), k
    vis = r["vis"] != 0
    assert 0.3 <= vis.mean() <= 0.7, vis.mean()
    assert any((f["erased"] & ~f["occ"]).any() for f in why)                  # a point only a rectangle hides
    # a hidden point keeps its position; a non-finite one is (0, 0)
    assert np.isfinite(r["tracks"]).all()
    assert all((r["tracks"][0, t][f["nonfinite"]] == 0).all() for t, f in enumerate(why))
    hidden_in = ~vis[0, 0] & ~why[0]["nonfinite"]
    P0 = clip_ref.tables(c["samples"][0][0])[0]
    with np.errstate(all="ignore"):
        ox, oy = aug_ref.apply(P0, c["pos"][0, 0, :, 0], c["pos"][0, 0, :, 1])
    assert hidden_in.any() and np.array_equal(r["tracks"][0, 0][hidden_in], np.stack([ox, oy], -1)[hidden_in])


def test_rounding_edge_of_erased():
    """rx = (int)floorf(o.x + 0.5f) in float32.  A point at k + 0.5 belongs to pixel k + 1, the float32 just below to
    pixel k -- but for k = 0, where 0.5 - 2^-25 + 0.5 is a tie that rounds to 1.0, to pixel 1 as well"""
    w, h = 32, 4
    ks = np.asarray([0, 1, 3, 7, 16])
    at = (ks + 0.5).astype(F)
    below = np.nextafter(at, F(0))
    assert (below < at).all()
    pos = np.stack([np.concatenate([at, below]), np.full(10, 1.0, F)], -1)[None, None]
    occ = np.zeros((1, 1, 10), np.uint8)
    for n, k in enumerate(ks):
        left = clip_ref.augment(None, [[frame(erase=((int(k) + 1, 0, int(k) + 3, h),))]], (w, h), pos=pos, occ=occ)["vis"][0, 0]
        right = clip_ref.augment(None, [[frame(erase=((int(k) - 2, 0, int(k) + 1, h),))]], (w, h), pos=pos, occ=occ)["vis"][0, 0]
        tie = k == 0
        assert left[n] == 0 and left[5 + n] == (0 if tie else 255), k             # the rectangle begins at pixel k + 1
        assert right[n] == 255 and right[5 + n] == (255 if tie else 0), k         # the rectangle ends with pixel k
    # in y alike
    posy = pos[..., ::-1].copy()
    up = clip_ref.augment(None, [[frame(erase=((0, 2, w, 4),))]], (w, 40), pos=posy, occ=occ)["vis"][0, 0]
    assert up[1] == 0 and up[6] == 255


# ---- bad taps and the guard, on a from-first link -----------------------------------------------------------------------------
def test_bad_taps_and_the_guard_on_a_from_first_link():
    W, H = 8, 4
    flow = np.zeros((1, 1, H, W, 2), F)
    flow[0, 0, :, 4:, 0] = 2.0                                   # a step of 2 between columns 3 and 4
    samples = [[frame((1, 0, 0.5, 0, 1, 0)), frame(), frame((1, 0, 1, 0, 1, 0))]]          # frame 0: fx = 0.5, fy = 0
    run = lambda fl, tau, skip=None: clip_ref.augment(None, samples, (W - 1, H), links=[(0, 2)], flows=fl, skip=skip, tau=tau)
    r = run(flow, 2.0)
    assert (r["valid"] == 255).all()                             # spread == tau passes
    assert np.array_equal(r["flows"][0, 0, 0, 1], np.asarray([-0.5, -0.5, -0.5, 0.5, 1.5, 1.5, 1.5], F))      # (0.5 + u - 1: T_2 is a shift by 1)
    r = run(flow, float(np.nextafter(F(2), F(0))))
    assert (r["valid"][0, 0][:, 3] == 0).all() and (np.delete(r["valid"][0, 0], 3, axis=1) == 255).all()
    assert (r["flows"][0, 0][:, :, 3] == 0).all()
    # fy == 0: the taps of the row below are unused, a NaN there changes nothing; in the used row it spoils two pixels
    unused = flow.copy()
    unused[0, 0, 2, 2] = np.nan
    a = run(unused, 2.0)
    assert (a["valid"][0, 0][[0, 1, 3]] == 255).all() and list(a["valid"][0, 0][2]) == [255, 0, 0, 255, 255, 255, 255]
    skip = np.zeros((1, 1, H, W), np.uint8)
    skip[0, 0, 1, 5] = 9
    b = run(flow, 2.0, skip)
    assert list(b["valid"][0, 0][1]) == [255, 255, 255, 255, 0, 0, 255] and (b["valid"][0, 0][[0, 2, 3]] == 255).all()


# ---- a link's flow and its frames' tracks agree ---------------------------------------------------------------------------------
def track_bound(T1, T2, w, h):
    """What |tracks[t+1] - P(pos[t+1])| and |P(pos[t+1]) - x - R| may add up to, f64[2,h,w], for the planted points
    pos[t] = T1 (x, y) and pos[t+1] = pos[t] + u(pos[t]), R = inv(T2)(q + u(q)) - x the real flow at q = T1 x.  Every
    float32 result contributes EPS times its magnitude (magnitudes from the float64 evaluation; SECOND_ORDER covers the
    products of two errors), and an error made early is carried through what follows:

      pos[t]   = the float64 q rounded once:                         Eq = EPS |q| per component
      pos[t+1] = the float64 pos[t] + u(pos[t]) rounded once:        Ep = EPS |p| + |I + G| Eq   (both terms move with pos[t])
      o = (Pa p.x + Pb p.y) + Pc: two products, two sums:            EPS (|Pa p.x| + |Pb p.y| + |Pa p.x + Pb p.y| + |o|)
      carried into it:                                               |Pa| Ep.x + |Pb| Ep.y
      P's coefficients, each the float64 inverse rounded once:       EPS (|Pa| |p.x| + |Pb| |p.y| + |Pc|)
    The subtraction of (x, y) is made in float64 by the test."""
    A1, P, _ = aug_cases._maps(T1, T2)
    ys, xs = np.mgrid[0:h, 0:w].astype(D)
    q = [A1[c, 0] * xs + A1[c, 1] * ys + A1[c, 2] for c in range(2)]
    Eq = [EPS * np.abs(q[c]) for c in range(2)]
    p = [q[c] + AFFINE_G[c, 0] * q[0] + AFFINE_G[c, 1] * q[1] + AFFINE_g[c] for c in range(2)]
    IG = np.abs(np.eye(2) + AFFINE_G)
    Ep = [EPS * np.abs(p[c]) + IG[c, 0] * Eq[0] + IG[c, 1] * Eq[1] for c in range(2)]
    bound = []
    for c in range(2):
        a, b, cc = P[c]
        t1, t2 = a * p[0], b * p[1]
        own = EPS * (np.abs(t1) + np.abs(t2) + np.abs(t1 + t2) + np.abs(t1 + t2 + cc))
        carried = abs(a) * Ep[0] + abs(b) * Ep[1]
        from_P = EPS * (abs(a) * np.abs(p[0]) + abs(b) * np.abs(p[1]) + abs(cc))
        bound.append(SECOND_ORDER * (own + carried + from_P))
    return np.stack(bound)


def planted(T1, w, h):
    """pos f32[2,w*h,2]: pos[0] = T1 (x, y) and pos[1] = pos[0] + u(pos[0]), each evaluated in float64 and rounded once"""
    A1 = np.asarray(T1, F).astype(D).reshape(2, 3)
    ys, xs = np.mgrid[0:h, 0:w].astype(D)
    x = np.stack([xs.ravel(), ys.ravel()], -1)
    p0 = (x @ A1[:, :2].T + A1[:, 2]).astype(F)
    p1 = (p0.astype(D) + p0.astype(D) @ AFFINE_G.T + AFFINE_g).astype(F)
    return np.stack([p0, p1])


def flow_track_check(name, out, valid, tracks, pos, T1, T2, w, h):
    """tracks[1] - (x, y) against the link's flow at (x, y), at the valid pixels -> the largest error / bound"""
    ys, xs = np.mgrid[0:h, 0:w].astype(D)
    x = np.stack([xs, ys])
    moved = tracks[1].astype(D).reshape(h, w, 2).transpose(2, 0, 1) - x
    bound = aug_cases.affine_bound(T1, T2, w, h) + track_bound(T1, T2, w, h)
    assert valid.mean() >= 0.25, (name, valid.mean())
    ratio = (np.abs(moved - out.astype(D)) / bound)[:, valid]
    assert (ratio <= 1).all(), (name, float(ratio.max()))
    # two misreadings of the tracks: frame t's inverse map used for frame t + 1; the map itself instead of its inverse
    A1, P2, A2 = aug_cases._maps(T1, T2)
    M = np.eye(3)
    M[:2] = A1
    P1 = np.linalg.inv(M)[:2]
    p = pos[1].astype(D).reshape(h, w, 2).transpose(2, 0, 1)
    at = lambda A: np.einsum("ij,jhw->ihw", A[:, :2], p) + A[:, 2, None, None] - x
    for what, wrong in (("P_t for frame t + 1", at(P1)), ("T instead of P", at(A2))):
        off = (np.abs(wrong - out.astype(D)) / bound).max(0)[valid]
        assert (off > 10).mean() >= 0.25, (name, what, float((off > 10).mean()))
    return float(ratio.max())


def flow_track_inputs():
    W, H, w, h = aug_cases.AFFINE_SIZES
    return aug_cases.affine_flow(W, H)[None, None], [(name, T1, T2, planted(T1, w, h)) for name, T1, T2 in aug_cases.affine_cases()]


def test_flow_and_tracks_agree_on_an_affine_field():
    """u(q) = G q + g on the 2^-6 lattice, 21 pairs of maps (tests/aug_cases.py): the twin's tracks[t+1] - (x, y) against
    its flow at (x, y) within the sum of aug_cases.affine_bound and track_bound.  Largest error / bound: DESIGN.md
    "Training clips"."""
    W, H, w, h = aug_cases.AFFINE_SIZES
    flow, cases = flow_track_inputs()
    worst = 0.0
    for name, T1, T2, pos in cases:
        r = clip_ref.augment(None, [[frame(T1), frame(T2)]], (w, h), links=[(0, 1)], flows=flow, pos=pos[None], tau=float("inf"),
                             want=("flows", "valid", "tracks"))
        worst = max(worst, flow_track_check(name, r["flows"][0, 0], r["valid"][0, 0] != 0, r["tracks"][0], pos, T1, T2, w, h))
    print("flow and tracks, twin: largest error / bound %.3f" % worst)
    assert worst > 0.01                                          # (the bound is no empty promise)


# ---- ArapFlow_ClipTables ----------------------------------------------------------------------------------------------------
def test_clip_tables_are_the_pair_tables_of_the_same_frame():
    from arap_flow_amd import data, opt
    scale, bias = (1 / 58.395, 1 / 57.12, 1 / 57.375), (-2.1179, -2.0357, -1.8044)
    for i in range(20):
        s = data.draw_sample(data.AUG_DEFAULT, 1, 0, i, 854, 480, 512, 384)
        P2, lut = opt.augment_tables(s, scale, bias)
        for k, f in enumerate((frame(s.T1, s.gain1, s.gamma1), frame(s.T2, s.gain2, s.gamma2, s.erase, s.fill))):
            P, t = opt.clip_tables(f, scale, bias)
            assert t.tobytes() == lut[k].tobytes()
            if k == 1:
                assert P.tobytes() == P2.tobytes()
            Pt, tt = clip_ref.tables(f, scale, bias)
            assert np.array_equal(P, Pt) and np.abs(t - tt).max() <= 1e-6 * np.abs(tt).max()
    P, lut = opt.clip_tables(opt.CLIP_NEUTRAL)
    assert np.array_equal(P, np.asarray(ID, F)) and np.array_equal(lut, np.tile(np.arange(256, dtype=F), (3, 1)))
    P, _ = opt.clip_tables(frame((2, 0, 3, 0, 4, -8)))
    assert np.array_equal(P, np.asarray([0.5, 0, -1.5, 0, 0.25, 2], F))


def test_clip_tables_refusals_and_names():
    from arap_flow_amd import capi, opt
    lib = capi.load()
    assert C.sizeof(capi.ClipFrame) == 120
    assert (capi.CLIP_MAX_FRAMES, capi.CLIP_MAX_LINKS) == (16, 32)
    nan, inf = float("nan"), float("inf")
    for bad in (frame((1, 0, nan, 0, 1, 0)), frame((inf, 0, 0, 0, 1, 0)), frame((1, 2, 0, 2, 4, 0)), frame((0, 0, 0, 0, 0, 0)),
                frame(gain=(1, 0, 1)), frame(gain=(1, -1, 1)), frame(gain=(nan, 1, 1)), frame(gain=(1, 1, inf)), frame(gamma=0.0),
                frame(gamma=-1.0), frame(gamma=nan), frame(gamma=inf)):
        with pytest.raises(ValueError):
            opt.clip_tables(bad)
        with pytest.raises(ValueError):
            clip_ref.tables(bad)
    f3 = (C.c_float * 3)(1, 1, 1)
    P, lut, good = (C.c_float * 6)(), (C.c_float * 768)(), opt.clip_frame(opt.CLIP_NEUTRAL)
    assert lib.ArapFlow_ClipTables(C.byref(good), f3, f3, P, lut) == 0
    assert lib.ArapFlow_ClipTables(None, f3, f3, P, lut) == -1
    assert lib.ArapFlow_ClipTables(C.byref(good), None, f3, P, lut) == -1
    assert lib.ArapFlow_ClipTables(C.byref(good), f3, None, P, lut) == -1
    assert lib.ArapFlow_ClipTables(C.byref(good), f3, f3, None, lut) == -1
    assert lib.ArapFlow_ClipTables(C.byref(good), f3, f3, P, None) == -1
    with pytest.raises(ValueError):
        opt.clip_frame(frame(erase=((0, 0, 1, 1),) * 5))
    good.n_erase = 77                                                   # (the rectangles are not read)
    assert lib.ArapFlow_ClipTables(C.byref(good), f3, f3, P, lut) == 0
