"""Cases for the tests of DESIGN.md "Training batches", and a statement of the augmented flow that does not go through
tests/aug_ref.py: for a source flow that is affine in the pixel the truth is a closed form, evaluated in float64, and the
error a float32 evaluation in the order of DESIGN.md may make is bounded operation by operation (`affine_bound`)."""
import math

import numpy as np

F = np.float32
D = np.float64
ID = (1, 0, 0, 0, 1, 0)
EPS = 2.0 ** -24                    # the relative error of one float32 operation, rounded to nearest
SECOND_ORDER = 1 + 2.0 ** -16       # the products of two such errors, which the sums below leave out: fewer than 2^8 of them


def rot(angle, scale, cx, cy, ox, oy):
    """output pixel -> source point: a rotation by `angle` and a scale about the output point (ox, oy), which shows the
    source point (cx, cy); composed in double"""
    a, b = scale * math.cos(angle), -scale * math.sin(angle)
    return (a, b, cx - (a * ox + b * oy), -b, a, cy - (-b * ox + a * oy))


def transforms(W, H, w, h):
    """the identity, the exact cases of the definition, a rotation with scale and a relative motion of frame 2, and a map
    that leaves the source; with tone curves, rectangles and fills of their own"""
    from arap_flow_amd import opt
    r1 = rot(0.2, 1.3, (W - 1) / 2, (H - 1) / 2, (w - 1) / 2, (h - 1) / 2)
    r2 = rot(0.23, 1.25, (W - 1) / 2 + 0.7, (H - 1) / 2 - 0.4, (w - 1) / 2, (h - 1) / 2)
    out = rot(-0.4, 2.5, -3.0, H + 2.0, 0, 0)
    S = opt.AugSample
    return [S(ID, ID, (1, 1, 1), 1.0, (1, 1, 1), 1.0, (), (0, 0, 0)),
            S((1, 0, 3, 0, 1, 1), (1, 0, 3, 0, 1, 1), (1.1, 0.9, 1.0), 0.8, (0.9, 1.0, 1.2), 1.1, ((1, 0, 3, 2),), (0.5, -1, 2)),
            S((-1, 0, W - 1, 0, 1, 0), (-1, 0, W - 1, 0, 1, 0), (1, 1, 1), 2.2, (1, 1, 1), 0.45, (), (0, 0, 0)),
            S((2, 0, 0, 0, 2, 0), (2, 0, 0, 0, 2, 0), (1.5, 1.5, 0.5), 1.0, (1, 1, 1), 1.0, ((-4, -4, 2, 1), (w - 1, h - 1, w + 5, h + 5)), (1, 2, 3)),
            S(ID, (1, 0, 2, 0, 1, 1), (1, 1, 1), 1.0, (0.8, 0.8, 0.8), 1.3, (), (0, 0, 0)),
            S(r1, r2, (1.2, 1.0, 0.8), 0.9, (1.0, 1.1, 0.9), 1.2,
              ((2, 1, 9, 4), (w // 2, 0, w // 2 + 7, h), (-3, h - 2, 4, h + 3), (w + 1, h + 1, w + 9, h + 9)), (0.25, 0.5, 0.75)),
            S(out, r2, (1, 1, 1), 1.0, (1, 1, 1), 1.0, (), (0, 0, 0))]


# ---- the flow under a general map, for a source flow u(q) = G q + g ------------------------------------------------------
# coefficients on the 2^-6 lattice: at the integer pixels of a source below 512 x 512 a sample is a multiple of 2^-6 below
# 2^6, which float32 holds exactly, and so it holds the difference of two samples
AFFINE_G = np.asarray([[3 / 64, -2 / 64], [1 / 64, 4 / 64]], D)
AFFINE_g = np.asarray([-1.25, 0.75], D)
AFFINE_SIZES = (70, 9, 48, 8)        # W, H, w, h


def affine_flow(W, H):
    """f32[H,W,2], the samples of u at the pixels, asserted exact"""
    ys, xs = np.mgrid[0:H, 0:W].astype(D)
    u = np.stack([AFFINE_G[0, 0] * xs + AFFINE_G[0, 1] * ys + AFFINE_g[0], AFFINE_G[1, 0] * xs + AFFINE_G[1, 1] * ys + AFFINE_g[1]], -1)
    assert np.array_equal(u.astype(F).astype(D), u)
    return u.astype(F)


def affine_cases():
    """[(name, T1, T2)]: transforms()[5], and draw_sample(AUG_DEFAULT, seed 0, epoch 0, index 0 .. 19) for 70x9 -> 48x8.
    Each shows more than 0.3 of the crop inside the source (affine_check asserts a quarter)."""
    from arap_flow_amd import data
    W, H, w, h = AFFINE_SIZES
    s = transforms(W, H, w, h)[5]
    cases = [("rotation", s.T1, s.T2)]
    for i in range(20):
        s = data.draw_sample(data.AUG_DEFAULT, 0, 0, i, W, H, w, h)
        cases.append(("draw%d" % i, s.T1, s.T2))
    return cases


def _maps(T1, T2):
    """the float32 coefficients as float64: A1 2x3, the inverse of T2 as a map P 2x3 in float64"""
    A1 = np.asarray(T1, F).astype(D).reshape(2, 3)
    M = np.eye(3)
    M[:2] = np.asarray(T2, F).astype(D).reshape(2, 3)
    return A1, np.linalg.inv(M)[:2], M[:2]


def affine_truth(T1, T2, w, h):
    """inv(T2)(T1 x + u(T1 x)) - x in float64 -> (truth f64[2,h,w], q1 f64[2,h,w])"""
    A1, P, _ = _maps(T1, T2)
    ys, xs = np.mgrid[0:h, 0:w].astype(D)
    x = np.stack([xs, ys])
    q = np.einsum("ij,jhw->ihw", A1[:, :2], x) + A1[:, 2, None, None]
    p = q + np.einsum("ij,jhw->ihw", AFFINE_G, q) + AFFINE_g[:, None, None]
    return np.einsum("ij,jhw->ihw", P[:, :2], p) + P[:, 2, None, None] - x, q


def affine_wrong_forms(T1, T2, w, h):
    """{name: f64[2,h,w]}: four plausible misreadings of the definition"""
    A1, P2, A2 = _maps(T1, T2)
    M = np.eye(3)
    M[:2] = A1
    P1 = np.linalg.inv(M)[:2]
    ys, xs = np.mgrid[0:h, 0:w].astype(D)
    x = np.stack([xs, ys])
    at = lambda A, v: np.einsum("ij,jhw->ihw", A[:, :2], v) + A[:, 2, None, None]
    u = lambda q: np.einsum("ij,jhw->ihw", AFFINE_G, q) + AFFINE_g[:, None, None]
    q1, q2 = at(A1, x), at(A2, x)
    return {"inverse of T1": at(P1, q1 + u(q1)) - x,
            "x not subtracted": at(P2, q1 + u(q1)),
            "u taken at T2 x": at(P2, q1 + u(q2)) - x,
            "u past the linear part": at(P2, q1) - x + u(q1)}


def affine_bound(T1, T2, w, h):
    """What |out - truth| may be per component and pixel when `out` is evaluated in float32 in DESIGN.md's order, f64[2,h,w].
    Every float32 operation contributes EPS times the magnitude of its result (magnitudes from the float64 evaluation;
    SECOND_ORDER covers the rest), and an error made early is carried through the operations after it:

      q1 = (a x + b y) + c         two products, two sums: Eq = EPS (|a x| + |b y| + |a x + b y| + |q1|) per component
      taps                         fx = bx - x0 is exact (the fraction of a float32 is one); the samples are exact
      u = mix(c00, c01, c10, c11)  in real arithmetic the mix of an affine field is u(q1) itself.  Ten operations:
                                   top = c00 + fx (c01 - c00) and bot: a difference (|G_c0|), a product (at most |G_c0|), a
                                   sum (at most U, the largest tap); bot - top (|G_c1|, and it carries Etop + Ebot),
                                   fy (..) with fy <= 1, top + (..).  With Etop = Ebot = EPS (2 |G_c0| + U):
                                   Eu = 3 Etop + 2 EPS |G_c1| + EPS U = EPS (6 |G_c0| + 2 |G_c1| + 4 U),
                                   U = |u(q1)| + |G_c0| + |G_c1| + |G_c .| Eq (the taps lie within a pixel of the rounded q1)
      out = (((Pa q1.x + Pb q1.y) + Pc) - x) + (Pa u.x + Pb u.y): nine operations, EPS times each result
      carried into it              Eq through P2 (I + G): u is taken at the rounded q1, so both q1 and u(q1) move;
                                   Eu through |Pa|, |Pb|;
                                   P2's coefficients, each the float64 inverse rounded once: EPS (|Pa| |q1.x + u.x| +
                                   |Pb| |q1.y + u.y| + |Pc|)
    The float64 evaluation of the truth itself errs by 2^-53 relative per operation, 2^-29 of the above."""
    A1, P, _ = _maps(T1, T2)
    G, g = AFFINE_G, AFFINE_g
    ys, xs = np.mgrid[0:h, 0:w].astype(D)
    x = [xs, ys]
    q, Eq = [], []
    for c in range(2):
        ax, by = A1[c, 0] * xs, A1[c, 1] * ys
        q.append(ax + by + A1[c, 2])
        Eq.append(EPS * (np.abs(ax) + np.abs(by) + np.abs(ax + by) + np.abs(q[c])))
    u, Eu = [], []
    for c in range(2):
        u.append(G[c, 0] * q[0] + G[c, 1] * q[1] + g[c])
        U = np.abs(u[c]) + abs(G[c, 0]) + abs(G[c, 1]) + abs(G[c, 0]) * Eq[0] + abs(G[c, 1]) * Eq[1]
        Eu.append(EPS * (6 * abs(G[c, 0]) + 2 * abs(G[c, 1]) + 4 * U))
    IG = np.abs(np.eye(2) + G)
    bound = []
    for c in range(2):
        a, b, cc = P[c]
        t1, t2, v1, v2 = a * q[0], b * q[1], a * u[0], b * u[1]
        t4 = t1 + t2 + cc
        own = EPS * (np.abs(t1) + np.abs(t2) + np.abs(t1 + t2) + np.abs(t4) + np.abs(t4 - x[c]) + np.abs(v1) + np.abs(v2) +
                     np.abs(v1 + v2) + np.abs(t4 - x[c] + v1 + v2))
        from_q = abs(a) * (IG[0, 0] * Eq[0] + IG[0, 1] * Eq[1]) + abs(b) * (IG[1, 0] * Eq[0] + IG[1, 1] * Eq[1])
        from_u = abs(a) * Eu[0] + abs(b) * Eu[1]
        from_P = EPS * (abs(a) * np.abs(q[0] + u[0]) + abs(b) * np.abs(q[1] + u[1]) + abs(cc))
        bound.append(SECOND_ORDER * (own + from_q + from_u + from_P))
    return np.stack(bound)


def affine_check(name, out, valid, T1, T2, W, H):
    """`out` f32[2,h,w] and `valid` bool[h,w] of one case against the closed form -> the largest error / bound.  Asserts:
    valid is inside(q1) wherever the float64 q1 is not within Eq of the source's border; a quarter of the crop is valid;
    the error is within the bound at every valid pixel; each wrong form misses the truth by more than ten times the bound
    on a quarter of the valid pixels."""
    h, w = valid.shape
    truth, q = affine_truth(T1, T2, w, h)
    bound = affine_bound(T1, T2, w, h)
    lim = np.asarray([W - 1, H - 1], D)[:, None, None]
    margin = np.minimum(q, lim - q).min(0)                     # > 0: inside
    slack = 2.0 ** -20 * (1 + np.abs(q).max(0))                # far above Eq (2^-22 relative at the most), far below a pixel
    assert (valid[margin > slack]).all() and not valid[margin < -slack].any(), name
    assert valid.mean() >= 0.25, (name, valid.mean())
    err = np.abs(out.astype(D) - truth)
    ratio = (err / bound)[:, valid]
    assert (ratio <= 1).all(), (name, float(ratio.max()))
    for what, wrong in affine_wrong_forms(T1, T2, w, h).items():
        off = (np.abs(wrong - truth) / bound).max(0)[valid]
        assert (off > 10).mean() >= 0.25, (name, what, float((off > 10).mean()))
    return float(ratio.max())


# ---- device work of a known duration ------------------------------------------------------------------------------------
class BusyWork:
    """A chain of 4096 x 4096 float32 matrix products on `stream`, one product timed once with events (`each`, seconds).
    queue(seconds) enqueues about that much work and returns at once: what a test puts in front of a call to see whether
    the call waits for its stream."""
    N = 4096

    def __init__(self, stream):
        import torch
        self.torch, self.stream = torch, stream
        with torch.cuda.stream(stream):
            self.x = torch.full((self.N, self.N), 1.0 / self.N, device="cuda")           # x @ x == x: nothing overflows
            self.y = torch.empty_like(self.x)
            torch.mm(self.x, self.x, out=self.y)                                          # (the BLAS library's first call)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(8):
                torch.mm(self.x, self.x, out=self.y)
            b.record()
        b.synchronize()
        self.each = a.elapsed_time(b) / 8e3

    def queue(self, seconds):
        n = max(1, int(math.ceil(seconds / self.each)))
        with self.torch.cuda.stream(self.stream):
            for _ in range(n):
                self.torch.mm(self.x, self.x, out=self.y)
        return n
