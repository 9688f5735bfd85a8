"""The inputs of the Gauss-Newton pins, in one place: tests/test_gn_host.py (CPU: the float64 twin tests/gn_ref.py against
the oracle, the oracle against the direct solve of the normal equations and against the energy), tests/test_gpu_gn.py
(GPU: the HIP paths against the same direct solves) and test_closed_forms_match_finite_differences of tests/test_oracle.py
read the same list.  Every case is a function of its name.

The inputs are chosen, and what they were chosen for is asserted here, on the case and not on the code under test
(check()): helpers.random_problem's 0.4 rad random start is a large-residual start on which undamped Gauss-Newton RISES
(cost 1.243 -> 1.337 from step 3 to step 20 at 12x10), so nothing about a minimum can be asked there; and a random mask can
leave vertices without an edge and without a handle, where J^T J is singular.  So:

  pixel-grid cases  UrShape = Offset = the pixel grid, Angle = 0, six handles (a frame as the generator starts it), as
    rigid  handles that agree with ONE rigid motion, a rotation of 0.3 rad about the centre plus a translation: the
           minimum is that motion, Angle = 0.3 everywhere, energy 0
    bent   the same with two handles moved by 2 px: the minimum has energy > 0
  tile    12x10 full mask: one column of 32-wide tiles, two bands of 8 rows
  seam    33x9 full mask: active edges across x = 31 | 32 and y = 7 | 8, one handle on each side of each
  blob    24x16 ellipse: excluded neighbours, vertices of degree 1, 2, 3 and 4
  holes   40x12: a block with single-vertex holes, a one-vertex-wide stripe across x = 31 | 32, and two isolated vertices
          with no edge and no handle -- the singular case
  generic 12x10, helpers.random_problem with a generic UrShape and non-zero angles: iterate and direct-solve checks only
  tile_bent_w10   `tile_bent` at weights 10 / 0.1 instead of the frame solver's 100 / 0.01 (opt.py: CombinedSolver.solve_all)

Arrays are float32-representable, so the float32 and the float64 code see the same problem; `C_exact` keeps the handles of
a pixel-grid case before that rounding (for the closed form of `rigid`, which the rounded handles miss by 1e-6 px).
"""
import collections
import math
import time

import numpy as np

import helpers

THETA = 0.3
W_FRAME = (10.0, float(np.float32(0.1)))                         # sqrt(100), sqrt(0.01) as float32 holds them
W_OTHER = (float(np.float32(math.sqrt(10.0))), float(np.float32(math.sqrt(0.1))))
GENERIC_SEED = 7                                                 # (seeds 1, 2, 3, 5, 6 leave J^T J singular)

Case = collections.namedtuple("Case", "name shape variant W H wf wr")

_SIZES = dict(tile=(12, 10), seam=(33, 9), blob=(24, 16), holes=(40, 12), generic=(12, 10))
_HANDLES = dict(tile=[(1, 1), (10, 1), (1, 8), (10, 8), (5, 3), (6, 7)],
                seam=[(2, 1), (31, 2), (32, 5), (10, 7), (20, 8), (3, 6)],
                blob=[(4, 7), (20, 7), (12, 2), (12, 12), (8, 5), (16, 10)],
                holes=[(3, 2), (26, 9), (14, 6), (36, 5), (8, 9), (21, 1)])
_BENT = {1: (2.0, 0.0), 4: (0.0, -2.0)}                          # handle index -> what `bent` adds to its target
ISOLATED = [(39, 0), (39, 11)]                                   # of `holes`

CASES = [Case("%s_%s" % (s, v), s, v, *_SIZES[s], *W_FRAME) for s in ("tile", "seam", "blob", "holes") for v in ("rigid", "bent")]
CASES += [Case("generic", "generic", None, *_SIZES["generic"], *W_FRAME), Case("tile_bent_w10", "tile", "bent", *_SIZES["tile"], *W_OTHER)]
BY_NAME = {c.name: c for c in CASES}
GRID = [c for c in CASES if c.shape != "generic"]
RIGID = [c for c in CASES if c.variant == "rigid"]
BENT = [c for c in CASES if c.variant == "bent"]


def active(shape):
    """bool[H, W]: the vertices of a pixel-grid shape"""
    W, H = _SIZES[shape]
    ys, xs = np.mgrid[0:H, 0:W]
    if shape in ("tile", "seam"):
        return np.ones((H, W), bool)
    if shape == "blob":
        return ((xs - 12) / 11.0) ** 2 + ((ys - 7) / 6.2) ** 2 <= 1.0
    a = np.zeros((H, W), bool)
    a[1:11, 2:28] = ~((xs[1:11, 2:28] % 5 == 0) & (ys[1:11, 2:28] % 3 == 2))
    a[5, 28:38] = True
    for x, y in ISOLATED:
        a[y, x] = True
    return a


def degree(act):
    """number of active neighbours of every vertex (0 on excluded ones)"""
    p = np.pad(act, 1)
    return (p[1:-1, 2:].astype(int) + p[1:-1, :-2] + p[2:, 1:-1] + p[:-2, 1:-1]) * act


def rigid_map(case):
    """float64 [H, W, 2]: where the rigid motion of the case's shape takes every pixel"""
    W, H = case.W, case.H
    ys, xs = np.mgrid[0:H, 0:W]
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    c, s = math.cos(THETA), math.sin(THETA)
    tx, ty = math.ceil(cy * s) + 1.0, math.ceil(cx * s) + 1.0     # keeps every target inside x, y >= 0
    dx, dy = xs - cx, ys - cy
    return np.stack([cx + c * dx - s * dy + tx, cy + s * dx + c * dy + ty], -1)


_PROBLEMS = {}


def problem(case):
    """dict(O, A, U, C, M: float64 arrays of float32-representable values; C_exact for pixel-grid cases); cached, read-only"""
    if case.name not in _PROBLEMS:
        W, H = case.W, case.H
        if case.shape == "generic":
            pb = helpers.random_problem(W, H, seed=GENERIC_SEED, generic_urshape=True, ncons=6)
            pb = {k: pb[k].astype(np.float64) for k in "OAUCM"}
        else:
            ys, xs = np.mgrid[0:H, 0:W]
            grid = np.stack([xs, ys], -1).astype(np.float64)
            act, rm = active(case.shape), rigid_map(case)
            C = -np.ones((H, W, 2))
            for k, (x, y) in enumerate(_HANDLES[case.shape]):
                assert act[y, x]
                C[y, x] = rm[y, x] + (_BENT.get(k, (0.0, 0.0)) if case.variant == "bent" else (0.0, 0.0))
                assert (C[y, x] > 0).all()
            pb = dict(O=grid.copy(), A=np.zeros((H, W)), U=grid, C=C.astype(np.float32).astype(np.float64),
                      M=np.where(act, 0.0, 255.0), C_exact=C)
        for a in pb.values():
            a.setflags(write=False)
        _PROBLEMS[case.name] = pb
    return _PROBLEMS[case.name]


def args(case, exact=False):
    pb = problem(case)
    return pb["O"], pb["A"], pb["U"], pb["C_exact" if exact else "C"], pb["M"], case.wf, case.wr


def handles(case):
    return _HANDLES[case.shape]


# ---- the plain reference: a central-difference Jacobian of the residual definition, and the direct solve ------------------

EPS = 1e-6
jacobian_seconds = {}


def jacobian_at(orc, U, C, M, wf, wr, O, A):
    """(J[residuals, 3 * active], F[residuals], idx): central differences (EPS) of oracle.residuals -- arap_plan.t:14-23 and
    nothing else -- at (O, A), over the unknowns of active vertices; idx are their positions in a flattened [H, W, 3]"""
    U, C, M = (np.asarray(v, np.float64) for v in (U, C, M))
    H, W = M.shape
    x0 = np.concatenate([np.asarray(O, np.float64).reshape(-1, 2), np.asarray(A, np.float64).reshape(-1, 1)], 1).reshape(-1)

    def res(x):
        x = x.reshape(-1, 3)
        return orc.residuals(x[:, :2].reshape(H, W, 2), x[:, 2].reshape(H, W), U, C, M, wf, wr, dtype=np.float64).reshape(-1)

    idx = np.flatnonzero(np.repeat(M.reshape(-1) == 0, 3))
    F = res(x0)
    J = np.zeros((F.size, idx.size))
    for k, j in enumerate(idx):
        xp, xm = x0.copy(), x0.copy()
        xp[j] += EPS
        xm[j] -= EPS
        J[:, k] = (res(xp) - res(xm)) / (2 * EPS)
    return J, F, idx


def jacobian(orc, case, O, A, exact=False):
    return jacobian_at(orc, *args(case, exact)[2:], O, A)


class Direct:
    """the Gauss-Newton step of a case from its start, by least squares on the finite-difference Jacobian: dstar =
    lstsq(J, -F) (minimum norm where J^T J is singular), and the A-seminorm |J v| of a step's error against it"""

    def __init__(self, orc, case):
        O, A = args(case)[:2]
        t0 = time.perf_counter()
        self.J, self.F, self.idx = jacobian(orc, case, O, A)
        jacobian_seconds[case.name] = time.perf_counter() - t0
        self.dstar = np.linalg.lstsq(self.J, -self.F, rcond=None)[0]
        self.norm = float(np.linalg.norm(self.J @ self.dstar))
        self.O, self.A = O, A

    def error(self, delta):
        """|delta - dstar|_A / |dstar|_A of a step delta[H, W, 3]"""
        e = np.asarray(delta, np.float64).reshape(-1)[self.idx] - self.dstar
        return float(np.linalg.norm(self.J @ e)) / self.norm

    def error_of(self, O, A):
        """the same of the state (O, A) one step leaves"""
        return self.error(np.concatenate([np.asarray(O, np.float64) - self.O, (np.asarray(A, np.float64) - self.A)[..., None]], -1))

    def rank_deficit(self):
        return self.J.shape[1] - int(np.linalg.matrix_rank(self.J))


_DIRECT = {}


def direct(orc, case):
    if case.name not in _DIRECT:
        _DIRECT[case.name] = Direct(orc, case)
    return _DIRECT[case.name]


def newton_decrement_at(orc, U, C, M, wf, wr, O, A):
    """sqrt(g^T (J^T J)^+ g) at (O, A), g = J^T F, everything from finite differences of the residuals there: the length, in
    the energy norm, of the Gauss-Newton step still to take"""
    J, F, _ = jacobian_at(orc, U, C, M, wf, wr, O, A)
    step = np.linalg.lstsq(J, -F, rcond=None)[0]
    return float(np.linalg.norm(J @ step))


def newton_decrement(orc, case, O, A):
    return newton_decrement_at(orc, *args(case)[2:], O, A)


def half_ssq_at(orc, U, C, M, wf, wr, O, A):
    """0.5 |F|^2 from oracle.residuals at (O, A)"""
    f64 = lambda v: np.asarray(v, np.float64)
    F = orc.residuals(f64(O), f64(A), f64(U), f64(C), f64(M), wf, wr, dtype=np.float64)
    return 0.5 * float((F * F).sum())


def half_ssq(orc, case, O, A, exact=False):
    return half_ssq_at(orc, *args(case, exact)[2:], O, A)


# ---- what the cases were chosen for ----------------------------------------------------------------------------------

def check(orc, case):
    """the case's preconditions (on the case, not on the code under test)"""
    pb = problem(case)
    act = pb["M"] == 0
    fit = (pb["C"] >= 0).all(-1) & act
    deficit = direct(orc, case).rank_deficit()
    if case.shape == "generic":
        assert not np.array_equal(pb["U"], np.stack(np.mgrid[0:case.H, 0:case.W][::-1], -1)) and np.abs(pb["A"]).max() > 0.1
        assert deficit == 0 and (~act).any()
        return
    assert fit.sum() == 6 and np.array_equal(pb["O"], pb["U"]) and not pb["A"].any()
    deg = degree(act)
    hs = handles(case)
    if case.shape == "tile":
        assert act.all() and case.W <= 32 and 8 < case.H <= 16
    if case.shape == "seam":
        assert act.all() and case.W == 33 and case.H == 9                      # every edge across x = 31 | 32 and y = 7 | 8 is active
        assert any(x == 31 for x, _ in hs) and any(x == 32 for x, _ in hs) and any(y == 7 for _, y in hs) and any(y == 8 for _, y in hs)
    if case.shape == "blob":
        assert all(((deg == d) & act).any() for d in (1, 2, 3, 4)) and (~act).any()
    if case.shape == "holes":
        assert act[5, 31] and act[5, 32] and not act[4, 28:38].any() and not act[6, 28:38].any()     # the stripe, across 31 | 32
        assert (act[7, 2:28] & act[8, 2:28]).any()                                                    # edges across y = 7 | 8
        holes = ~act[1:11, 2:28]
        assert holes.sum() == 15 and (degree(~act)[1:11, 2:28][holes] == 0).all()                     # single-vertex holes
        assert all(act[y, x] and deg[y, x] == 0 and not fit[y, x] for x, y in ISOLATED)
        assert ((deg == 0) & act).sum() == len(ISOLATED)
        assert all(((deg == d) & act).any() for d in (1, 2, 3, 4))
        assert deficit == 3 * len(ISOLATED)                                     # singular, and by the isolated vertices alone
    else:
        assert deficit == 0
    if case.variant == "rigid":
        assert half_ssq(orc, case, rigid_map(case), np.full((case.H, case.W), THETA), exact=True) < 1e-24
