"""An independent float64 twin of the "gaussNewtonGPU" solver kind, in plain numpy, and of the frame schedule around it.

Written from the reference's solver, ARAP/API/src/solverGPUGaussNewton.t: init :956-1007, the Gauss-Newton branch of the
step :1016-1177, PCGInit1 :361-397 with guardedInvert :323-351 in the variant the reference builds with (CERES, selected at
:22) and the `usepreconditioner` switch (:379-381, :467-470; what it does to evalJTF's second output is o.t:2162-2167),
PCGStep1 :421-434, PCGStep2 :446-489 without q, PCGStep3 :537-550, PCGLinearUpdate :552-557, and the guards against a
division by zero (:17, :457, :545) -- not from the oracle's restatement of them (oracle/arap_oracle_impl.h: solve_), which
this twin is there to pin.  The frame schedule is written from ARAP/deformation/src/main.cpp:130-136 (border pins),
ARAP/deformation/src/CombinedSolver.h:172-189 (weights), :199-201 (ramp fraction), :207-221 (resetGPU), :223-242
(setConstraintImage) and ARAP/shared/CombinedSolverBase.h:99-120 (singleSolve) -- not from oracle_frame.

Like tests/lm_ref.py it stands on three float64 primitives only, each pinned by finite differences in tests/test_oracle.py:
  oracle.evalJTF   g = J^T F and diag(J^T J)
  oracle.applyJTJ  J^T J p
  oracle.cost      0.5 |F|^2
Everything else is numpy on [H, W, 3] images (Offset.x, Offset.y, Angle).  Sums are numpy's pairwise float64 sums:
summation order is the only thing that separates this loop from oracle.solve(dtype=float64).

pcg() is the loop body both solver kinds share; tests/lm_ref.py adds q, CtC and the residual reset around it.
"""
import numpy as np


def dot(a, b):
    return float((a * b).sum())


def pcg(apply_a, r, p, pre, lIterations, reset=None):
    """The PCG loop of the step (:1056-1103) from the state PCGInit1 leaves: residual r, direction p, and the
    preconditioner `pre` that PCGStep2 applies.  Yields (l + 1, delta, r) after inner iteration l.  `reset(l, delta)`, when
    given, returns the recomputed residual of an iteration that resets it (LM only, :1077-1083), else None."""
    delta = np.zeros_like(r)
    rho = dot(r, p)                                             # scanAlphaNumerator, PCGInit1 :389,395
    for l in range(lIterations):
        Ap = apply_a(p)                                         # PCGStep1 :427-429
        sigma = dot(p, Ap)
        alpha = rho / sigma if sigma > 0.0 else 0.0             # PCGStep2 :456-459
        delta = delta + alpha * p                               # :461
        fresh = reset(l, delta) if reset is not None else None
        r = r - alpha * Ap if fresh is None else fresh          # :464
        z = pre * r                                             # :472
        rho_new = dot(z, r)                                     # :475
        beta = rho_new / rho if rho > 0.0 else 0.0              # PCGStep3 :544-547: new over old
        p = z + beta * p                                        # :548
        rho = rho_new                                           # :1091
        yield l + 1, delta, r


def guarded_invert(d):
    """guardedInvert, CERES variant :327-331"""
    return 1.0 / (1.0 + np.sqrt(d)) ** 2


def solve(orc, O, A, U, Cn, M, wf, wr, nIterations, lIterations, use_preconditioner=True, iterates=None):
    """One Opt_ProblemSolve of kind "gaussNewtonGPU".  Returns (O, A, costs[0..nIterations]).  iterates: a list that
    receives, per Gauss-Newton step, the list of the PCG iterates delta_1 .. delta_L ([H, W, 3] each)."""
    f64 = lambda a: np.array(a, np.float64)
    O, A, U, Cn, M = f64(O), f64(A), f64(U), f64(Cn), f64(M)
    wf, wr = float(wf), float(wr)
    act = (M == 0)[..., None]                                   # Exclude(Not(eq(Mask(0,0),0))), arap_plan.t:11
    on = lambda v: np.where(act, v, 0.0)
    apply_a = lambda v: on(orc.applyJTJ(A, U, Cn, M, wf, wr, v, dtype=np.float64))
    costs = [orc.cost(O, A, U, Cn, M, wf, wr, dtype=np.float64)]                               # init :1006
    for _ in range(nIterations):                                                                # :1027
        g, diag = orc.evalJTF(O, A, U, Cn, M, wf, wr, dtype=np.float64)                        # PCGInit1 :375
        r = on(-g)                                                                              # :376-377
        if not use_preconditioner:
            diag = np.ones_like(diag)                                                           # o.t:2163-2164, :379-381
        pre = on(guarded_invert(diag))                                                          # :385 (also of the 1.0)
        p = pre * r                                                                             # :386
        loop_pre = pre if use_preconditioner else on(np.ones_like(pre))                         # PCGStep2 :467-470
        delta, its = np.zeros_like(r), []
        for _, delta, _ in pcg(apply_a, r, p, loop_pre, lIterations):
            its.append(delta)
        if iterates is not None:
            iterates.append(its)
        O, A = O + delta[..., :2], A + delta[..., 2]                                            # PCGLinearUpdate :555
        costs.append(orc.cost(O, A, U, Cn, M, wf, wr, dtype=np.float64))                        # :1117, :1161
    return O, A, np.asarray(costs)


# ---- the frame schedule ------------------------------------------------------------------------------------------------

def border_pins(W, H):
    """main.cpp:130-136: (x, y, x, y) of every border pixel, y outer, x inner, appended after the file's handles"""
    return [(x, y, x, y) for y in range(H) for x in range(W) if y == 0 or x == 0 or y == H - 1 or x == W - 1]


def constraint_image(mask_red, cons, alpha):
    """setConstraintImage, CombinedSolver.h:223-242: float32 arithmetic; a handle on an excluded pixel is dropped, a later
    handle on the same pixel overwrites an earlier one, the target is not looked at.  (The reference reads the mask out of
    bounds for a source outside the frame; such a handle is dropped here.)"""
    H, W = mask_red.shape
    img = np.full((H, W, 2), -1.0, np.float32)
    alpha, one = np.float32(alpha), np.float32(1.0)
    for x, y, tx, ty in cons:
        if not (0 <= x < W and 0 <= y < H):
            continue
        if mask_red[y, x] == 0:
            img[y, x, 0] = (one - alpha) * np.float32(x) + alpha * np.float32(tx)
            img[y, x, 1] = (one - alpha) * np.float32(y) + alpha * np.float32(ty)
    return img


def frame(orc, mask_red, cons, numIter, nIterations, lIterations, pins=True):
    """solveAll for one frame.  Returns (Offset, Angle, final_costs[numIter])."""
    mask_red = np.asarray(mask_red, np.uint8)
    H, W = mask_red.shape
    cons = [tuple(int(v) for v in c) for c in np.asarray(cons).reshape(-1, 4)] + (border_pins(W, H) if pins else [])
    ys, xs = np.mgrid[0:H, 0:W]
    U = np.stack([xs, ys], -1).astype(np.float32).astype(np.float64)                            # resetGPU :207-221
    O, A, M = U.copy(), np.zeros((H, W)), mask_red.astype(np.float32).astype(np.float64)
    wf = float(np.sqrt(np.float32(100.0)))                                                      # combinedSolveInit :173-177
    wr = float(np.sqrt(np.float32(0.01)))
    finals = []
    for i in range(numIter):                                                                    # singleSolve :99-120
        alpha = np.float32(i + 1) / np.float32(numIter)                                         # preNonlinearSolve :199-201
        Cn = constraint_image(mask_red, cons, alpha)
        O, A, costs = solve(orc, O, A, U, Cn, M, wf, wr, nIterations, lIterations)              # the unknowns carry over
        finals.append(costs[-1])
    return O, A, np.asarray(finals)
