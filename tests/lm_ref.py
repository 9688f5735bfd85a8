"""An independent float64 twin of the "LMGPU" solver kind, in plain numpy.

Written from the reference's solver, ARAP/API/src/solverGPUGaussNewton.t: the step at :1016-1177 and the kernels at
:361-397 (PCGInit1), :421-434 (PCGStep1), :446-489 (PCGStep2 with q), :491-535 (the residual reset), :537-557 (PCGStep3,
PCGLinearUpdate), :616-662 (PCGSaveSSq, PCGComputeCtC, PCGFinalizeDiagonal), guardedInvert :323-332 -- not from the
oracle's restatement of them (oracle/arap_oracle_impl.h: oracle_solve_lm), which this twin is there to pin.  The loop body
it shares with the Gauss-Newton kind (PCGStep1, the alpha, delta and r updates of PCGStep2, PCGStep3) is gn_ref.pcg.

It stands on three float64 primitives only, each pinned by finite differences in tests/test_oracle.py:
  oracle.evalJTF   g = J^T F and diag(J^T J)
  oracle.applyJTJ  J^T J p
  oracle.cost      0.5 |F|^2
Everything else is numpy on [H, W, 3] images (Offset.x, Offset.y, Angle).  The model cost 0.5 |F + J delta|^2
(computeModelCost :666-678) is not evaluated residual by residual: it is the quadratic identity
  0.5 |F + J d|^2 = 0.5 |F|^2 + g . d + 0.5 d . (J^T J d)
so nothing here knows what a residual looks like.  Sums are numpy's pairwise float64 sums: summation order is the only
thing that separates this loop from oracle.solve_lm(dtype=float64).
"""
import numpy as np

import gn_ref

OUTCOMES = ("accepted", "rejected", "function_tolerance", "min_radius")

DEFAULTS = dict(min_relative_decrease=1e-3, min_trust_region_radius=1e-32, max_trust_region_radius=1e16,
                q_tolerance=1e-4, function_tolerance=1e-6, trust_region_radius=1e4, radius_decrease_factor=2.0,
                min_lm_diagonal=1e-6, max_lm_diagonal=1e32)            # solverGPUGaussNewton.t:26-39


def model_cost(orc, O, A, U, Cn, M, wf, wr, delta, prev_cost=None):
    """0.5 |F + J delta|^2 at (O, A) by the quadratic identity; delta[H,W,3] is zero on excluded vertices"""
    g, _ = orc.evalJTF(O, A, U, Cn, M, wf, wr, dtype=np.float64)
    JtJd = orc.applyJTJ(A, U, Cn, M, wf, wr, delta, dtype=np.float64)
    if prev_cost is None:
        prev_cost = orc.cost(O, A, U, Cn, M, wf, wr, dtype=np.float64)
    return prev_cost + float((g * delta).sum()) + 0.5 * float((delta * JtJd).sum())


def solve_lm(orc, O, A, U, Cn, M, wf, wr, nIterations, lIterations, residual_reset_period=10, **lm):
    """Returns (O, A, costs[0..steps], steps, final radius, records): one record per step attempted, a dict of
    pcg_iterations, outcome (a name of OUTCOMES), radius and decrease after the step."""
    f64 = lambda a: np.array(a, np.float64)
    O, A, U, Cn, M = f64(O), f64(A), f64(U), f64(Cn), f64(M)
    wf, wr = float(wf), float(wr)
    par = dict(DEFAULTS)
    par.update(lm)
    act = (M == 0)[..., None]                                   # Exclude(Not(eq(Mask(0,0),0))), arap_plan.t:11
    on = lambda v: np.where(act, v, 0.0)
    dot = lambda a, b: float((a * b).sum())
    with np.errstate(all="ignore"):
        radius, decrease = par["trust_region_radius"], par["radius_decrease_factor"]        # init :996-1001
        prev_cost = orc.cost(O, A, U, Cn, M, wf, wr, dtype=np.float64)                          # :1006
        costs, records, SSq = [prev_cost], [], None
        n_iter = 0
        while n_iter < nIterations:                                                             # :1027
            # PCGInit1 :361-397
            g, diag = orc.evalJTF(O, A, U, Cn, M, wf, wr, dtype=np.float64)
            delta = np.zeros_like(g)
            r = on(-g)
            pre = on(1.0 / (1.0 + np.sqrt(diag)) ** 2)                                          # guardedInvert :323-332
            if n_iter == 0:
                SSq = pre.copy()                                                                # PCGSaveSSq, once per solve
            unclamped = on(diag / radius)                                                       # PCGComputeCtC
            mult = (1.0 / SSq) / radius                                                         # PCGFinalizeDiagonal :631-664
            CtC = on(np.minimum(np.maximum(unclamped, par["min_lm_diagonal"] * mult), par["max_lm_diagonal"] * mult))
            pre = on(1.0 / (CtC + radius * unclamped))
            b = r.copy()
            p = pre * r
            Q0 = 0.5 * dot(delta, r + r)
            apply_a = lambda v: on(orc.applyJTJ(A, U, Cn, M, wf, wr, v, dtype=np.float64) + CtC * v)   # o.t:2076-2082
            reset = lambda l, d: b - apply_a(d) if (l + 1) % residual_reset_period == 0 else None      # :1077-1083
            ran = 0
            for ran, delta, r in gn_ref.pcg(apply_a, r, p, pre, lIterations, reset):           # :1056-1103, PCGStep1-3
                Q1 = 0.5 * dot(delta, r + b)                                                    # PCGStep2 :477-482
                zeta = np.float64(ran) * (np.float64(Q1) - Q0) / np.float64(Q1)                # :1093-1102
                if zeta < par["q_tolerance"]:
                    break
                Q0 = Q1
            model_cost_change = np.float64(prev_cost) - model_cost(orc, O, A, U, Cn, M, wf, wr, delta, prev_cost)
            prev_O, prev_A = O, A                                                               # savePreviousUnknowns
            O, A = O + delta[..., :2], A + delta[..., 2]                                        # PCGLinearUpdate
            new_cost = orc.cost(O, A, U, Cn, M, wf, wr, dtype=np.float64)
            cost_change = np.float64(prev_cost) - new_cost
            relative_decrease = cost_change / model_cost_change
            if cost_change >= 0 and relative_decrease > par["min_relative_decrease"]:           # :1127
                if cost_change <= prev_cost * par["function_tolerance"]:
                    records.append(dict(pcg_iterations=ran, outcome="function_tolerance", radius=radius, decrease=decrease))
                    break
                tmp_factor = 1.0 - (2.0 * float(relative_decrease) - 1.0) ** 3
                radius = min(radius / max(1.0 / 3.0, tmp_factor), par["max_trust_region_radius"])
                decrease = 2.0
                prev_cost = new_cost
                outcome = "accepted"
            else:
                O, A = prev_O, prev_A                                                           # revertUpdate
                radius = radius / decrease
                decrease = 2.0 * decrease
                if radius <= par["min_trust_region_radius"]:
                    records.append(dict(pcg_iterations=ran, outcome="min_radius", radius=radius, decrease=decrease))
                    break
                outcome = "rejected"
            records.append(dict(pcg_iterations=ran, outcome=outcome, radius=radius, decrease=decrease))
            costs.append(prev_cost)
            n_iter += 1
    return O, A, np.asarray(costs), n_iter, radius, records
