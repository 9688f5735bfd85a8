"""The Gauss-Newton solve (oracle.solve, oracle.frame) pinned on the CPU by things that are not the oracle's own hands:

 (a) tests/gn_ref.py, a float64 numpy twin written from the reference's solver source, iterate by iterate;
 (b) the direct least-squares solve of the normal equations, built from a finite-difference Jacobian of the residual
     definition alone (tests/gn_cases.py: Direct): the PCG error against it never rises and ends at the floor;
 (c) the energy: a rigid set of handles is answered by that rigid motion, a bent one by a stationary point, and the cost
     reported is the energy at the state returned;
 (d) a numpy restatement of the frame schedule (gn_ref.frame) written from the reference's host code.

Every bound below is a measured number times a stated margin; DESIGN.md "Gauss-Newton: pins" has the same tables.  Cases and
their preconditions: tests/gn_cases.py."""
import numpy as np
import pytest

import gn_cases
import gn_ref
import helpers

NAMES = [c.name for c in gn_cases.CASES]
N_SET, L_SET = (1, 2, 3), (0, 1, 2, 3, 5, 30)

# (a) Twin against oracle.solve(dtype=float64).  Summation order is the only difference between the two sides, as for the LM
# twin (tests/test_lm_host.py: TWIN_BOUND 7.5e-11), but undamped PCG on these weights (100 against 0.01) amplifies a 1e-16
# far more than the LM loop with its CtC diagonal does, and an unconverged Gauss-Newton step hands the difference to the
# next one: two runs of the TWIN that differ only in how a dot product is summed (numpy's pairwise sum against math.fsum)
# part by 8.4e-10 / 1.3e-7 / 4.2e-6 after 1 / 2 / 3 steps of 30 iterations on seam_rigid.  So GN gets two bounds of its own.
#  * STEP_BOUND, every step on its own: step n of the twin taken FROM THE ORACLE'S state after step n - 1 against the
#    oracle's step n.  Worst of all cases, n and L: 9.83e-9 (Offset update, blob_rigid, n = 1, L = 30); bound = 10 x.
#  * RUN_BOUND, the free-running twin against the oracle after n steps.  Worst: 5.59e-5 (cost, seam_rigid, n = 3, L = 30;
#    Angle 1.37e-5, Offset 2.26e-6); bound = 10 x.  At L <= 5, where nothing has been amplified yet, the worst is 7.6e-13.
# Neither may be looser than 1e-3 of an update, and the step bound stays below what one float32 operation would show.
STEP_MEASURED, RUN_MEASURED = 9.83e-9, 5.59e-5
STEP_BOUND, RUN_BOUND = 10 * STEP_MEASURED, 10 * RUN_MEASURED
assert STEP_BOUND <= 1e-7 and RUN_BOUND <= 1e-3

# (b) |delta_L - dstar|_A / |dstar|_A of the first step at L = 300, dstar = lstsq(J, -F), J by central differences (1e-6) of
# oracle.residuals.  float32 is oracle.solve(dtype=float32, mode=1, trig=1): the arithmetic of the HIP kernels.
L_PCG = (1, 2, 3, 5, 10, 30, 100, 300)
FLOOR = {                # case: (float64, float32) measured
    "tile_rigid": (5.07e-10, 2.52e-7), "tile_bent": (6.39e-10, 1.91e-7), "seam_rigid": (4.10e-10, 3.03e-7),
    "seam_bent": (4.58e-10, 5.69e-7), "blob_rigid": (7.36e-10, 3.17e-7), "blob_bent": (7.71e-10, 2.58e-7),
    "holes_rigid": (7.16e-10, 2.78e-7), "holes_bent": (7.12e-10, 2.50e-7), "generic": (4.55e-10, 2.05e-7),
    "tile_bent_w10": (3.77e-10, 3.46e-7),
}
# float64: the floor is the finite-difference Jacobian's own error, margin 10; float32: the floor is the arithmetic, margin 4
FLOOR64_BOUND = 10 * max(v[0] for v in FLOOR.values())
FLOOR32_BOUND = 4 * max(v[1] for v in FLOOR.values())
# PCG does not let the energy-norm error rise, whatever the SPD preconditioner.  What may rise is what is measured: the
# norm goes through J (relative error ~1e-9 from the differences, so 1e-6 relative is generous for float64 rounding), and
# once the error is at the floor it is the sum of a still-falling part and a constant one (the Jacobian's error, or the
# float32 quantisation of the state), whose norm may move by the size of the floor itself.
RISE_RELATIVE = 1e-6

# (c) the outer loop, PCG converged (L = 300).  float64 from the exact handles, four steps, against the closed form:
# worst |Offset - rigid map| 5.33e-14 px and |Angle - 0.3| 1.37e-14 rad (seam_rigid); bounds 10 x.
L_CONV, N_RIGID, N_BENT = 300, 4, 20
RIGID_OFFSET_MEASURED, RIGID_ANGLE_MEASURED = 5.33e-14, 1.37e-14
RIGID_OFFSET_BOUND, RIGID_ANGLE_BOUND = 10 * RIGID_OFFSET_MEASURED, 10 * RIGID_ANGLE_MEASURED
# Newton decrement sqrt(g^T (J^T J)^+ g) from finite differences at the result: case: (float64, float32) measured.  The
# float32 values are the stall levels: no further step lowers them.
DECREMENT = {
    "tile_rigid": (0.0, 8.74e-7), "seam_rigid": (0.0, 2.98e-6), "blob_rigid": (0.0, 2.35e-6), "holes_rigid": (0.0, 2.55e-6),
    "tile_bent": (4.22e-7, 7.69e-6), "seam_bent": (8.73e-10, 2.24e-5), "blob_bent": (1.07e-10, 1.09e-5), "holes_bent": (4.84e-11, 2.33e-5),
    "tile_bent_w10": (9.45e-7, 3.67e-6),
}
DECREMENT64_BOUND = 10 * max(v[0] for v in DECREMENT.values())
DECREMENT32_BOUND = 4 * max(v[1] for v in DECREMENT.values())


def _update(O, A, O0, A0):
    return np.concatenate([np.asarray(O, np.float64) - O0, (np.asarray(A, np.float64) - A0)[..., None]], -1)


def _dev(got, ref, base):
    """(Offset update rel-L2, Angle update rel-L2, worst relative cost difference) of (O, A, costs) against the oracle's"""
    rel = lambda a, b: float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(b))))
    return (helpers.rel_l2(got[0] - base[0], ref[0] - base[0]), helpers.rel_l2(got[1] - base[1], ref[1] - base[1]),
            rel(got[2], ref[2]))


@pytest.mark.parametrize("name", NAMES)
def test_case_preconditions(oracle, name):
    gn_cases.check(oracle, gn_cases.BY_NAME[name])


@pytest.mark.parametrize("name", NAMES)
def test_twin_vs_oracle_float64(oracle, name):
    """nIterations 1, 2, 3 x lIterations 0, 1, 2, 3, 5, 30: Offset, Angle and every cost; a first-step mismatch names the
    first PCG iterate that differs"""
    case = gn_cases.BY_NAME[name]
    a = gn_cases.args(case)
    start = a[:2]
    its = []
    gn_ref.solve(oracle, *a, 1, max(L_SET), iterates=its)
    worst_step = worst_run = 0.0
    for L in L_SET:
        prev = start
        for n in N_SET:
            ref = oracle.solve(*a, n, L, dtype=np.float64)
            assert len(ref[2]) == n + 1
            if L == 0:                                       # the API takes it: no PCG iteration, nothing moves, n + 1 equal costs
                tw = gn_ref.solve(oracle, *a, n, 0)
                assert all(np.array_equal(x[0], start[0]) and np.array_equal(x[1], start[1]) for x in (ref, tw))
                assert len(set(ref[2].tolist())) == 1 and len(set(tw[2].tolist())) == 1
                assert abs(tw[2][0] - ref[2][0]) <= 1e-14 * ref[2][0]
                continue
            if n == 1:
                d = _update(ref[0], ref[1], *start)
                dev = helpers.rel_l2(its[0][L - 1], d)
                assert dev <= STEP_BOUND, "%s: PCG iterate %d is the first to differ (%.3g)" % (name, L, dev)
            step = gn_ref.solve(oracle, prev[0], prev[1], *a[2:], 1, L)
            ds = _dev(step, (ref[0], ref[1], ref[2][-2:]), prev)
            run = gn_ref.solve(oracle, *a, n, L)
            dr = _dev(run, ref, start)
            print("twin %-14s n %d L %2d  step: offset %.2e angle %.2e cost %.2e   run: offset %.2e angle %.2e cost %.2e" %
                  ((name, n, L) + ds + dr))
            assert max(ds) <= STEP_BOUND, (name, n, L, ds)
            assert max(dr) <= RUN_BOUND, (name, n, L, dr)
            worst_step, worst_run = max(worst_step, *ds), max(worst_run, *dr)
            prev = ref[:2]
    print("twin %-14s worst step %.2e (bound %.2e)  worst run %.2e (bound %.2e)" % (name, worst_step, STEP_BOUND, worst_run, RUN_BOUND))


def test_twin_without_preconditioner_is_another_loop(oracle):
    """the `usepreconditioner` switch of the twin: off, PCGInit1 still runs guardedInvert -- on 1.0, so p0 = r / 4 -- and
    PCGStep2 applies 1.0.  The energy (arap_plan.t:10) switches it on; the oracle follows that, not this."""
    case = gn_cases.BY_NAME["tile_bent"]
    a = gn_cases.args(case)
    its = []
    gn_ref.solve(oracle, *a, 1, 3, use_preconditioner=False, iterates=its)
    g, _ = oracle.evalJTF(*a, dtype=np.float64)
    Ag = oracle.applyJTJ(*a[1:], g, dtype=np.float64)
    alpha = float((g * g).sum()) / float((g * Ag).sum())      # (r.p0) / (p0.A p0) with p0 = r / 4, times p0: the /4 cancels
    assert helpers.rel_l2(its[0][0], -alpha * g) <= 1e-12
    ref = oracle.solve(*a, 1, 3, dtype=np.float64)
    assert helpers.rel_l2(its[0][2], _update(ref[0], ref[1], *a[:2])) > 1e-2


@pytest.mark.parametrize("name", NAMES)
def test_pcg_against_direct_solve(oracle, name):
    """first step, L = 1 .. 300, float64 and float32: the energy-norm error against lstsq(J, -F) never rises and ends below
    the recorded floor; on `holes` that is the A-seminorm, and the isolated vertices do not move"""
    case = gn_cases.BY_NAME[name]
    a = gn_cases.args(case)
    d = gn_cases.direct(oracle, case)
    for dtype, bound, kw in ((np.float64, FLOOR64_BOUND, {}), (np.float32, FLOOR32_BOUND, dict(mode=1, trig=1))):
        errs = []
        for L in L_PCG:
            O, A, _ = oracle.solve(*a, 1, L, dtype=dtype, **kw)
            errs.append(d.error_of(O, A))
            if case.shape == "holes":
                for x, y in gn_cases.ISOLATED:
                    assert np.array_equal(O[y, x], a[0][y, x]) and A[y, x] == a[1][y, x]
        print("pcg %-14s %s  " % (name, np.dtype(dtype).name) + " ".join("%.2e" % e for e in errs) + "  bound %.2e" % bound)
        for e0, e1, L in zip(errs, errs[1:], L_PCG[1:]):
            assert e1 <= e0 * (1 + RISE_RELATIVE) + bound, "%s %s: the error rises at L = %d" % (name, np.dtype(dtype).name, L)
        assert errs[0] <= 1.0 and errs[-1] <= bound, (name, errs)      # (delta_0 = 0 has error 1)


@pytest.mark.parametrize("name", [c.name for c in gn_cases.RIGID])
def test_rigid_handles_give_the_rigid_motion(oracle, name):
    case = gn_cases.BY_NAME[name]
    a = gn_cases.args(case, exact=True)
    M = a[4]
    live = (M == 0) & (gn_cases.degree(M == 0) > 0)              # (an isolated vertex has no residual: it stays)
    rm = gn_cases.rigid_map(case)
    O, A, costs = oracle.solve(*a, N_RIGID, L_CONV, dtype=np.float64)
    dO, dA = np.abs(O - rm)[live].max(), np.abs(A - gn_cases.THETA)[live].max()
    print("rigid %-12s float64 costs %s  |Offset - rigid| %.2e  |Angle - 0.3| %.2e" % (name, " ".join("%.2e" % c for c in costs), dO, dA))
    assert np.all(np.diff(costs) < 0)
    assert dO <= RIGID_OFFSET_BOUND and dA <= RIGID_ANGLE_BOUND
    ssq = gn_cases.half_ssq(oracle, case, O, A, exact=True)
    assert abs(costs[-1] - ssq) <= 1e-12 * ssq
    # float32, the handles as float32 holds them: where it stalls
    a32 = gn_cases.args(case)
    O, A, costs = oracle.solve(*a32, N_RIGID, L_CONV, dtype=np.float32, mode=1, trig=1)
    dec = gn_cases.newton_decrement(oracle, case, O, A)
    print("rigid %-12s float32 costs %s  |Offset - rigid| %.2e  |Angle - 0.3| %.2e  decrement %.2e (bound %.2e)" %
          (name, " ".join("%.2e" % c for c in costs), np.abs(O - rm)[live].max(), np.abs(A - gn_cases.THETA)[live].max(), dec, DECREMENT32_BOUND))
    assert dec <= DECREMENT32_BOUND


@pytest.mark.parametrize("name", [c.name for c in gn_cases.BENT])
def test_bent_handles_give_a_stationary_point(oracle, name):
    case = gn_cases.BY_NAME[name]
    a = gn_cases.args(case)
    start = gn_cases.direct(oracle, case).norm                   # the decrement at the start
    O, A, costs = oracle.solve(*a, N_BENT, L_CONV, dtype=np.float64)
    assert costs[-1] > 1e-6                                      # the case's precondition: a minimum with energy
    dec = gn_cases.newton_decrement(oracle, case, O, A)
    ssq = gn_cases.half_ssq(oracle, case, O, A)
    print("bent %-14s float64 cost %.9e  decrement %.2e (start %.2e, bound %.2e)" % (name, costs[-1], dec, start, DECREMENT64_BOUND))
    assert np.all(np.diff(costs) <= 1e-12 * costs[-1])
    assert dec <= DECREMENT64_BOUND
    assert abs(costs[-1] - ssq) <= 1e-12 * ssq
    O, A, costs32 = oracle.solve(*a, N_BENT, L_CONV, dtype=np.float32, mode=1, trig=1)
    dec32 = gn_cases.newton_decrement(oracle, case, O, A)
    print("bent %-14s float32 cost %.9e  decrement %.2e (bound %.2e)" % (name, costs32[-1], dec32, DECREMENT32_BOUND))
    assert dec32 <= DECREMENT32_BOUND


# (d) two small frames for the schedule.  `odd`: a handle on an excluded pixel, two handles with one source (the later one
# wins), a target outside the frame, a target with a negative coordinate (valid only while the ramp keeps it >= 0)
def _frames():
    ys, xs = np.mgrid[0:9, 0:14]
    odd_mask = np.where((xs >= 10) & (ys <= 2), 255, 0).astype(np.uint8)
    odd = [(3, 3, 5, 4), (11, 1, 12, 2), (7, 6, 9, 6), (7, 6, 6, 7), (12, 7, 16, 8), (2, 6, -3, 6)]
    plain = [(2, 2, 3, 3), (8, 2, 7, 3), (2, 7, 3, 6), (8, 7, 9, 8)]
    return [("plain", np.zeros((10, 11), np.uint8), plain, True, (2, 2, 20)), ("odd", odd_mask, odd, True, (3, 2, 15)),
            ("odd_nopins", odd_mask, odd, False, (3, 2, 15))]


@pytest.mark.parametrize("k", range(3))
def test_frame_schedule(oracle, k):
    name, mask, cons, pins, sched = _frames()[k]
    H, W = mask.shape
    allc = list(cons) + (gn_ref.border_pins(W, H) if pins else [])
    if pins:
        assert np.array_equal(np.asarray(gn_ref.border_pins(W, H), np.int32), oracle.border_pins(W, H))
    for i in range(sched[0]):
        alpha = np.float32(i + 1) / np.float32(sched[0])
        mine = gn_ref.constraint_image(mask, allc, alpha)
        assert np.array_equal(mine, oracle.constraint_image(mask, allc, alpha))
        if name.startswith("odd"):
            assert (mine[1, 11] == -1).all() and (mine[6, 7] >= 0).all() and mine[7, 12, 0] > 12
            assert mine[6, 7, 1] == np.float32(6) * (np.float32(1) - alpha) + alpha * np.float32(7)     # the later handle
    if name.startswith("odd"):
        assert mine[6, 2, 0] == -3                                                      # at alpha = 1: invalid, the handle is off
    O, A, finals = oracle.frame(mask, cons, *sched, dtype=np.float64, border_pins=pins)
    O2, A2, finals2 = gn_ref.frame(oracle, mask, cons, *sched, pins=pins)
    grid = np.stack(np.mgrid[0:H, 0:W][::-1], -1).astype(np.float64)
    dev = _dev((O2, A2, finals2), (O, A, finals), (grid, np.zeros((H, W))))
    print("frame %-10s offset %.2e angle %.2e cost %.2e (bound %.2e)" % ((name,) + dev + (RUN_BOUND,)))
    assert np.abs(O - grid).max() > 0.5 and max(dev) <= RUN_BOUND
    ex = mask != 0
    assert np.array_equal(O[ex], grid[ex]) and not A[ex].any()
