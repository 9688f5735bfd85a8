"""The "LMGPU" restatement (oracle.solve_lm) pinned on the CPU, and the branch census of the LM cases.

The reference holds no LM output, so oracle.solve_lm cannot be compared with the reference.  It is compared with
tests/lm_ref.py instead: a float64 loop in plain numpy, written from the reference's solver source and standing only on
oracle.evalJTF / applyJTJ / cost, which tests/test_oracle.py pins by finite differences.  DESIGN.md "LM: pins and
branches" has the measured values behind TWIN_BOUND."""
import numpy as np
import pytest

import helpers
import lm_cases
import lm_ref

# Twin against oracle.solve_lm(dtype=float64): summation order is the only difference between the two sides.  Worst
# value measured over the 16 cases: 3.71e-12 (rel-L2 of the Angle update, 130x37 with L=40: six steps of up to 40 PCG
# iterations amplify the 1e-16 of a sum; offsets 5.7e-13, costs 5.2e-14, radius 2.1e-13).  The bound is 20x that, which
# leaves room for another seed or another pairwise order inside numpy's sum, and it may never be looser than 1e-6: a slip
# into float32 anywhere in the restatement would show as 1e-7 or more.
TWIN_BOUND = 7.5e-11
assert TWIN_BOUND <= 1e-6


def _args(pb):
    return pb["O"], pb["A"], pb["U"], pb["C"], pb["M"], lm_cases.WF, lm_cases.WR


def test_quadratic_identity_ingredients(oracle):
    """What lm_ref.model_cost stands on: g . d is the directional derivative of oracle.cost (central difference), J^T J is
    symmetric, and for a step that leaves the angles alone -- where the residuals are linear -- the identity
    0.5 |F|^2 + g . d + 0.5 d . (J^T J d) IS oracle.cost at the stepped point."""
    case = lm_cases.BY_NAME["defaults"]
    pb = lm_cases.problem(case)
    O, A, U, Cn, M, wf, wr = [np.array(a, np.float64) for a in _args(pb)]
    rng = np.random.default_rng(1)
    act = (M == 0)[..., None]
    d = np.where(act, rng.normal(size=A.shape + (3,)), 0.0)
    e = np.where(act, rng.normal(size=A.shape + (3,)), 0.0)
    g, _ = oracle.evalJTF(O, A, U, Cn, M, wf, wr, dtype=np.float64)
    cost = lambda t, v: oracle.cost(O + t * v[..., :2], A + t * v[..., 2], U, Cn, M, wf, wr, dtype=np.float64)
    # central difference, h = 1e-5: truncation h^2 / 6 * |third derivative| ~ 1e-10 relative, rounding eps * cost / h ~ 1e-11
    h = 1e-5
    fd = (cost(h, d) - cost(-h, d)) / (2 * h)
    gd = float((g * d).sum())
    print("g.d %.12g, central difference %.12g, relative difference %.3g" % (gd, fd, abs(fd - gd) / abs(gd)))
    assert abs(fd - gd) <= 1e-8 * abs(gd)
    Jd = oracle.applyJTJ(A, U, Cn, M, wf, wr, d, dtype=np.float64)
    Je = oracle.applyJTJ(A, U, Cn, M, wf, wr, e, dtype=np.float64)
    eJd, dJe = float((e * Jd).sum()), float((d * Je).sum())
    print("e.(JtJ d) %.15g, d.(JtJ e) %.15g" % (eJd, dJe))
    assert abs(eJd - dJe) <= 1e-12 * abs(eJd)
    assert float((d * Jd).sum()) > 0
    dO = d.copy()
    dO[..., 2] = 0.0
    model = lm_ref.model_cost(oracle, O, A, U, Cn, M, wf, wr, dO)
    true = cost(1.0, dO)
    print("model cost %.15g, cost at the stepped point %.15g" % (model, true))
    assert abs(model - true) <= 1e-12 * true


def test_twin_vs_oracle_float64(oracle):
    """16 cases: equal outcome sequences, updates / costs / radius within TWIN_BOUND"""
    worst = dict(offset=0.0, angle=0.0, cost=0.0, radius=0.0)
    where = dict(worst)
    for case in lm_cases.TWIN_CASES:
        pb = lm_cases.problem(case)
        ref = lm_cases.oracle_run(oracle, case, dtype=np.float64)
        O, A, costs, steps, radius, recs = lm_ref.solve_lm(oracle, *_args(pb), case.n, case.L,
                                                            residual_reset_period=case.period, **dict(case.lm))
        assert [r["outcome"] for r in recs] == [t["outcome"] for t in ref["trace"]], case.name
        assert [r["pcg_iterations"] for r in recs] == [t["pcg_iterations"] for t in ref["trace"]], case.name
        assert steps == ref["steps"] and len(costs) == len(ref["costs"]), case.name
        rel = lambda a, b: float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(b))))
        got = dict(offset=helpers.rel_l2(O - pb["O"], ref["O"] - pb["O"]), angle=helpers.rel_l2(A - pb["A"], ref["A"] - pb["A"]),
                   cost=rel(costs, ref["costs"]),
                   radius=max(rel([r["radius"] for r in recs], [t["radius"] for t in ref["trace"]]), rel(radius, ref["radius"])))
        assert [r["decrease"] for r in recs] == [t["decrease"] for t in ref["trace"]], case.name
        print("twin %-20s " % case.name + "  ".join("%s %.2e" % kv for kv in got.items()))
        for k, v in got.items():
            if v > worst[k]:
                worst[k], where[k] = v, case.name
    print("twin vs oracle.solve_lm(float64), worst of %d cases: " % len(lm_cases.TWIN_CASES) +
          "  ".join("%s %.2e (%s)" % (k, worst[k], where[k]) for k in worst) + "  bound %.1e" % TWIN_BOUND)
    assert len(lm_cases.TWIN_CASES) == 16
    assert all(v <= TWIN_BOUND for v in worst.values()), worst


def test_branch_census(oracle):
    """On the float32 oracle's trace alone: every labelled case takes its branches, every branch has a case, all finite"""
    taken = {}
    for case in lm_cases.GPU_CASES:
        run = lm_cases.oracle_run(oracle, case)
        assert np.isfinite(run["O"]).all() and np.isfinite(run["A"]).all() and np.isfinite(run["costs"]).all(), case.name
        assert np.isfinite([t["radius"] for t in run["trace"]]).all() and len(run["trace"]) >= 1, case.name
        for label in case.labels:
            assert lm_cases.BRANCHES[label](case, run), "%s no longer takes '%s': %s" % (case.name, label, run["trace"])
            taken.setdefault(label, []).append(case.name)
        print("census %-26s %s" % (case.name, " ".join("%d/%d%s" % (t["pcg_iterations"], t["resets"], t["outcome"][0].upper())
                                                          for t in run["trace"])))
    for label in sorted(taken):
        print("branch %-24s %s" % (label, ", ".join(taken[label])))
    assert not set(lm_cases.REQUIRED) - set(taken), set(lm_cases.REQUIRED) - set(taken)


def test_branch_rows_match_the_probe_table(oracle):
    """the step sequences the parameter rows were written down with (issue table)"""
    seq = lambda name: [(t["pcg_iterations"], t["outcome"]) for t in lm_cases.oracle_run(oracle, lm_cases.BY_NAME[name])["trace"]]
    A, R = "accepted", "rejected"
    assert seq("defaults") == [(6, A), (25, R), (25, R), (25, R), (25, A), (25, A)]
    run = lm_cases.oracle_run(oracle, lm_cases.BY_NAME["function_tolerance"])
    assert run["steps"] == 4 and len(run["trace"]) == 5 and len(run["costs"]) == 5
    assert [t["radius"] for t in lm_cases.oracle_run(oracle, lm_cases.BY_NAME["all_rejected"])["trace"]] == [5e3, 1250.0, 156.25, 9.765625]
    assert lm_cases.oracle_run(oracle, lm_cases.BY_NAME["radius_cap"])["radius"] == 312.5
    assert [n for n, _ in seq("q_tolerance_half")] == [2, 4, 2]
    assert seq("period_3")[0] == (6, A)


def test_function_tolerance_tie_is_exact(oracle):
    """lm_cases.TIE_TOLERANCE is a float32 at which the first step's cost_change EQUALS prevCost * function_tolerance in
    float32: that step exits with <= and would go on with <; one float32 lower it goes on either way."""
    base = lm_cases.BY_NAME["defaults"]
    costs = lm_cases.oracle_run(oracle, base, 1)["costs"]
    prev, new = np.float32(costs[0]), np.float32(costs[1])
    tol = np.float32(lm_cases.TIE_TOLERANCE)
    assert float(tol) == lm_cases.TIE_TOLERANCE and np.float32(prev - new) == np.float32(prev * tol)
    tie = lm_cases.oracle_run(oracle, lm_cases.BY_NAME["function_tolerance_tie"])
    assert [t["outcome"] for t in tie["trace"]] == ["function_tolerance"]
    below = lm_cases.derive(base, "_below_tie", n=2, period=100, lm=(("function_tolerance", float(np.nextafter(tol, np.float32(0)))),))
    assert lm_cases.oracle_run(oracle, below)["trace"][0]["outcome"] == "accepted"


def test_trace_is_optional_and_period_is_checked(oracle):
    case = lm_cases.BY_NAME["defaults"]
    pb = lm_cases.problem(case)
    a = oracle.solve_lm(*_args(pb), case.n, case.L)
    b = lm_cases.oracle_run(oracle, case)
    assert np.array_equal(a[0], b["O"]) and np.array_equal(a[1], b["A"]) and np.array_equal(a[2], b["costs"])
    assert a[3] == b["steps"] and a[4] == b["radius"] == b["trace"][-1]["radius"]
    for period in (0, -3):
        with pytest.raises(ValueError):
            oracle.solve_lm(*_args(pb), case.n, case.L, residual_reset_period=period)
