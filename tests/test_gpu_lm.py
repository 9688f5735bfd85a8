"""Solver kind "LMGPU" against the float32 CPU restatement (oracle.solve_lm), bit for bit after every step, on the
cases of tests/lm_cases.py: each takes a branch of host_lm.h:plan_step_lm or of the arap_lm.h kernels that
tests/test_lm_host.py shows the oracle taking, or a workgroup count at which block_reduce_fixed<2> changes shape.
The restatement itself is pinned by tests/test_lm_host.py.  DESIGN.md "LM: pins and branches"."""
import numpy as np
import pytest
import torch

import lm_cases
from arap_flow_amd import opt

pytestmark = pytest.mark.gpu

_IMAGES = [("Offset", "O"), ("Angle", "A"), ("UrShape", "U"), ("Constraints", "C"), ("Mask", "M")]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _upload(pb):
    dev = {k: torch.from_numpy(pb[k].copy()).cuda() for k in "OAUCM"}
    pp = opt.NamedParameters()
    for n, k in _IMAGES:
        pp.set(n, dev[k])
    pp.set("w_fitSqrt", lm_cases.WF)
    pp.set("w_regSqrt", lm_cases.WR)
    return dev, pp


def _solver_params(case, L=None, period=None):
    sp = opt.NamedParameters()
    sp.set("nIterations", int(case.n))
    sp.set("lIterations", int(case.L if L is None else L))
    sp.set("residual_reset_period", int(case.period if period is None else period))
    for k, v in case.lm:
        sp.set(k, float(v))
    return sp


def _snap(s, dev, ret):
    return dict(ret=ret, cost=s.current_cost(), O=dev["O"].cpu().numpy(), A=dev["A"].cpu().numpy(), state=s.lm_state())


def _drive(s, case, dev, pp, sp):
    """Init, then case.n Steps and one more: the snapshot after Init and after every Step"""
    s.set_solver_parameters(sp)
    s.init(pp)
    recs = [_snap(s, dev, None)]
    for _ in range(case.n + 1):
        recs.append(_snap(s, dev, s.step(pp)))
    return recs


def _gpu_run(gpu_state, case):
    dev, pp = _upload(lm_cases.problem(case))
    s = opt.OptSolver(gpu_state, (case.W, case.H), opt.BUILTIN_PLAN, b"LMGPU")
    try:
        return _drive(s, case, dev, pp, _solver_params(case))
    finally:
        s.close()


def _same_records(a, b):
    return len(a) == len(b) and all(
        x["ret"] == y["ret"] and x["cost"] == y["cost"] and np.array_equal(_bits(x["O"]), _bits(y["O"])) and
        np.array_equal(_bits(x["A"]), _bits(y["A"])) and x["state"] == y["state"] for x, y in zip(a, b))


def _check_against_oracle(oracle, case, recs):
    pb = lm_cases.problem(case)
    ex = pb["M"] != 0
    full = lm_cases.oracle_run(oracle, case)
    assert recs[0]["cost"] == float(np.float32(full["costs"][0])) and recs[0]["state"]["outcome"] is None
    steps = [case.n] if case.final_only else range(1, case.n + 1)
    for k in steps:
        ref, got = lm_cases.oracle_run(oracle, case, k), recs[k]
        what = "%s after Step %d" % (case.name, k)
        assert got["ret"] == int(ref["steps"] == k), what
        assert got["cost"] == float(np.float32(ref["costs"][-1])), what
        nO, nA = int((_bits(got["O"]) != _bits(ref["O"])).sum()), int((_bits(got["A"]) != _bits(ref["A"])).sum())
        assert nO == 0 and nA == 0, "%s: %d Offset and %d Angle floats differ" % (what, nO, nA)
        assert np.array_equal(_bits(got["O"][ex]), _bits(pb["O"][ex])) and np.array_equal(_bits(got["A"][ex]), _bits(pb["A"][ex])), what
        last = ref["trace"][-1]
        want = dict(radius=np.float32(last["radius"]), decrease=np.float32(last["decrease"]),
                    pcg_iterations=last["pcg_iterations"], outcome=last["outcome"])
        assert got["state"] == want, "%s: %s, oracle %s" % (what, got["state"], want)
    # one Step more than nIterations: returns 0, attempts nothing
    end, extra = recs[case.n], recs[case.n + 1]
    assert extra["ret"] == 0 and _same_records([dict(end, ret=0)], [extra])
    assert end["state"]["radius"] == np.float32(full["radius"])


@pytest.mark.parametrize("name", [c.name for c in lm_cases.GPU_CASES])
def test_lm_steps_equal_oracle_bits(gpu_state, oracle, name):
    """Opt_ProblemInit, then Step by Step: return value, cost, every Offset and Angle float, the excluded vertices'
    input bits and ArapFlow_LMState equal the oracle run with nIterations = k; and a second run gives the same bytes."""
    case = lm_cases.BY_NAME[name]
    first = _gpu_run(gpu_state, case)
    _check_against_oracle(oracle, case, first)
    assert _same_records(first, _gpu_run(gpu_state, case)), "%s: a second run differs from the first" % name


def test_lm_plan_life_cycle(gpu_state, oracle):
    """One plan: a solve with L=12, Init again with L=40 (the per-iteration Q slots regrow, and the first step must save
    SSq again), then with L=5.  Each solve equals a fresh plan's, and the oracle's, bit for bit."""
    base = lm_cases.BY_NAME["period_3"]
    pb = lm_cases.problem(base)
    dev, pp = _upload(pb)
    s = opt.OptSolver(gpu_state, (base.W, base.H), opt.BUILTIN_PLAN, b"LMGPU")
    try:
        for L in (12, 40, 5):
            case = lm_cases.derive(base, "_L%d" % L, L=L)
            dev["O"].copy_(torch.from_numpy(pb["O"].copy()))
            dev["A"].copy_(torch.from_numpy(pb["A"].copy()))
            recs = _drive(s, case, dev, pp, _solver_params(case))
            assert _same_records(recs, _gpu_run(gpu_state, case)), "L=%d on the reused plan differs from a fresh plan" % L
            _check_against_oracle(oracle, case, recs)
    finally:
        s.close()


def test_lm_and_gauss_newton_plans_side_by_side(gpu_state):
    """An LM plan and a Gauss-Newton plan alive on one state, stepped alternately, each on its own images: each equals
    its solo run, and the LM plan never takes the resident kernel, which the Gauss-Newton plan is free to take."""
    case = lm_cases.BY_NAME["defaults_grid"]
    pb = lm_cases.problem(case)
    gpu_state.set_resident(True)

    def gn_params():
        sp = opt.NamedParameters()
        sp.set("nIterations", int(case.n))
        sp.set("lIterations", int(case.L))
        return sp

    def gn_snap(s, dev, ret):
        return dict(ret=ret, cost=s.current_cost(), O=dev["O"].cpu().numpy(), A=dev["A"].cpu().numpy(), state=None)

    dev, pp = _upload(pb)
    solo = opt.OptSolver(gpu_state, (case.W, case.H))
    solo.set_solver_parameters(gn_params())
    solo.init(pp)
    gn_solo = [gn_snap(solo, dev, None)] + [gn_snap(solo, dev, solo.step(pp)) for _ in range(case.n + 1)]
    solo.close()
    lm_solo = _gpu_run(gpu_state, case)

    dev_l, pp_l = _upload(pb)
    dev_g, pp_g = _upload(pb)
    lm = opt.OptSolver(gpu_state, (case.W, case.H), opt.BUILTIN_PLAN, b"LMGPU")
    gn = opt.OptSolver(gpu_state, (case.W, case.H))
    try:
        lm.set_solver_parameters(_solver_params(case))
        gn.set_solver_parameters(gn_params())
        lm.init(pp_l)
        gn.init(pp_g)
        lm_recs, gn_recs = [_snap(lm, dev_l, None)], [gn_snap(gn, dev_g, None)]
        for _ in range(case.n + 1):
            lm_recs.append(_snap(lm, dev_l, lm.step(pp_l)))
            gn_recs.append(gn_snap(gn, dev_g, gn.step(pp_g)))
        assert _same_records(lm_recs, lm_solo), "the LM plan beside a Gauss-Newton plan differs from its solo run"
        assert _same_records(gn_recs, gn_solo), "the Gauss-Newton plan beside an LM plan differs from its solo run"
        assert [r["ret"] for r in gn_recs[1:]] == [1] * case.n + [0]
        assert lm.resident_launches() == 0
        with pytest.raises(ValueError):
            gn.lm_state()
    finally:
        lm.close()
        gn.close()


def test_residual_reset_period_below_one_is_not_stored(gpu_state, oracle):
    """Opt_SetSolverParameter keeps the plan's previous residual_reset_period for a value below 1 (the step takes the
    PCG iteration number modulo it): 0 on a fresh plan gives the default period's result, -1 after 3 gives period 3's."""
    base = lm_cases.BY_NAME["never_breaks"]                      # all 25 iterations run: period 10 resets at 10 and 20
    assert base.period == 10 and lm_cases.oracle_run(oracle, base)["trace"][0]["resets"] == 2
    pb = lm_cases.problem(base)
    for first, then, want in ((None, 0, 10), (3, -1, 3)):
        case = lm_cases.derive(base, "_p%d" % want, period=want)
        dev, pp = _upload(pb)
        s = opt.OptSolver(gpu_state, (case.W, case.H), opt.BUILTIN_PLAN, b"LMGPU")
        try:
            if first is not None:
                s.set_solver_parameters(_solver_params(case, period=first))
            recs = _drive(s, case, dev, pp, _solver_params(case, period=then))
        finally:
            s.close()
        _check_against_oracle(oracle, case, recs)
    p3 = lm_cases.oracle_run(oracle, lm_cases.derive(base, "_p3", period=3))
    assert not np.array_equal(p3["O"], lm_cases.oracle_run(oracle, base)["O"])      # the period matters on this case
