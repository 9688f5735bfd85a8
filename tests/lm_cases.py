"""The cases of the "LMGPU" tests, in one place: tests/test_lm_host.py (CPU: the float64 twin against the oracle, and
the census of the branches the float32 oracle takes on each case) and tests/test_gpu_lm.py (GPU: bit equality with the
float32 oracle per step) read the same list, so a case cannot be compared on the GPU for a branch it no longer takes.

A case's `labels` name the branches it was written for; BRANCHES holds, per name, the predicate on the oracle's trace
(oracle.solve_lm(trace=...)) that says the branch was taken.  DESIGN.md "LM: pins and branches" has the table."""
import collections

import numpy as np

import helpers

WF, WR = 10.0, 0.1
TIE_TOLERANCE = 0.9997093081474304

Case = collections.namedtuple("Case", "name W H seed ncons generic n L period lm mask labels final_only")


def _case(name, W=65, H=5, seed=200, ncons=6, generic=True, n=6, L=25, period=10, lm=None, mask=None, labels=(),
          final_only=False):
    return Case(name, W, H, seed, ncons, generic, n, L, period, tuple(sorted((lm or {}).items())), mask, tuple(labels),
                final_only)


# The parameter rows at 65x5 (two partial 64x4 blocks each way), generic UrShape.  A period the row does not name is
# 100: no PCG loop here runs 100 iterations, so those cases take no residual reset at all.
_ROWS = [
    _case("defaults", period=10, labels=("zeta_break", "accept", "reject", "clamp_low_isolated", "arm_third", "arm_tmp")),
    _case("function_tolerance", period=100, lm=dict(function_tolerance=0.9), labels=("function_tolerance", "no_reset")),
    # the float32 function tolerance at which step 1 of `defaults` meets cost_change == prevCost * function_tolerance exactly
    # (tests/test_lm_host.py checks the equality): the exit is taken with <=, not with <
    _case("function_tolerance_tie", n=2, period=100, lm=dict(function_tolerance=TIE_TOLERANCE), labels=("function_tolerance_first_step",)),
    _case("all_rejected", n=8, period=100, lm=dict(min_relative_decrease=2.0, min_trust_region_radius=100.0),
          labels=("min_radius", "nothing_moves")),
    _case("radius_cap", n=4, period=100, lm=dict(max_trust_region_radius=2e4), labels=("radius_cap",)),
    _case("clamp_low", period=100, lm=dict(min_lm_diagonal=0.5), labels=("clamp_low",)),
    _case("clamp_high", period=100, lm=dict(max_lm_diagonal=0.01), labels=("clamp_high",)),
    _case("q_tolerance_half", n=3, period=100, lm=dict(q_tolerance=0.5), labels=("zeta_break", "no_reset")),
    _case("never_breaks", n=3, period=10, lm=dict(q_tolerance=-1e30), labels=("full_pcg", "reset")),
    _case("never_breaks_no_reset", n=3, period=100, lm=dict(q_tolerance=-1e30), labels=("full_pcg", "no_reset")),
    _case("period_1", n=3, L=12, period=1, labels=("every_iteration_resets",)),
    _case("period_3", n=3, L=12, period=3, labels=("reset_other_period", "break_on_reset")),
    _case("no_pcg", n=3, L=0, labels=("nan_reject", "nothing_moves")),
    _case("all_excluded", n=3, mask="all", labels=("nan_reject", "nothing_moves")),
    _case("small_radius", n=3, period=100, lm=dict(trust_region_radius=1e-3), labels=("accept",)),
    _case("large_radius", n=3, period=100, lm=dict(trust_region_radius=1e12), labels=("accept",)),
]

# the same rows with a pixel-grid UrShape: another trajectory, so no branch is claimed for them
_GRID_ROWS = [c._replace(name=c.name + "_grid", generic=False, labels=()) for c in _ROWS]

# shapes at the defaults: the smallest at which each thing can go wrong (64x4 vertices per workgroup; a reduction
# group is the workgroups that share one of the 32 shards)
_SHAPES = [
    _case("1x1", W=1, H=1, seed=4, ncons=1, n=4, labels=("active",)),
    _case("1x9", W=1, H=9, seed=201, ncons=2, n=4, labels=("active",)),
    _case("9x1", W=9, H=1, seed=202, ncons=2, n=4, labels=("active",)),
    _case("64x4", W=64, H=4, seed=203, ncons=6, n=4, labels=("active",)),                   # exactly one block
    _case("130x37", W=130, H=37, seed=204, ncons=96, n=4, labels=("active",)),              # 30 workgroups, full-width blocks
    _case("3x128", W=3, H=128, seed=205, ncons=8, n=3, L=12, period=3, labels=("reset_other_period",)),     # 32 workgroups
    _case("3x129", W=3, H=129, seed=206, ncons=8, n=3, L=12, period=3, labels=("reset_other_period",)),     # 33: group 0 has two members
    _case("3x8196", W=3, H=8196, seed=207, ncons=400, n=3, L=12, period=3, labels=("reset_other_period",), final_only=True),  # 2049
]

# whole 64x4 tiles without an active vertex (columns 0-63, rows 4-7) next to active ones
_TILES = [_case("excluded_tiles", W=192, H=12, seed=208, ncons=24, n=4, mask="tiles", labels=("empty_tiles", "accept"))]

GPU_CASES = _ROWS + _GRID_ROWS + _SHAPES + _TILES
BY_NAME = {c.name: c for c in GPU_CASES}
assert len(BY_NAME) == len(GPU_CASES)

# the 16 cases of the float64 twin against oracle.solve_lm(dtype=float64)
TWIN_CASES = [BY_NAME[k] for k in ("defaults", "defaults_grid", "period_1", "period_3", "function_tolerance", "all_rejected",
                                   "radius_cap", "clamp_low", "clamp_high", "q_tolerance_half", "never_breaks",
                                   "small_radius", "large_radius", "64x4")] + \
             [_case("33x9", W=33, H=9, seed=209, ncons=6, n=4), _case("130x37_L40", W=130, H=37, seed=204, ncons=96, n=6, L=40)]

_PROBLEMS = {}


def problem(case):
    """the case's frame (cached; do not modify): helpers.random_problem, then the case's mask"""
    if case.name not in _PROBLEMS:
        pb = helpers.random_problem(case.W, case.H, seed=case.seed, generic_urshape=case.generic, ncons=case.ncons)
        if case.mask == "all":
            pb["M"][:] = 255.0
        elif case.mask == "tiles":
            pb["M"][:, :64] = 255.0
            pb["M"][4:8, :] = 255.0
        for a in pb.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _PROBLEMS[case.name] = pb
    return _PROBLEMS[case.name]


def derive(case, suffix, **changes):
    """a variant of a case on the same frame (another L, another period), under its own name"""
    new = case._replace(name=case.name + suffix, labels=(), **changes)
    _PROBLEMS[new.name] = problem(case)
    return new


_RUNS = {}


def oracle_run(orc, case, k=None, dtype=np.float32):
    """oracle.solve_lm on the case with nIterations = k (default: the case's n), cached:
    dict(O, A, costs, steps, radius, trace)"""
    k = case.n if k is None else k
    key = (case.name, k, np.dtype(dtype).name)
    if key not in _RUNS:
        pb, trace = problem(case), []
        O, A, costs, steps, radius = orc.solve_lm(pb["O"], pb["A"], pb["U"], pb["C"], pb["M"], WF, WR, k, case.L,
                                                  residual_reset_period=case.period, dtype=dtype, trace=trace, **dict(case.lm))
        _RUNS[key] = dict(O=O, A=A, costs=costs, steps=steps, radius=radius, trace=trace)
    return _RUNS[key]


def _moved(case, run):
    pb = problem(case)
    return not (np.array_equal(run["O"], pb["O"]) and np.array_equal(run["A"], pb["A"]))


def _isolated(case):
    """active vertices without an active neighbour and without a constraint: the zero rows of J^T J"""
    pb = problem(case)
    act = np.pad(pb["M"] == 0, 1)
    nb = act[1:-1, 2:] | act[1:-1, :-2] | act[2:, 1:-1] | act[:-2, 1:-1]
    fit = (pb["C"] >= 0).all(-1)
    return int((act[1:-1, 1:-1] & ~nb & ~fit).sum())


def _tile_active(case):
    M = problem(case)["M"]
    H, W = M.shape
    return [[bool((M[y:y + 4, x:x + 64] == 0).any()) for x in range(0, W, 64)] for y in range(0, H, 4)]


# name -> predicate(case, run): did the float32 oracle take this branch on this case
BRANCHES = {
    "zeta_break": lambda c, r: any(t["pcg_iterations"] < c.L for t in r["trace"]),
    "full_pcg": lambda c, r: c.L > 0 and all(t["pcg_iterations"] == c.L for t in r["trace"]),
    "accept": lambda c, r: any(t["outcome"] == "accepted" for t in r["trace"]),
    "reject": lambda c, r: any(t["outcome"] == "rejected" for t in r["trace"]) and r["trace"][-1]["outcome"] == "accepted",
    "function_tolerance": lambda c, r: r["trace"][-1]["outcome"] == "function_tolerance" and r["steps"] == len(r["trace"]) - 1
                                       and _moved(c, r),
    "function_tolerance_first_step": lambda c, r: [t["outcome"] for t in r["trace"]] == ["function_tolerance"] and r["steps"] == 0
                                                  and _moved(c, r),
    "min_radius": lambda c, r: r["trace"][-1]["outcome"] == "min_radius" and r["steps"] == len(r["trace"]) - 1
                               and r["radius"] <= dict(c.lm)["min_trust_region_radius"],
    "radius_cap": lambda c, r: any(t["outcome"] == "accepted" and t["radius"] == float(np.float32(dict(c.lm)["max_trust_region_radius"]))
                                   for t in r["trace"]),
    # at the defaults the lower clamp is what keeps 1 / CtC finite on the zero diagonal of an active vertex with no active
    # neighbour and no constraint (3 entries each), and the upper clamp takes nothing
    "clamp_low_isolated": lambda c, r: all(t["clamped_low"] == 3 * _isolated(c) > 0 and t["clamped_high"] == 0 for t in r["trace"]),
    "clamp_low": lambda c, r: all(t["clamped_low"] > 3 * _isolated(c) for t in r["trace"]),
    "clamp_high": lambda c, r: all(t["clamped_high"] > 0 for t in r["trace"]),
    "reset": lambda c, r: any(t["resets"] > 0 for t in r["trace"]),
    "reset_other_period": lambda c, r: c.period != 10 and any(t["resets"] > 0 for t in r["trace"]),
    "no_reset": lambda c, r: all(t["resets"] == 0 for t in r["trace"]),
    "every_iteration_resets": lambda c, r: c.period == 1 and all(t["resets"] == t["pcg_iterations"] > 0 for t in r["trace"]),
    "break_on_reset": lambda c, r: any(0 < t["pcg_iterations"] < c.L and t["pcg_iterations"] % c.period == 0 for t in r["trace"]),
    "nan_reject": lambda c, r: len(r["trace"]) == c.n and all(t["outcome"] == "rejected" for t in r["trace"])
                               and r["radius"] < dict(c.lm).get("trust_region_radius", 1e4),
    "nothing_moves": lambda c, r: not _moved(c, r) and len(set(r["costs"].tolist())) == 1,
    "arm_third": lambda c, r: any(t["arm"] == "third" for t in r["trace"]),
    "arm_tmp": lambda c, r: any(t["arm"] == "tmp" for t in r["trace"]),
    "active": lambda c, r: bool((problem(c)["M"] == 0).any()) and _moved(c, r),
    "empty_tiles": lambda c, r: (lambda ta: not ta[1][0] and not ta[0][0] and not ta[1][1] and ta[0][1] and ta[2][2])(_tile_active(c)),
}

# every branch the issue's table names must be taken by at least one labelled case
REQUIRED = ("function_tolerance_first_step", "zeta_break", "full_pcg", "accept", "reject", "function_tolerance", "min_radius", "radius_cap", "clamp_low",
            "clamp_low_isolated", "clamp_high", "reset", "reset_other_period", "break_on_reset", "every_iteration_resets", "nan_reject", "nothing_moves", "arm_third",
            "arm_tmp", "no_reset", "empty_tiles")
