"""The HIP Gauss-Newton paths held directly to the plain float64 references of tests/gn_cases.py -- the direct least-squares
solve of the normal equations from a finite-difference Jacobian of the residual definition, the closed form of a translated
frame, the energy at the state returned -- and not to the float32 oracle (that parity is asserted in test_gpu_solve.py and
its neighbours, and is not repeated here).  The bounds are the float32 oracle's own distances from those references, measured
on the CPU (tests/test_gn_host.py) or, for the two frames, computed beside the GPU run, times the margin 4 of float32 there.

Paths: the drop-in plan as it chooses (the resident kernel for a pixel-grid UrShape, the generic-UrShape kernels otherwise),
the kernel-per-phase pair (ArapFlow_SetResident(state, 0)), and that pair with an LDS-tiled phase A (ArapFlow_SetTile 32x8);
the frame solver in a batch of three slots, resident and not.  At these sizes a resident launch is one group of 64
workgroups with at most one tile each (asserted through ArapFlow_ResidentDeal), so `seam` -- 33x9, four tiles -- has its
handles' neighbourhoods and every edge across x = 31 | 32 and y = 7 | 8 in different workgroups."""
import ctypes

import numpy as np
import pytest
import torch

import gn_cases
import gn_ref
from arap_flow_amd import capi, opt
from test_gn_host import DECREMENT32_BOUND, FLOOR32_BOUND, RISE_RELATIVE

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in gn_cases.CASES]
PATHS = ("plan", "pair", "tiled")
L_GPU = (1, 2, 3, 5, 10, 30, 300)
F32_MARGIN = 4


def _set_path(state, path):
    state.set_resident(path == "plan")
    state.set_tile(*((32, 8) if path == "tiled" else (-1, -1)))


@pytest.fixture
def path_state(gpu_state):
    yield gpu_state
    gpu_state.set_tile(-1, -1)
    gpu_state.set_resident(True)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", NAMES)
def test_drop_in_step_against_direct_solve(path_state, oracle, name, path):
    """one Gauss-Newton step of L = 1 .. 300 PCG iterations through Opt_ProblemSolve: the energy-norm error against
    lstsq(J, -F) never rises and at L = 300 is within the float32 floor measured on the oracle; excluded and isolated
    vertices do not move"""
    case = gn_cases.BY_NAME[name]
    d = gn_cases.direct(oracle, case)
    O0, A0, U, C, M, wf, wr = gn_cases.args(case)
    _set_path(path_state, path)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    dev = dict(O=f32(O0).cuda(), A=f32(A0).cuda(), U=f32(U).cuda(), C=f32(C).cuda(), M=f32(M).cuda())
    s = opt.OptSolver(path_state, (case.W, case.H))
    try:
        pp = opt.NamedParameters()
        for n, k in [("Offset", "O"), ("Angle", "A"), ("UrShape", "U"), ("Constraints", "C"), ("Mask", "M")]:
            pp.set(n, dev[k])
        pp.set("w_fitSqrt", wf); pp.set("w_regSqrt", wr)
        errs = []
        for L in L_GPU:
            dev["O"].copy_(f32(O0)); dev["A"].copy_(f32(A0))
            sp = opt.NamedParameters()
            sp.set("nIterations", 1); sp.set("lIterations", L)
            before = s.resident_launches()
            cost = s.solve(sp, pp)
            O, A = dev["O"].cpu().numpy(), dev["A"].cpu().numpy()
            assert (s.resident_launches() > before) == (path == "plan" and case.shape != "generic"), (name, path, L)
            assert np.isfinite(cost) and np.isfinite(O).all() and np.isfinite(A).all()
            ex = M != 0
            assert np.array_equal(O[ex], O0[ex].astype(np.float32)) and np.array_equal(A[ex], A0[ex].astype(np.float32))
            if case.shape == "holes":
                for x, y in gn_cases.ISOLATED:
                    assert np.array_equal(O[y, x], O0[y, x]) and A[y, x] == A0[y, x]
            errs.append(d.error_of(O, A))
    finally:
        s.close()
    print("gpu %-14s %-5s " % (name, path) + " ".join("%.2e" % e for e in errs) + "  bound %.2e" % FLOOR32_BOUND)
    for e0, e1, L in zip(errs, errs[1:], L_GPU[1:]):
        assert e1 <= e0 * (1 + RISE_RELATIVE) + FLOOR32_BOUND, "%s %s: the error rises at L = %d" % (name, path, L)
    assert errs[0] <= 1.0 and errs[-1] <= FLOOR32_BOUND, (name, path, errs)


def test_seam_is_dealt_one_tile_per_workgroup():
    """ArapFlow_ResidentTiles / ArapFlow_ResidentDeal (pure host functions of the library) on the 33x9 full mask: four
    tiles -- origins 0, 32, 8 rows down, and 32 beside that -- and one group of 64 workgroups, of which ranks 0 .. 3 take one
    tile each: the tile borders of `seam` are workgroup borders"""
    lib = capi.load()
    case = gn_cases.BY_NAME["seam_rigid"]
    mask = np.zeros((case.H, case.W), np.uint8)
    org, bx = np.zeros(4608, np.int32), np.zeros((case.H + 7) // 8, np.int32)
    ip = ctypes.POINTER(ctypes.c_int)
    nt = lib.ArapFlow_ResidentTiles(mask.ctypes.data, case.W, case.H, 1, org.ctypes.data_as(ip), 4608, bx.ctypes.data_as(ip))
    assert nt == 4 and org[:4].tolist() == [0, 32, 8 * case.W, 8 * case.W + 32]
    t = np.asarray([nt], np.int32)
    tab = np.full((1, 512, 4), -7, np.int32)
    assert lib.ArapFlow_ResidentDeal(t.ctypes.data_as(ip), 1, tab.ctypes.data_as(ip), 1) == 1
    mine = tab[0][tab[0][:, 0] == 0]
    assert len(mine) == 64 and (mine[:, 2] == 64).all() and sorted(mine[:, 1].tolist()) == list(range(64))
    assert nt <= len(mine)                                                      # nt / wgs = 0, nt % wgs = 4: one tile each


# ---- the frame solver ------------------------------------------------------------------------------------------------

FW, FH = 33, 9
SCHED = (3, 8, 300)                 # ramp steps, Gauss-Newton steps, PCG iterations: long enough to converge at this size
_SRC = [(2, 1), (31, 2), (32, 5), (10, 7), (20, 8), (3, 6)]
_frame_cache = {}


def _frames(oracle):
    """three frames without border pins, and per frame what the float32 oracle leaves of the same input (computed once):
      shift  integer handles that all move by (3, 2): the answer is the translated grid, Angle = 0, energy 0
      bent   the same with two handles moved by 2 px more
      other  `bent`'s handles on another mask (every seventh column cut, but for one row in four)"""
    if not _frame_cache:
        ys, xs = np.mgrid[0:FH, 0:FW]
        full = np.zeros((FH, FW), np.uint8)
        cut = np.where((xs % 7 == 5) & (ys % 4 != 1), 255, 0).astype(np.uint8)
        shift = [(x, y, x + 3, y + 2) for x, y in _SRC]
        bent = [(x, y, x + 3 + (2 if k == 1 else 0), y + 2 - (2 if k == 4 else 0)) for k, (x, y) in enumerate(_SRC)]
        grid = np.stack([xs, ys], -1).astype(np.float64)
        wf, wr = float(np.sqrt(np.float32(100.0))), float(np.sqrt(np.float32(0.01)))
        for name, mask, cons in (("shift", full, shift), ("bent", full, bent), ("other", cut, bent)):
            assert all(mask[y, x] == 0 for x, y, _, _ in cons)
            pb = (grid, gn_ref.constraint_image(mask, cons, 1.0).astype(np.float64), mask.astype(np.float64), wf, wr)
            O, A, costs = oracle.frame(mask, cons, *SCHED, dtype=np.float32, mode=1, trig=1, border_pins=False)
            ssq = gn_cases.half_ssq_at(oracle, *pb, O, A)
            _frame_cache[name] = dict(mask=mask, cons=np.asarray(cons, np.int32), pb=pb, grid=grid, O=O, A=A, cost=costs[-1],
                                      cost_gap=abs(costs[-1] - ssq), decrement=gn_cases.newton_decrement_at(oracle, *pb, O, A))
    return _frame_cache


@pytest.mark.parametrize("resident", [True, False])
def test_frame_solver_against_the_energy(path_state, oracle, resident):
    """float32 oracle on the same input (CPU): shift |Offset - translated grid| 0, |Angle| 4.3e-16, cost 7.2e-32; bent
    decrement 1.72e-5 (float64: 2.97e-6 after the same schedule), |cost - 0.5 |F|^2| / cost 1.0e-8; other 1.89e-5, 6.2e-9"""
    fr = _frames(oracle)
    path_state.set_resident(resident)
    fs = opt.FrameSolver(path_state, FW, FH, batch=3)
    try:
        for b, k in enumerate(("shift", "bent", "other")):
            fs.set_frame(b, fr[k]["mask"], fr[k]["cons"], border_pins=False)
        fs.solve(3, *SCHED)
        res = {k: fs.results(b, want_rgb=False) for b, k in enumerate(("shift", "bent", "other"))}
        assert (fs.stats()["resident_launches"] > 0) == resident
    finally:
        fs.close()
    f = fr["shift"]
    target = f["grid"] + np.array([3.0, 2.0])
    r = res["shift"]
    print("frame shift resident %d: |Offset - translated| %.2e (oracle %.2e)  |Angle| %.2e (oracle %.2e)  cost %.2e (oracle %.2e)" %
          (resident, np.abs(r["offset"] - target).max(), np.abs(f["O"] - target).max(), np.abs(r["angle"]).max(), np.abs(f["A"]).max(),
           r["cost"], f["cost"]))
    assert np.abs(r["offset"] - target).max() <= F32_MARGIN * np.abs(f["O"] - target).max()
    assert np.abs(r["angle"]).max() <= F32_MARGIN * np.abs(f["A"]).max()
    assert 0.0 <= r["cost"] <= F32_MARGIN * f["cost"]
    for k in ("bent", "other"):
        f, r = fr[k], res[k]
        ex = f["mask"] != 0
        assert np.array_equal(r["offset"][ex], f["grid"][ex].astype(np.float32)) and not r["angle"][ex].any()
        ssq = gn_cases.half_ssq_at(oracle, *f["pb"], r["offset"], r["angle"])
        dec = gn_cases.newton_decrement_at(oracle, *f["pb"], r["offset"], r["angle"])
        print("frame %-5s resident %d: cost %.9e  0.5 |F|^2 %.9e (gap %.2e, oracle's %.2e)  decrement %.2e (oracle's %.2e)" %
              (k, resident, r["cost"], ssq, abs(r["cost"] - ssq), f["cost_gap"], dec, f["decrement"]))
        assert ssq > 1e-6 and abs(r["cost"] - ssq) <= F32_MARGIN * f["cost_gap"]
        assert dec <= F32_MARGIN * f["decrement"] and f["decrement"] <= DECREMENT32_BOUND
