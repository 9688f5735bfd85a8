"""Host-side mirror of the reference's C++ driver layer, over the C ABI of libarapopt.so.

  OptSolver        ARAP/shared/OptSolver.h:43-91        (Opt_NewState/ProblemDefine/ProblemPlan, solve)
  NamedParameters  ARAP/shared/NamedParameters.h:34-87  (name -> pointer table, insertion order = void**)
  CombinedSolver   ARAP/deformation/src/CombinedSolver.h:99-390 + ARAP/shared/CombinedSolverBase.h:23-120
                   (the reference's own host loop: ramp on the host, one Opt_ProblemSolve per ramp step)
  FrameSolver      the device-resident batched counterpart (ArapFlow_Solver*, include/arap_opt.h part 2)
  warp_image       ARAP/warping/src/main.cpp:145-225 through ArapFlow_Warp
  warp_image_ex    the same, plus backward flow and occlusion maps (ArapFlow_WarpEx)
  warp_step        the warp of one deformation state and the flow from it to a second one (ArapFlow_WarpStep)
  background       full-frame RGB, flow and occlusion behind a warped pair's objects (ArapFlow_Background)
  background_seq   the same over frame 1, a pair's in-between frames and frame 2 in one call (ArapFlow_BackgroundSeq)
  warp_diag        fold diagnostics of a flow: mesh statistics and the fold map (ArapFlow_WarpDiag)
  seg_maps         object index maps, motion boundaries and boundary distance of a pair (ArapFlow_SegMaps)
  flow_score       the Sintel / KITTI error table of an estimated flow against a pair (ArapFlow_FlowScore)
  frame_score      the PSNR / integer-SSIM table of estimated frames (ArapFlow_FrameScore)
  label_score      the DAVIS J / F counts of estimated label maps per object (ArapFlow_LabelScore)
  map_score        the precision / recall counts of estimated occlusion / boundary maps (ArapFlow_MapScore)
  track_score      the TAP-Vid table of estimated tracks against a track file's (ArapFlow_TrackScore)
  chain_flows      estimated tracks from per-link flow estimates (ArapFlow_ChainFlows)
  interp_frames    estimated in-between frames from a flow estimate, by splatting (ArapFlow_InterpFrames)
  augment_pairs    a training batch: B pairs augmented, cropped and normalised on the device (ArapFlow_AugmentPairs)
  augment_clips    a batch of training clips: T frames, L flow links and P point tracks each (ArapFlow_AugmentClips)

torch is used only to own device memory (tensor.data_ptr()) and streams.
"""
import collections
import ctypes as C
import math

import numpy as np
import torch

from . import capi
# the rows and fields of the score tables, in their order (LSCORE_FIELDS: the 8 of a label row as the table holds it)
from .scores import (SCORE_ROWS, SCORE_FIELDS, FSCORE_ROWS, FSCORE_FIELDS, TSCORE_CLASSES, TSCORE_FIELDS,        # noqa: F401
                     LSCORE_TABLE_FIELDS as LSCORE_FIELDS, LSCORE_FRAME_FIELDS, MSCORE_MAX_THR)

BUILTIN_PLAN = b"builtin:arap"
LM_OUTCOMES = ("accepted", "rejected", "function_tolerance", "min_radius")      # ARAPFLOW_LM_* of include/arap_opt.h


def _dev_ptr(t):
    assert t.is_cuda and t.is_contiguous()
    return C.c_void_p(t.data_ptr())


def _host_ptr(a):
    """the pointer of a host array, or NULL for None"""
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _view(ptr, ctype, shape):
    """numpy view (no copy) of the memory a c_void_p points to, None for NULL"""
    if not ptr.value:
        return None
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(int(np.prod(shape)),)).reshape(shape)


class State:
    """Opt_State (Opt.h:35).  One per process/device; shared by solvers."""

    def __init__(self, verbosity=0, timing=False):
        self.lib = capi.load()
        if not torch.cuda.is_available():
            raise RuntimeError("no GPU: libarapopt has no CPU path")
        torch.cuda.init()
        torch.zeros(1, device="cuda")  # make sure the primary context of the current device exists
        ip = capi.Opt_InitializationParameters(0, int(verbosity), int(bool(timing)), 0)
        self.handle = self.lib.Opt_NewState(ip)
        if not self.handle:
            raise RuntimeError("Opt_NewState failed")

    def use_own_stream(self):
        """non-blocking compute stream owned by the library (hosts that overlap copies with solves)"""
        self.lib.ArapFlow_UseOwnStream(self.handle)

    def set_stream(self, stream=None):
        self.lib.ArapFlow_SetStream(self.handle, C.c_void_p(stream.cuda_stream if stream is not None else 0))

    def timer_begin(self):
        self.lib.ArapFlow_TimerBegin(self.handle)

    def timer_end(self):
        return float(self.lib.ArapFlow_TimerEnd(self.handle))

    def set_resident(self, on):
        """allow (default) / forbid the on-chip resident PCG kernel of the frame solver"""
        self.lib.ArapFlow_SetResident(self.handle, int(bool(on)))

    def set_tile(self, tx, ty):
        """phase-A variant of the two-kernel path: (0, 0) direct loads, or an LDS tile shape"""
        if self.lib.ArapFlow_SetTile(self.handle, int(tx), int(ty)) != 0:
            raise ValueError("unsupported tile %dx%d" % (tx, ty))

    def set_kernel_timing(self, on):
        self.lib.ArapFlow_SetKernelTiming(self.handle, int(bool(on)))

    def kernel_time(self, name):
        """(total_ms, launches) of the named kernel since timing was switched on, or None"""
        t, n = C.c_double(), C.c_uint64()
        if self.lib.ArapFlow_KernelTime(self.handle, name.encode(), C.byref(t), C.byref(n)) != 0:
            return None
        return t.value, n.value

    def close(self):
        if self.handle:
            self.lib.ArapFlow_FreeState(self.handle)
            self.handle = None


class NamedParameters:
    """NamedParameters.h:34-87: ordered name -> value table; data() is the void** of the C API.
    Device images are torch CUDA tensors; scalars are kept in host ctypes floats/ints."""

    def __init__(self):
        self._names, self._vals, self._keep = [], [], []

    def set(self, name, value):
        if isinstance(value, torch.Tensor):
            holder, ptr = value, C.c_void_p(value.data_ptr())
        elif isinstance(value, int):
            holder = C.c_int(value)
            ptr = C.cast(C.pointer(holder), C.c_void_p)
        else:
            holder = C.c_float(float(value))
            ptr = C.cast(C.pointer(holder), C.c_void_p)
        if name in self._names:
            k = self._names.index(name)
            self._vals[k], self._keep[k] = ptr, holder
        else:
            self._names.append(name)
            self._vals.append(ptr)
            self._keep.append(holder)

    def names(self):
        return list(self._names)

    def items(self):
        return list(zip(self._names, self._vals))

    def data(self):
        arr = (C.c_void_p * len(self._vals))(*self._vals)
        return arr


class OptSolver:
    """OptSolver.h:43-91."""

    def __init__(self, state, dims, plan_file=BUILTIN_PLAN, solverkind=b"gaussNewtonGPU"):
        self.state, self.lib = state, state.lib
        if isinstance(plan_file, str):
            plan_file = plan_file.encode()
        if isinstance(solverkind, str):
            solverkind = solverkind.encode()
        self.problem = self.lib.Opt_ProblemDefine(state.handle, plan_file, solverkind)
        assert self.problem, "Opt_ProblemDefine returned NULL"       # OptSolver.h:55
        d = (C.c_uint * 2)(int(dims[0]), int(dims[1]))
        self.plan = self.lib.Opt_ProblemPlan(state.handle, self.problem, d)
        assert self.plan, "Opt_ProblemPlan returned NULL"            # OptSolver.h:56
        self.final_cost = float("nan")

    def set_solver_parameters(self, solver_params):
        for name, ptr in solver_params.items():                      # OptUtils.h:104-108
            self.lib.Opt_SetSolverParameter(self.state.handle, self.plan, name.encode(), ptr)

    def solve(self, solver_params, problem_params, profiled=False, iters=None):
        """OptSolver.h:72-91.  profiled=True is launchProfiledSolve (OptUtils.h:47-64): Init, then Step by Step,
        appending a (cost, milliseconds) record per Gauss-Newton iteration to `iters` (SolverIteration.h)."""
        self.set_solver_parameters(solver_params)
        if profiled:
            import time
            import torch
            recs = iters if iters is not None else []
            self.lib.Opt_ProblemInit(self.state.handle, self.plan, problem_params.data())
            torch.cuda.synchronize()
            recs.append((self.lib.Opt_ProblemCurrentCost(self.state.handle, self.plan), 0.0))
            while True:
                t0 = time.perf_counter()
                more = self.lib.Opt_ProblemStep(self.state.handle, self.plan, problem_params.data())
                if not more:
                    break
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3
                recs.append((self.lib.Opt_ProblemCurrentCost(self.state.handle, self.plan), ms))
        else:
            self.lib.Opt_ProblemSolve(self.state.handle, self.plan, problem_params.data())
        self.final_cost = self.lib.Opt_ProblemCurrentCost(self.state.handle, self.plan)
        return self.final_cost

    def init(self, problem_params):
        self.lib.Opt_ProblemInit(self.state.handle, self.plan, problem_params.data())

    def step(self, problem_params):
        return self.lib.Opt_ProblemStep(self.state.handle, self.plan, problem_params.data())

    def current_cost(self):
        return self.lib.Opt_ProblemCurrentCost(self.state.handle, self.plan)

    def resident_launches(self):
        return int(self.lib.ArapFlow_PlanResidentLaunches(self.plan))

    def lm_state(self):
        """ArapFlow_LMState of an "LMGPU" plan: dict(radius, decrease: numpy float32, pcg_iterations: of the last step
        attempted since Init, outcome: a name of LM_OUTCOMES, None before the first step)"""
        r, d, n, o = C.c_float(), C.c_float(), C.c_int(), C.c_int()
        if self.lib.ArapFlow_LMState(self.plan, C.byref(r), C.byref(d), C.byref(n), C.byref(o)) != 0:
            raise ValueError("ArapFlow_LMState: not an LMGPU plan")
        return dict(radius=np.float32(r.value), decrease=np.float32(d.value), pcg_iterations=n.value,
                    outcome=LM_OUTCOMES[o.value] if o.value >= 0 else None)

    def close(self):
        if self.plan:
            self.lib.Opt_PlanFree(self.state.handle, self.plan)
            self.plan = None
        if self.problem:
            self.lib.Opt_ProblemDelete(self.state.handle, self.problem)
            self.problem = None


def load_constraints(path):
    """main.cpp:26-50: first token n, then n x 4 ints."""
    with open(path) as f:
        tok = f.read().split()
    n = int(tok[0])
    vals = [int(t) for t in tok[1:1 + 4 * n]]
    return np.asarray(vals, np.int32).reshape(n, 4)


def border_pins(W, H):
    """main.cpp:130-136"""
    ys, xs = np.mgrid[0:H, 0:W]
    sel = (ys == 0) | (xs == 0) | (ys == H - 1) | (xs == W - 1)
    x, y = xs[sel], ys[sel]                  # row-major order, as the reference's nested loops
    return np.stack([x, y, x, y], -1).astype(np.int32)


class CombinedSolver:
    """The reference's host loop, kept as it is in the reference (ramp built on the host and uploaded,
    one Opt_ProblemSolve per ramp step), driving the drop-in Opt_* symbols only.

    CombinedSolver.h:105-112,139-170 (ctor/addImage), :172-189 (combinedSolveInit), :207-221
    (resetGPU), :223-242 (setConstraintImage); CombinedSolverBase.h:23-31,99-120 (solveAll)."""

    def __init__(self, state, width, height, plan_file=BUILTIN_PLAN, num_iter=19, non_linear_iter=8,
                 linear_iter=400):
        self.state = state
        self.W, self.H = int(width), int(height)
        self.num_iter, self.non_linear_iter, self.linear_iter = num_iter, non_linear_iter, linear_iter
        self.solver = OptSolver(state, (self.W, self.H), plan_file, b"gaussNewtonGPU")
        self.mask_red = None
        self.constraints = None
        self.final_costs = []

    def add_image(self, mask_red, constraints):
        H, W = self.H, self.W
        assert mask_red.shape == (H, W)
        self.mask_red = np.ascontiguousarray(mask_red, np.uint8)
        self.constraints = np.asarray(constraints, np.int32).reshape(-1, 4)
        dev = "cuda"
        self.urshape = torch.empty(H, W, 2, dtype=torch.float32, device=dev)
        self.warp_field = torch.empty(H, W, 2, dtype=torch.float32, device=dev)
        self.warp_angles = torch.empty(H, W, dtype=torch.float32, device=dev)
        self.constraint_image = torch.empty(H, W, 2, dtype=torch.float32, device=dev)
        self.mask = torch.empty(H, W, dtype=torch.float32, device=dev)
        self.reset_gpu()

    def reset_gpu(self):
        H, W = self.H, self.W
        ys, xs = np.mgrid[0:H, 0:W]
        h_ur = np.stack([xs, ys], -1).astype(np.float32)
        self.set_constraint_image(1.0)
        self.urshape.copy_(torch.from_numpy(h_ur))
        self.warp_field.copy_(torch.from_numpy(h_ur))
        self.mask.copy_(torch.from_numpy(self.mask_red.astype(np.float32)))
        self.warp_angles.zero_()

    def set_constraint_image(self, alpha):
        H, W = self.H, self.W
        alpha = np.float32(alpha)
        h = np.full((H, W, 2), -1.0, np.float32)
        one = np.float32(1.0)
        for x, y, tx, ty in self.constraints:          # later entries overwrite earlier ones
            if self.mask_red[y, x] == 0:
                h[y, x, 0] = (one - alpha) * np.float32(x) + alpha * np.float32(tx)
                h[y, x, 1] = (one - alpha) * np.float32(y) + alpha * np.float32(ty)
        self.constraint_image.copy_(torch.from_numpy(h))

    def solve_all(self):
        w_fit_sqrt = math.sqrt(np.float32(100.0))
        w_reg_sqrt = float(np.sqrt(np.float32(0.01)))
        pp = NamedParameters()
        pp.set("Offset", self.warp_field)
        pp.set("Angle", self.warp_angles)
        pp.set("UrShape", self.urshape)
        pp.set("Constraints", self.constraint_image)
        pp.set("Mask", self.mask)
        pp.set("w_fitSqrt", float(np.float32(w_fit_sqrt)))
        pp.set("w_regSqrt", float(np.float32(w_reg_sqrt)))
        sp = NamedParameters()
        sp.set("nIterations", int(self.non_linear_iter))
        sp.set("lIterations", int(self.linear_iter))
        self.reset_gpu()                                   # preSingleSolve
        self.final_costs = []
        for i in range(self.num_iter):
            self.set_constraint_image(np.float32(i + 1) / np.float32(self.num_iter))
            self.final_costs.append(self.solver.solve(sp, pp))
        return self.final_costs

    def warp_field_as_flow(self):
        """warpField(): CombinedSolver.h:352-366"""
        H, W = self.H, self.W
        o = self.warp_field.cpu().numpy()
        ys, xs = np.mgrid[0:H, 0:W]
        o[..., 0] -= xs.astype(np.float32)
        o[..., 1] -= ys.astype(np.float32)
        return o

    def close(self):
        self.solver.close()


def _stats_dict(s):
    """an ArapFlow_MeshStats as a dict in the struct's order, without `reserved`; the floats as numpy float32"""
    return {k: (np.float32(getattr(s, k)) if k.startswith(("det", "disp")) else int(getattr(s, k)))
            for k in capi.MESH_STATS_KEYS}


# ArapFlow_SolverStepRecipe's kernel numbers (host_plan.h: PhaseA, PhaseB) as FrameSolver.stats() names them
PHASE_A_NAMES = ("", "direct", "lds16x16", "lds32x8", "lds64x4", "lds32x16", "lds64x8", "march", "march2", "grid")
PHASE_B_NAMES = ("", "b", "b4", "b4_lean", "b4_r")


class FrameSolver:
    """Batched, device-resident CombinedSolver (ArapFlow_Solver)."""

    def __init__(self, state, width, height, batch=1):
        self.state, self.lib = state, state.lib
        self.W, self.H, self.batch = int(width), int(height), int(batch)
        self.h = self.lib.ArapFlow_SolverCreate(state.handle, self.W, self.H, self.batch)
        if not self.h:
            raise RuntimeError("ArapFlow_SolverCreate failed")
        self.outputs = 0
        self.diag = False

    def set_diag(self, on):
        """fold diagnostics of every later warp (ArapFlow_SolverSetDiag, DESIGN.md "Fold diagnostics"): results() /
        host_results() then carry mesh_stats (a dict over capi.MESH_STATS_KEYS) and fold u8[H,W] -- when the last warp
        (or download) computed them."""
        if self.lib.ArapFlow_SolverSetDiag(self.h, int(bool(on))) != 0:
            raise RuntimeError("ArapFlow_SolverSetDiag failed")
        self.diag = bool(on)

    def set_outputs(self, backward=False, occlusion=False):
        """optional outputs of every later warp (ArapFlow_SolverSetOutputs): backward flow + backward occlusion,
        forward occlusion.  results() / host_results() then carry backward_flow, occlusion_bwd, occlusion -- when the
        last warp (or download) computed them; otherwise they return the base results without those keys."""
        which = (capi.OUT_BACKWARD if backward else 0) | (capi.OUT_OCCLUSION if occlusion else 0)
        if self.lib.ArapFlow_SolverSetOutputs(self.h, which) != 0:
            raise RuntimeError("ArapFlow_SolverSetOutputs failed")
        self.outputs = which

    def set_snapshots(self, steps):
        """in-between frames (ArapFlow_SolverSetSnapshots, DESIGN.md "In-between frames"): strictly increasing ramp-step
        indices 1 <= i <= num_iter, at most capi.MAX_SNAPSHOTS; () switches them off.  Every later solve keeps the
        state after those ramp steps and every warp after it writes their outputs: snapshot() / host_snapshot()."""
        steps = [int(v) for v in steps]
        if any(v < 0 for v in steps):
            raise ValueError("ArapFlow_SolverSetSnapshots: bad arguments")
        arr = (C.c_uint * max(1, len(steps)))(*steps)
        if self.lib.ArapFlow_SolverSetSnapshots(self.h, arr, len(steps)) != 0:
            raise ValueError("ArapFlow_SolverSetSnapshots: bad arguments")

    def snapshot(self, slot, k, want_rgb=True):
        """snapshot k (0-based) of a slot after the last warp: dict(flow, rgb, mask, step)"""
        H, W = self.H, self.W
        flow, step = np.empty((H, W, 2), np.float32), np.empty((H, W, 2), np.float32)
        rgb = np.empty((H, W, 3), np.uint8) if want_rgb else None
        mask = np.empty((H, W), np.uint8)
        p = _host_ptr
        if self.lib.ArapFlow_SolverGetSnapshot(self.h, slot, k, p(flow), p(rgb), p(mask), p(step)) != 0:
            raise ValueError("ArapFlow_SolverGetSnapshot: no snapshot %d for slot %d" % (k, slot))
        return dict(flow=flow, rgb=rgb, mask=mask, step=step)

    def host_snapshot(self, slot, k):
        """views (no copy) of the pinned buffers of snapshot k of a `download` solve: valid until this solver's next
        solve"""
        H, W = self.H, self.W
        pf, pr, pm, ps = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        rc = self.lib.ArapFlow_SolverHostSnapshot(self.h, slot, k, C.byref(pf), C.byref(pr), C.byref(pm), C.byref(ps))
        if rc != 0:
            raise ValueError("ArapFlow_SolverHostSnapshot: no downloaded snapshot %d for slot %d" % (k, slot))
        return dict(flow=_view(pf, C.c_float, (H, W, 2)), rgb=_view(pr, C.c_uint8, (H, W, 3)),
                    mask=_view(pm, C.c_uint8, (H, W)), step=_view(ps, C.c_float, (H, W, 2)))

    def set_frame(self, slot, mask_red, constraints, rgb=None, border_pins=True):
        mask_red = np.ascontiguousarray(mask_red, np.uint8)
        assert mask_red.shape == (self.H, self.W)
        cons = np.ascontiguousarray(np.asarray(constraints, np.int32).reshape(-1, 4))
        rgbp = None
        if rgb is not None:
            rgb = np.ascontiguousarray(rgb, np.uint8)
            assert rgb.shape == (self.H, self.W, 3)
            rgbp = rgb.ctypes.data_as(C.c_void_p)
        rc = self.lib.ArapFlow_SolverSetFrame(self.h, slot, rgbp, mask_red.ctypes.data_as(C.c_void_p),
                                              cons.ctypes.data_as(C.c_void_p), len(cons), int(border_pins))
        if rc != 0:
            raise ValueError("ArapFlow_SolverSetFrame: bad arguments")

    def launches_for(self, nframes):
        """resident launches per Gauss-Newton step a solve of slots [0, nframes) would take (0: two-kernel path)"""
        return int(self.lib.ArapFlow_SolverLaunchesFor(self.h, int(nframes)))

    def solve(self, nframes=None, num_iter=19, non_linear_iter=8, linear_iter=400):
        n = self.batch if nframes is None else nframes
        rc = self.lib.ArapFlow_SolverSolve(self.h, n, num_iter, non_linear_iter, linear_iter)
        if rc != 0:
            raise ValueError("ArapFlow_SolverSolve: bad arguments")

    def solve_async(self, nframes=None, num_iter=19, non_linear_iter=8, linear_iter=400, warp=True, download=True):
        """ArapFlow_SolverSolveAsync: enqueue schedule (+ warp, + download into pinned host buffers), do not wait"""
        n = self.batch if nframes is None else nframes
        rc = self.lib.ArapFlow_SolverSolveAsync(self.h, n, num_iter, non_linear_iter, linear_iter, int(warp), int(download))
        if rc != 0:
            raise ValueError("ArapFlow_SolverSolveAsync: bad arguments")

    def wait(self):
        rc = self.lib.ArapFlow_SolverWait(self.h)
        if rc != 0:
            raise RuntimeError("ArapFlow_SolverWait failed: %d" % rc)

    def host_results(self, slot):
        """views (no copy) of the pinned result buffers of a `download` solve: valid until this solver's next solve"""
        H, W = self.H, self.W
        pf, pr, pm = C.c_void_p(), C.c_void_p(), C.c_void_p()
        rc = self.lib.ArapFlow_SolverHostResults(self.h, slot, C.byref(pf), C.byref(pr), C.byref(pm))
        if rc != 0:
            raise ValueError("ArapFlow_SolverHostResults: no downloaded results for slot %d" % slot)
        out = dict(flow=_view(pf, C.c_float, (H, W, 2)), warped_rgb=_view(pr, C.c_uint8, (H, W, 3)),
                   warped_mask=_view(pm, C.c_uint8, (H, W)))
        if self.outputs:
            pb, pob, po = C.c_void_p(), C.c_void_p(), C.c_void_p()
            rc = self.lib.ArapFlow_SolverHostExtraResults(self.h, slot, C.byref(pb), C.byref(pob), C.byref(po))
            if rc != 0:                 # (that solve computed or downloaded none: the base results only)
                return out
            if pb.value:
                out.update(backward_flow=_view(pb, C.c_float, (H, W, 2)), occlusion_bwd=_view(pob, C.c_uint8, (H, W)))
            if po.value:
                out.update(occlusion=_view(po, C.c_uint8, (H, W)))
        if self.diag:
            ps, pf = C.POINTER(capi.MeshStats)(), C.c_void_p()
            if self.lib.ArapFlow_SolverHostDiag(self.h, slot, C.byref(ps), C.byref(pf)) == 0:
                out.update(mesh_stats=_stats_dict(ps.contents), fold=_view(pf, C.c_uint8, (H, W)))
        return out

    def warp(self, nframes=None):
        n = self.batch if nframes is None else nframes
        rc = self.lib.ArapFlow_SolverWarp(self.h, n)
        if rc != 0:
            raise ValueError("ArapFlow_SolverWarp: bad arguments")

    def results(self, slot, want_rgb=True):
        H, W = self.H, self.W
        flow = np.empty((H, W, 2), np.float32)
        wrgb = np.empty((H, W, 3), np.uint8) if want_rgb else None
        wmsk = np.empty((H, W), np.uint8)
        off = np.empty((H, W, 2), np.float32)
        ang = np.empty((H, W), np.float32)
        cost = C.c_double(0.0)
        p = _host_ptr
        rc = self.lib.ArapFlow_SolverGetResults(self.h, slot, p(flow), p(wrgb), p(wmsk), p(off), p(ang),
                                                C.byref(cost))
        if rc != 0:
            raise ValueError("ArapFlow_SolverGetResults: bad arguments")
        out = dict(flow=flow, warped_rgb=wrgb, warped_mask=wmsk, offset=off, angle=ang, cost=cost.value)
        if self.diag:
            st, fold = capi.MeshStats(), np.empty((H, W), np.uint8)
            if self.lib.ArapFlow_SolverGetDiag(self.h, slot, C.byref(st), p(fold)) == 0:
                out.update(mesh_stats=_stats_dict(st), fold=fold)
        if self.outputs:
            bwd = np.empty((H, W, 2), np.float32) if self.outputs & capi.OUT_BACKWARD else None
            obwd = np.empty((H, W), np.uint8) if self.outputs & capi.OUT_BACKWARD else None
            occ = np.empty((H, W), np.uint8) if self.outputs & capi.OUT_OCCLUSION else None
            if self.lib.ArapFlow_SolverGetExtraResults(self.h, slot, p(bwd), p(obwd), p(occ)) != 0:
                return out              # (the last warp did not compute them: the base results only)
            if bwd is not None:
                out.update(backward_flow=bwd, occlusion_bwd=obwd)
            if occ is not None:
                out.update(occlusion=occ)
        return out

    def stats(self):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self.lib.ArapFlow_SolverStats(self.h, C.byref(a), C.byref(b), C.byref(c))
        ls, fl = C.c_int(0), C.c_int(0)
        self.lib.ArapFlow_SolverResidentLayout(self.h, C.byref(ls), C.byref(fl))
        # group-sum flavour of the resident kernel per launch of a step ("flat" / "any"; one word when they agree, "" when
        # the two-kernel path ran)
        sums = (C.c_int * 64)()
        n = max(0, min(64, self.lib.ArapFlow_SolverResidentSums(self.h, sums, 64)))
        names = ["flat" if sums[k] == 1 else "any" for k in range(n)]
        # the kernels of the last Gauss-Newton step enqueued as a graph (ArapFlow_SolverStepRecipe): "" after a resident step
        rec = (C.c_int * 6)()
        self.lib.ArapFlow_SolverStepRecipe(self.h, rec)
        return dict(pcg_iterations_per_frame=a.value, active_vertices=b.value, grid_vertices=c.value,
                    resident_launches=int(self.lib.ArapFlow_SolverResidentLaunches(self.h)),
                    resident_launches_per_step=ls.value, resident_solves_in_flight=fl.value,
                    resident_sums=names[0] if len(set(names)) == 1 else ",".join(names),
                    lean_stream=bool(self.lib.ArapFlow_SolverLeanStream(self.h)),
                    phase_a=PHASE_A_NAMES[rec[0]], phase_b=PHASE_B_NAMES[rec[1]], a_args=(rec[2], rec[3], rec[4]), lag=rec[5])

    def close(self):
        if self.h:
            self.lib.ArapFlow_SolverFree(self.h)
            self.h = None


def _warp_call(state, name, dims, inputs, outputs, scratch=None, bad_args=True, lead=(), view=None):
    """One ArapFlow_<name> call on host arrays.  `dims`: (W, H) or (W, H, n); `inputs`: (array or None, dtype) and
    `outputs`: (dict key, shape or None = not asked, torch dtype), both in the library's argument order; `scratch`: the
    name of the *ScratchBytes function of a call that takes a scratch buffer, or (name, its arguments) where those are
    not `dims`; `lead`: arguments between the dims and
    the inputs, an (array, dtype) to upload or a value passed as it is; an input (value, None) is passed as it is too (a
    host table among the device buffers).  An input that is a list of arrays, or an
    output whose shape is a list of shapes, is passed as a host array of device pointers and comes back as a list.
    `view`: {key: numpy dtype} of outputs that come back reinterpreted (torch has no unsigned 16-bit tensors to allocate).
    Uploads, allocates, synchronises, calls, and downloads {key: array} of the outputs asked.  A return code of -1 is a
    ValueError where `bad_args`, every other non-zero code a RuntimeError."""
    lib = state.lib
    up = lambda a, dt: a if a is None or dt is None else torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
    new = lambda shape, dt: None if shape is None else torch.empty(*shape, dtype=dt, device="cuda")
    lead = [up(*a) if isinstance(a, tuple) else a for a in lead]
    args = [[up(x, dt) for x in a] if isinstance(a, list) else up(a, dt) for a, dt in inputs]
    outs = {k: [new(q, dt) for q in shape] if isinstance(shape, list) else new(shape, dt) for k, shape, dt in outputs}
    outs = {k: t for k, t in outs.items() if t is not None}
    args += [outs.get(k) for k, _, _ in outputs]
    if scratch:
        sname, sdims = scratch if isinstance(scratch, tuple) else (scratch, dims)
        args.append(torch.empty(int(getattr(lib, "ArapFlow_" + sname)(*sdims)), dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()

    def ptr(t):
        if isinstance(t, list):
            return (C.c_void_p * len(t))(*[None if x is None else x.data_ptr() for x in t])
        return _dev_ptr(t) if isinstance(t, torch.Tensor) else t
    rc = getattr(lib, "ArapFlow_" + name)(state.handle, *dims, *[ptr(t) for t in lead], *[ptr(t) for t in args])
    if rc == -1 and bad_args:
        raise ValueError("ArapFlow_%s: bad arguments" % name)
    if rc != 0:
        raise RuntimeError("ArapFlow_%s failed: %d" % (name, rc))
    torch.cuda.synchronize()
    down = lambda t: None if t is None else t.cpu().numpy()
    res = {k: [down(x) for x in t] if isinstance(t, list) else down(t) for k, t in outs.items()}
    return {k: a.view(view[k]) if view and k in view else a for k, a in res.items()}


def warp_image(state, rgb, mask_red, flow):
    """warp_image (ARAP/warping/src/main.cpp:302-336 minus file I/O) on the GPU.
    rgb u8[H,W,3], mask_red u8[H,W], flow f32[H,W,2] (numpy) -> (warped_rgb, warped_mask)."""
    H, W = mask_red.shape
    r = _warp_call(state, "Warp", (W, H), [(rgb, np.uint8), (mask_red, np.uint8), (flow, np.float32)],
                   [("warped_rgb", (H, W, 3), torch.uint8), ("warped_mask", (H, W), torch.uint8)], "WarpScratchBytes", bad_args=False)
    return r["warped_rgb"], r["warped_mask"]


def warp_image_ex(state, rgb, mask_red, flow, backward=True, occlusion=True):
    """warp_image plus the optional outputs (ArapFlow_WarpEx): a dict of warped_rgb, warped_mask and, as asked for,
    backward_flow f32[H,W,2] + occlusion_bwd u8[H,W], occlusion u8[H,W].  rgb may be None."""
    H, W = mask_red.shape
    r = _warp_call(state, "WarpEx", (W, H), [(rgb, np.uint8), (mask_red, np.uint8), (flow, np.float32)],
                   [("warped_rgb", (H, W, 3) if rgb is not None else None, torch.uint8), ("warped_mask", (H, W), torch.uint8),
                    ("backward_flow", (H, W, 2) if backward else None, torch.float32),
                    ("occlusion_bwd", (H, W) if backward else None, torch.uint8),
                    ("occlusion", (H, W) if occlusion else None, torch.uint8)], "WarpExScratchBytes", bad_args=False)
    return {"warped_rgb": None, **r}


def warp_step(state, rgb, mask_red, flow_a, flow_b):
    """the warp of flow_a and the flow from that warped frame to the state flow_b (ArapFlow_WarpStep, DESIGN.md
    "In-between frames").  rgb u8[H,W,3] or None, mask_red u8[H,W], flow_a / flow_b f32[H,W,2] (numpy) -> a dict of
    warped_rgb (None without rgb), warped_mask and step f32[H,W,2]."""
    H, W = mask_red.shape
    if tuple(np.shape(flow_a)) != (H, W, 2) or tuple(np.shape(flow_b)) != (H, W, 2):
        raise ValueError("warp_step: flows [H,W,2] expected")
    r = _warp_call(state, "WarpStep", (W, H),
                   [(rgb, np.uint8), (mask_red, np.uint8), (flow_a, np.float32), (flow_b, np.float32)],
                   [("warped_rgb", (H, W, 3) if rgb is not None else None, torch.uint8), ("warped_mask", (H, W), torch.uint8),
                    ("step", (H, W, 2), torch.float32)])
    return {"warped_rgb": None, **r}


def warp_layers(state, rgb, masks, flows, bwd=False, occ_bwd=False, occ=True):
    """the layered warp (ArapFlow_WarpLayers, DESIGN.md "Layered warp"): one pass over the n layers of a frame, the
    higher index on top.  rgb u8[H,W,3] or None, masks u8[n,H,W] (red channels, 0 = object), flows f32[n,H,W,2] (numpy)
    -> a dict of the composite warped_rgb (None without rgb), warped_mask and, as asked for, backward_flow f32[H,W,2],
    occlusion_bwd u8[H,W], occlusion u8[H,W] (the forward occlusion across layers)."""
    masks = np.ascontiguousarray(masks, np.uint8)
    flows = np.ascontiguousarray(flows, np.float32)
    if masks.ndim != 3 or flows.shape != masks.shape + (2,):
        raise ValueError("warp_layers: masks [n,H,W] and flows [n,H,W,2] expected")
    n, H, W = masks.shape
    if rgb is not None and tuple(np.shape(rgb)) != (H, W, 3):
        raise ValueError("warp_layers: rgb [H,W,3] expected")
    r = _warp_call(state, "WarpLayers", (W, H, n), [(rgb, np.uint8), (masks, np.uint8), (flows, np.float32)],
                   [("warped_rgb", (H, W, 3) if rgb is not None else None, torch.uint8), ("warped_mask", (H, W), torch.uint8),
                    ("backward_flow", (H, W, 2) if bwd else None, torch.float32), ("occlusion_bwd", (H, W) if occ_bwd else None, torch.uint8),
                    ("occlusion", (H, W) if occ else None, torch.uint8)], "WarpLayersScratchBytes")
    return {"warped_rgb": None, **r}


def warp_layers_step(state, rgb, masks, flows_a, flows_b, step=True, occ=True):
    """layered in-between frames (ArapFlow_WarpLayersStep, DESIGN.md "Layered in-between frames"): the layered warp of
    state a of the n layers, the flow from that composite to state b and the forward occlusion of that link.  rgb
    u8[H,W,3] or None, masks u8[n,H,W] (red channels, 0 = object), flows_a / flows_b f32[n,H,W,2] (numpy) -> a dict of
    warped_rgb (None without rgb), warped_mask and, as asked for, step f32[H,W,2], occlusion_step u8[H,W]."""
    masks = np.ascontiguousarray(masks, np.uint8)
    flows_a = np.ascontiguousarray(flows_a, np.float32)
    flows_b = np.ascontiguousarray(flows_b, np.float32)
    if masks.ndim != 3 or flows_a.shape != masks.shape + (2,) or flows_b.shape != flows_a.shape:
        raise ValueError("warp_layers_step: masks [n,H,W] and flows [n,H,W,2] expected")
    n, H, W = masks.shape
    if rgb is not None and tuple(np.shape(rgb)) != (H, W, 3):
        raise ValueError("warp_layers_step: rgb [H,W,3] expected")
    r = _warp_call(state, "WarpLayersStep", (W, H, n),
                   [(rgb, np.uint8), (masks, np.uint8), (flows_a, np.float32), (flows_b, np.float32)],
                   [("warped_rgb", (H, W, 3) if rgb is not None else None, torch.uint8), ("warped_mask", (H, W), torch.uint8),
                    ("step", (H, W, 2) if step else None, torch.float32), ("occlusion_step", (H, W) if occ else None, torch.uint8)],
                   "WarpLayersStepScratchBytes")
    return {"warped_rgb": None, **r}


def track_points(state, masks, flows, points):
    """point tracks through a sequence (ArapFlow_TrackPoints, DESIGN.md "Point tracks"): masks u8[n,H,W] (red channels,
    0 = object), flows f32[T,n,H,W,2] the T states of the n layers, points f32[P,2] in frame-1 coordinates (numpy) ->
    dict(pos f32[T,P,2], occ u8[T,P]): where each point is in each state, and 255 where it is hidden there."""
    masks = np.ascontiguousarray(masks, np.uint8)
    flows = np.ascontiguousarray(flows, np.float32)
    points = np.ascontiguousarray(points, np.float32)
    if masks.ndim != 3 or flows.ndim != 5 or flows.shape[1:] != masks.shape + (2,):
        raise ValueError("track_points: masks [n,H,W] and flows [T,n,H,W,2] expected")
    if points.ndim != 2 or points.shape[1] != 2:
        raise ValueError("track_points: points [P,2] expected")
    n, H, W = masks.shape
    T, P = flows.shape[0], points.shape[0]
    if state.lib.ArapFlow_TrackPointsScratchBytes(W, H, T, P) == 0 or not 1 <= n <= 255:
        raise ValueError("track_points: 1 <= n <= 255, 1 <= T <= %d, 1 <= P <= 2^24, W * H < 2^31 expected" % (capi.MAX_SNAPSHOTS + 1))
    return _warp_call(state, "TrackPoints", (W, H, n),
                      [(masks, np.uint8), (T, None), (flows, np.float32), (P, None), (points, np.float32)],
                      [("pos", (T, P, 2), torch.float32), ("occ", (T, P), torch.uint8)],
                      ("TrackPointsScratchBytes", (W, H, T, P)))


def warp_diag(state, mask_red, flow, fold=True):
    """fold diagnostics of a flow (ArapFlow_WarpDiag, DESIGN.md "Fold diagnostics"): mask_red u8[H,W], flow f32[H,W,2]
    (numpy) -> dict(stats: a dict over capi.MESH_STATS_KEYS, fold: u8[H,W], 255 = no valid correspondence; None when
    not asked)."""
    mask_red = np.ascontiguousarray(mask_red, np.uint8)
    H, W = mask_red.shape
    if tuple(np.shape(flow)) != (H, W, 2):
        raise ValueError("warp_diag: flow [H,W,2] expected")
    r = _warp_call(state, "WarpDiag", (W, H), [(mask_red, np.uint8), (flow, np.float32)],
                   [("fold", (H, W) if fold else None, torch.uint8), ("stats", (C.sizeof(capi.MeshStats),), torch.uint8)])
    return dict(stats=_stats_dict(capi.MeshStats.from_buffer_copy(r["stats"].tobytes())), fold=r.get("fold"))


def tex_table(layers):
    """a sequence of layer descriptions (kind, seed, m[6], p0, p1, c0, c1, c2) -- pipeline.TexLayer, the kind a number or a
    name of capi.TEX_KINDS -- as the ArapFlow_TexLayer array the library reads; floats are rounded to float32 here"""
    table = (capi.TexLayer * max(1, len(layers)))()
    for q, (kind, seed, m, p0, p1, c0, c1, c2) in zip(table, layers):
        q.kind = capi.TEX_KINDS.index(kind) if isinstance(kind, str) else int(kind)
        q.seed = int(seed) & 0xffffffff
        q.m = _map6(m)
        q.p0, q.p1 = float(p0), float(p1)
        for dst, c in ((q.c0, c0), (q.c1, c1), (q.c2, c2)):
            dst[:] = [int(v) for v in c]
    return table


def texture(state, rgb, masks, layers):
    """procedural textures on the objects of a frame (ArapFlow_Texture, DESIGN.md "Random textures").  rgb u8[H,W,3];
    masks u8[n,H,W] (red channels, 0 = object; the higher index on top) or None: every pixel belongs to layer 0; layers:
    n descriptions (tex_table) -> the retextured frame u8[H,W,3]: a pixel of a layer shows that layer's texture, every
    other pixel rgb."""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("texture: rgb [H,W,3] expected")
    H, W = rgb.shape[:2]
    if masks is not None:
        masks = np.ascontiguousarray(masks, np.uint8)
        if masks.ndim != 3 or masks.shape[1:] != (H, W) or len(masks) != len(layers):
            raise ValueError("texture: masks [n,H,W] with one layer description each expected")
    r = _warp_call(state, "Texture", (W, H, len(layers)), [(rgb, np.uint8), (masks, np.uint8), (tex_table(layers), None)],
                   [("rgb", (H, W, 3), torch.uint8)])
    return r["rgb"]


def retexture_pair(state, rgb, masks, flows, layers):
    """the random-texture twin of a pair (DESIGN.md "Random textures"): texture() on frame 1, then the layered warp of the
    retextured frame with the pair's ALREADY SOLVED flows -- no solve, no new rasteriser.  rgb u8[H,W,3], masks u8[n,H,W],
    flows f32[n,H,W,2], layers: n descriptions -> (rgb1_tex, rgb2_tex, mask2); mask2 is the warped mask of the original
    pair (same flows, same geometry), and with n = 1 rgb2_tex is warp_image of rgb1_tex."""
    rgb1 = texture(state, rgb, masks, layers)
    r = warp_layers(state, rgb1, masks, flows, occ=False)
    return rgb1, r["warped_rgb"], r["warped_mask"]


def blur_schedule(centre, shutter, samples, maps=None, lib=None):
    """the sample times and, with maps = (Ma, Mb), the per-sample sampling maps of an exposure window
    (ArapFlow_BlurSchedule, DESIGN.md "Motion blur"): (times f32[samples], maps f32[samples,6] or None), the library's own
    bits.  Host only (no GPU, no state)."""
    lib = lib or capi.load()
    n = max(1, min(int(samples), capi.MAX_BLUR_SAMPLES))
    times, out = (C.c_float * n)(), (C.c_float * (6 * n))() if maps is not None else None
    Ma, Mb = (_map6(maps[0]), _map6(maps[1])) if maps is not None else (None, None)
    if lib.ArapFlow_BlurSchedule(centre, shutter, samples, Ma, Mb, times, out) != 0:
        raise ValueError("ArapFlow_BlurSchedule: bad arguments")
    return np.array(times[:], np.float32), None if out is None else np.array(out[:], np.float32).reshape(n, 6)


def blur_layers(state, rgb, masks, flows_b, centre, shutter, samples, flows_a=None, bg=None, maps=None, want=("rgb", "alpha")):
    """a motion-blurred frame (ArapFlow_BlurLayers, DESIGN.md "Motion blur"): the integer mean of `samples` layered warps at
    the times centre + shutter * ((k + 0.5) / samples - 0.5) of the flows (1 - t) * flows_a + t * flows_b.  rgb u8[H,W,3],
    masks u8[n,H,W] (red channels, 0 = object), flows_b / flows_a f32[n,H,W,2] (flows_a None: all zero); bg u8[bgH,bgW,3]
    with maps = (Ma, Mb), six floats each (None: both the identity), shows behind the samples that leave a pixel uncovered
    (numpy) -> (rgb u8[H,W,3], alpha u8[H,W]), None for one that `want` leaves out."""
    masks = np.ascontiguousarray(masks, np.uint8)
    flows_b = np.ascontiguousarray(flows_b, np.float32)
    if masks.ndim != 3 or flows_b.shape != masks.shape + (2,):
        raise ValueError("blur_layers: masks [n,H,W] and flows [n,H,W,2] expected")
    if flows_a is not None and np.shape(flows_a) != flows_b.shape:
        raise ValueError("blur_layers: flows_a [n,H,W,2] expected")
    n, H, W = masks.shape
    if tuple(np.shape(rgb)) != (H, W, 3):
        raise ValueError("blur_layers: rgb [H,W,3] expected")
    if set(want) - {"rgb", "alpha"} or not want:
        raise ValueError("blur_layers: want some of rgb, alpha")
    bgW = bgH = 0
    Ma = Mb = None
    if bg is not None:
        bg = np.ascontiguousarray(bg, np.uint8)
        if bg.ndim != 3 or bg.shape[2] != 3:
            raise ValueError("blur_layers: bg [bgH,bgW,3] expected")
        bgH, bgW = bg.shape[:2]
        ident = (1, 0, 0, 0, 1, 0)
        Ma, Mb = (_map6(m) for m in (maps if maps is not None else (ident, ident)))
    elif maps is not None:
        raise ValueError("blur_layers: maps without bg")
    samples = int(samples)
    if state.lib.ArapFlow_BlurLayersScratchBytes(W, H, n, max(samples, 0)) == 0:
        raise ValueError("blur_layers: 1 <= n <= 255, 1 <= samples <= %d, W * H < 2^31 expected" % capi.MAX_BLUR_SAMPLES)
    r = _warp_call(state, "BlurLayers", (W, H, n),
                   [(rgb, np.uint8), (masks, np.uint8), (flows_a, np.float32), (flows_b, np.float32), (float(centre), None),
                    (float(shutter), None), (samples, None), (bg, np.uint8), (bgW, None), (bgH, None), (Ma, None), (Mb, None)],
                   [("rgb", (H, W, 3) if "rgb" in want else None, torch.uint8),
                    ("alpha", (H, W) if "alpha" in want else None, torch.uint8)],
                   ("BlurLayersScratchBytes", (W, H, n, samples)))
    return r.get("rgb"), r.get("alpha")


def blur_pair(state, rgb, masks, flows, shutter, samples, bg=None, maps=None, want=("rgb", "alpha")):
    """the two motion-blurred frames of a pair (DESIGN.md "Motion blur"): frame 1 exposed around t = 0 and frame 2 around
    t = 1, the same shutter and inputs, so the flow between the exposure centres is the pair's own `flows` ->
    ((rgb1, alpha1), (rgb2, alpha2))"""
    return tuple(blur_layers(state, rgb, masks, flows, c, shutter, samples, bg=bg, maps=maps, want=want) for c in (0.0, 1.0))


def light_frame(frame):
    """a frame's light description (seed, m[6], amp, vig, gain[3], gamma, sh_dx, sh_dy, sh_r, sh_g, sigma0, sigma1) --
    pipeline.LightFrame -- as the ArapFlow_LightFrame the library reads; floats are rounded to float32 here"""
    seed, m, amp, vig, gain, gamma, sh_dx, sh_dy, sh_r, sh_g, sigma0, sigma1 = frame
    q = capi.LightFrame()
    q.seed = int(seed) & 0xffffffff
    q.m = _map6(m)
    q.amp, q.vig, q.gamma, q.sigma0, q.sigma1 = float(amp), float(vig), float(gamma), float(sigma0), float(sigma1)
    if len(gain) != 3:
        raise ValueError("a tone curve has three gains")
    q.gain = (C.c_float * 3)(*[float(g) for g in gain])
    q.sh_dx, q.sh_dy, q.sh_r, q.sh_g = (max(-1 << 31, min(int(v), (1 << 31) - 1)) for v in (sh_dx, sh_dy, sh_r, sh_g))
    return q


def light_tables(frame, W, H, lib=None):
    """the tone table and the vignette's geometry of a light description on a W x H frame (ArapFlow_LightTables, DESIGN.md
    "Relit frames"): (lut u8[3,256], geom f32[3] = (cx, cy, inv_r2)), the library's own bits.  Host only (no GPU, no
    state).  A description outside its ranges is a ValueError."""
    lib = lib or capi.load()
    lut, geom = (C.c_uint8 * 768)(), (C.c_float * 3)()
    if not (0 <= int(W) < 1 << 32 and 0 <= int(H) < 1 << 32) or \
            lib.ArapFlow_LightTables(C.byref(light_frame(frame)), int(W), int(H), lut, geom) != 0:
        raise ValueError("ArapFlow_LightTables: bad arguments")
    return np.array(lut[:], np.uint8).reshape(3, 256), np.array(geom[:], np.float32)


def relight(state, rgb, cover, frame, cover_is_mask=False):
    """a finished frame under one light description (ArapFlow_Relight, DESIGN.md "Relit frames"): the objects' shadow on
    the background, the tone curve, the illumination field, the vignette and the noise.  rgb u8[H,W,3]; cover u8[H,W]
    (object: != 0, or == 0 with cover_is_mask, the solver's convention) or None when the description has no shadow;
    frame: a pipeline.LightFrame (numpy) -> the relit frame u8[H,W,3]."""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("relight: rgb [H,W,3] expected")
    H, W = rgb.shape[:2]
    if cover is not None and tuple(np.shape(cover)) != (H, W):
        raise ValueError("relight: cover [H,W] expected")
    r = _warp_call(state, "Relight", (W, H),
                   [(rgb, np.uint8), (cover, np.uint8), (int(bool(cover_is_mask)), None), (C.byref(light_frame(frame)), None)],
                   [("rgb", (H, W, 3), torch.uint8)])
    return r["rgb"]


def relight_pair(state, rgb1, mask1, rgb2, cover2, frames):
    """the relit variant of a pair (DESIGN.md "Relit frames"): frame 1 under frames[0] with mask1 read in the solver's
    convention (object: == 0), frame 2 under frames[1] with cover2 read as a cover (object: != 0) -- the two masks a solve
    and its warp leave.  The geometry is untouched: the pair's flow is shared -> (rgb1_light, rgb2_light)"""
    if len(frames) != 2:
        raise ValueError("relight_pair: two light descriptions expected")
    return relight(state, rgb1, mask1, frames[0], cover_is_mask=True), relight(state, rgb2, cover2, frames[1])


# a sample of a training batch (DESIGN.md "Training batches"): T1, T2 six floats each (output pixel -> source point of
# frame 1 / frame 2), the tone curves (gain[3], gamma per frame), up to four eraser rectangles (x0, y0, x1, y1) on frame
# 2 in output pixels, half-open, and their fill colour
AugSample = collections.namedtuple("AugSample", "T1 T2 gain1 gamma1 gain2 gamma2 erase fill")
AUG_NEUTRAL = AugSample((1, 0, 0, 0, 1, 0), (1, 0, 0, 0, 1, 0), (1, 1, 1), 1.0, (1, 1, 1), 1.0, (), (0, 0, 0))
AUG_OUTPUTS = ("img1", "img2", "flow", "valid")


def _f3(v, what):
    if len(v) != 3:
        raise ValueError("%s: three values expected" % what)
    return (C.c_float * 3)(*[float(x) for x in v])


def aug_sample(sample):
    """an AugSample as the ArapFlow_AugSample the library reads; floats are rounded to float32 here.  More rectangles than
    a sample holds are a ValueError (the library would see only a count)."""
    T1, T2, gain1, gamma1, gain2, gamma2, erase, fill = sample
    q = capi.AugSample()
    q.T1, q.T2 = _map6(T1), _map6(T2)
    q.gain1, q.gain2, q.fill = _f3(gain1, "gain1"), _f3(gain2, "gain2"), _f3(fill, "fill")
    q.gamma1, q.gamma2 = float(gamma1), float(gamma2)
    erase = [tuple(r) for r in erase]
    if len(erase) > capi.AUG_MAX_ERASE or any(len(r) != 4 for r in erase):
        raise ValueError("a sample has at most %d rectangles (x0, y0, x1, y1)" % capi.AUG_MAX_ERASE)
    q.n_erase = len(erase)
    for i, r in enumerate(erase):
        q.erase[i] = (C.c_int32 * 4)(*[max(-1 << 31, min(int(v), (1 << 31) - 1)) for v in r])
    return q


def augment_tables(sample, scale=(1, 1, 1), bias=(0, 0, 0), lib=None):
    """what the library derives of a sample (ArapFlow_AugmentTables, DESIGN.md "Training batches"): (P2 f32[6], the
    inverse of T2; lut f32[2,3,256], the tone table of each frame with the normalisation folded in), the library's own
    bits.  Host only (no GPU, no state).  A sample outside its ranges is a ValueError."""
    lib = lib or capi.load()
    P2, lut = (C.c_float * 6)(), (C.c_float * 1536)()
    if lib.ArapFlow_AugmentTables(C.byref(aug_sample(sample)), _f3(scale, "scale"), _f3(bias, "bias"), P2, lut) != 0:
        raise ValueError("ArapFlow_AugmentTables: bad arguments")
    return np.array(P2[:], np.float32), np.array(lut[:], np.float32).reshape(2, 3, 256)


def augment_pairs(state, rgb1, rgb2, flow, samples, size, skip=None, scale=(1, 1, 1), bias=(0, 0, 0), tau=1.0,
                  want=AUG_OUTPUTS, out=None):
    """a training batch in one launch (ArapFlow_AugmentPairs, DESIGN.md "Training batches").  rgb1, rgb2 u8[B,H,W,3], flow
    f32[B,H,W,2], skip u8[B,H,W] or None (non-zero: no ground truth), numpy arrays or CUDA tensors; an input no wanted
    output needs may be None.  samples: B AugSample; size = (w, h), the crop; scale, bias: the normalisation per channel;
    tau: the most a pixel's flow taps may differ for its flow to count.  -> {name: CUDA tensor} of the outputs `want`
    names: img1, img2 f32[B,3,h,w], flow f32[B,2,h,w], valid u8[B,h,w] (0 / 255).  Nothing is downloaded and nothing
    waited for: the call is enqueued on the state's stream (State.set_stream; by default the null stream, torch's
    default), where the inputs must be ready and the outputs are.  A state has one device table of samples, written in
    the stream's order: calls on one stream follow each other; before a call on another stream than the last one's,
    make that stream wait for the last call (data.AugmentLoader does).  `out`: {name: tensor} of caller-owned CUDA tensors
    (contiguous, of the output's shape and type) to write instead of new ones."""
    want = tuple(want)
    if not want or set(want) - set(AUG_OUTPUTS) or len(set(want)) != len(want):
        raise ValueError("augment_pairs: want: some of %s" % ", ".join(AUG_OUTPUTS))
    w, h = (int(v) for v in size)
    samples = list(samples)
    B = len(samples)

    def up(a, dt, tail, what):
        if a is None:
            return None
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dt))
        if t.dtype != getattr(torch, np.dtype(dt).name) or t.dim() != 1 + len(tail) + 2 or t.shape[0] != B or \
                tuple(t.shape[3:]) != tail:
            raise ValueError("augment_pairs: %s: %s[B,H,W%s] expected" % (what, np.dtype(dt).name, "".join(",%d" % v for v in tail)))
        return t.cuda().contiguous()
    ins = [up(rgb1, np.uint8, (3,), "rgb1"), up(rgb2, np.uint8, (3,), "rgb2"), up(flow, np.float32, (2,), "flow"),
           up(skip, np.uint8, (), "skip")]
    shapes = {tuple(t.shape[1:3]) for t in ins if t is not None}
    if len(shapes) != 1:
        raise ValueError("augment_pairs: inputs of one size [B,H,W,..] expected")
    H, W = shapes.pop()
    if not (0 < w < 1 << 31 and 0 < h < 1 << 31 and 0 < B <= capi.AUG_MAX_BATCH):
        raise ValueError("augment_pairs: a crop of at least one pixel and 1 .. %d samples expected" % capi.AUG_MAX_BATCH)
    form = {"img1": ((B, 3, h, w), torch.float32), "img2": ((B, 3, h, w), torch.float32), "flow": ((B, 2, h, w), torch.float32),
            "valid": ((B, h, w), torch.uint8)}
    outs = {}
    for k in want:
        shape, dt = form[k]
        t = (out or {}).get(k)
        if t is None:
            t = torch.empty(shape, dtype=dt, device="cuda")
        elif not (t.is_cuda and t.is_contiguous() and tuple(t.shape) == shape and t.dtype == dt):
            raise ValueError("augment_pairs: out[%r]: a contiguous CUDA %s tensor of shape %s expected" % (k, dt, shape))
        outs[k] = t
    table = (capi.AugSample * B)(*[aug_sample(s) for s in samples])
    ptr = lambda t: None if t is None else _dev_ptr(t)
    rc = state.lib.ArapFlow_AugmentPairs(state.handle, W, H, w, h, B, *[ptr(t) for t in ins], table, _f3(scale, "scale"),
                                         _f3(bias, "bias"), float(tau), *[ptr(outs.get(k)) for k in AUG_OUTPUTS])
    if rc == -1:
        raise ValueError("ArapFlow_AugmentPairs: bad arguments")
    if rc != 0:
        raise RuntimeError("ArapFlow_AugmentPairs failed: %d" % rc)
    return outs


# a frame of a training clip (DESIGN.md "Training clips"): T six floats (output pixel -> source point of this frame), its
# tone curve (gain[3], gamma), up to four eraser rectangles (x0, y0, x1, y1) in output pixels, half-open, and their fill
ClipFrame = collections.namedtuple("ClipFrame", "T gain gamma erase fill")
CLIP_NEUTRAL = ClipFrame((1, 0, 0, 0, 1, 0), (1, 1, 1), 1.0, (), (0, 0, 0))
CLIP_OUTPUTS = ("video", "flows", "valid", "tracks", "vis")


def clip_frame(frame):
    """a ClipFrame as the ArapFlow_ClipFrame the library reads; floats are rounded to float32 here.  More rectangles than
    a frame holds are a ValueError (the library would see only a count)."""
    T, gain, gamma, erase, fill = frame
    q = capi.ClipFrame()
    q.T, q.gain, q.fill, q.gamma = _map6(T), _f3(gain, "gain"), _f3(fill, "fill"), float(gamma)
    erase = [tuple(r) for r in erase]
    if len(erase) > capi.AUG_MAX_ERASE or any(len(r) != 4 for r in erase):
        raise ValueError("a frame has at most %d rectangles (x0, y0, x1, y1)" % capi.AUG_MAX_ERASE)
    q.n_erase = len(erase)
    for i, r in enumerate(erase):
        q.erase[i] = (C.c_int32 * 4)(*[max(-1 << 31, min(int(v), (1 << 31) - 1)) for v in r])
    return q


def clip_tables(frame, scale=(1, 1, 1), bias=(0, 0, 0), lib=None):
    """what the library derives of a clip's frame (ArapFlow_ClipTables, DESIGN.md "Training clips"): (P f32[6], the
    inverse of T; lut f32[3,256], the frame's tone table with the normalisation folded in), the library's own bits.  Host
    only (no GPU, no state).  A frame outside its ranges is a ValueError."""
    lib = lib or capi.load()
    P, lut = (C.c_float * 6)(), (C.c_float * 768)()
    if lib.ArapFlow_ClipTables(C.byref(clip_frame(frame)), _f3(scale, "scale"), _f3(bias, "bias"), P, lut) != 0:
        raise ValueError("ArapFlow_ClipTables: bad arguments")
    return np.array(P[:], np.float32), np.array(lut[:], np.float32).reshape(3, 256)


def augment_clips(state, frames, samples, size, links=(), flows=None, skip=None, pos=None, occ=None, scale=(1, 1, 1),
                  bias=(0, 0, 0), tau=1.0, want=None, out=None):
    """a batch of training clips in at most two launches (ArapFlow_AugmentClips, DESIGN.md "Training clips").  frames
    u8[B,T,H,W,3]; links: L pairs (i, j) of frame numbers, one table for the batch; flows f32[B,L,H,W,2], link l on the
    pixels of frame i towards frame j; skip u8[B,L,H,W] or None (non-zero: no ground truth); pos f32[B,T,P,2] and occ
    u8[B,T,P] (non-zero: hidden), a point's position in every source frame; numpy arrays or CUDA tensors, and an input no
    wanted output needs may be None.  samples: B sequences of T ClipFrame; size = (w, h), the crop; scale, bias, tau as in
    augment_pairs.  -> {name: CUDA tensor} of the outputs `want` names (by default every one whose inputs are given):
    video f32[B,T,3,h,w], flows f32[B,L,2,h,w], valid u8[B,L,h,w] (0 / 255), tracks f32[B,T,P,2], vis u8[B,T,P]
    (0 / 255).  Nothing is downloaded and nothing waited for: the call is enqueued on the state's stream, under
    augment_pairs' rules (one device table per state; data.ClipLoader orders its calls).  `out`: {name: tensor} of
    caller-owned CUDA tensors (contiguous, of the output's shape and type) to write instead of new ones."""
    given = {"video": frames is not None, "flows": flows is not None, "valid": flows is not None, "tracks": pos is not None,
             "vis": pos is not None and occ is not None}
    want = tuple(k for k in CLIP_OUTPUTS if given[k]) if want is None else tuple(want)
    if not want or set(want) - set(CLIP_OUTPUTS) or len(set(want)) != len(want):
        raise ValueError("augment_clips: want: some of %s" % ", ".join(CLIP_OUTPUTS))
    w, h = (int(v) for v in size)
    samples = [list(s) for s in samples]
    B = len(samples)
    T = len(samples[0]) if B else 0
    if not (0 < B <= capi.AUG_MAX_BATCH and 0 < T <= capi.CLIP_MAX_FRAMES and B * T <= capi.CLIP_MAX_UNITS) or \
            any(len(s) != T for s in samples):
        raise ValueError("augment_clips: samples: 1 .. %d clips of one length 1 .. %d, at most %d frames in all expected"
                         % (capi.AUG_MAX_BATCH, capi.CLIP_MAX_FRAMES, capi.CLIP_MAX_UNITS))
    links = [tuple(int(v) for v in l) for l in links]
    L = len(links)
    if L > capi.CLIP_MAX_LINKS or any(len(l) != 2 for l in links):
        raise ValueError("augment_clips: links: at most %d pairs (i, j) expected" % capi.CLIP_MAX_LINKS)

    def up(a, dt, lead, tail, what):
        if a is None:
            return None
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dt))
        if t.dtype != getattr(torch, np.dtype(dt).name) or t.dim() != 2 + len(tail) or tuple(t.shape[:2]) != (B, lead) or \
                any(v is not None and t.shape[2 + i] != v for i, v in enumerate(tail)):
            raise ValueError("augment_clips: %s: %s[%d,%d,%s] expected" % (what, np.dtype(dt).name, B, lead, ",".join(
                "*" if v is None else "%d" % v for v in tail)))
        return t.cuda().contiguous()
    frames, flows, skip = (up(frames, np.uint8, T, (None, None, 3), "frames"), up(flows, np.float32, L, (None, None, 2), "flows"),
                           up(skip, np.uint8, L, (None, None), "skip"))
    pos, occ = up(pos, np.float32, T, (None, 2), "pos"), up(occ, np.uint8, T, (None,), "occ")
    shapes = {tuple(t.shape[2:4]) for t in (frames, flows, skip) if t is not None}
    counts = {t.shape[2] for t in (pos, occ) if t is not None}
    if len(shapes) > 1 or len(counts) > 1:
        raise ValueError("augment_clips: frames, flows and skip of one size [..,H,W,..], pos and occ of one P expected")
    H, W = shapes.pop() if shapes else (1, 1)                      # (no plane is read: any size serves)
    P = counts.pop() if counts else 0
    if not (0 < w < 1 << 31 and 0 < h < 1 << 31):
        raise ValueError("augment_clips: a crop of at least one pixel expected")
    form = {"video": ((B, T, 3, h, w), torch.float32), "flows": ((B, L, 2, h, w), torch.float32), "valid": ((B, L, h, w), torch.uint8),
            "tracks": ((B, T, P, 2), torch.float32), "vis": ((B, T, P), torch.uint8)}
    outs = {}
    for k in want:
        shape, dt = form[k]
        t = (out or {}).get(k)
        if t is None:
            t = torch.empty(shape, dtype=dt, device="cuda")
        elif not (t.is_cuda and t.is_contiguous() and tuple(t.shape) == shape and t.dtype == dt):
            raise ValueError("augment_clips: out[%r]: a contiguous CUDA %s tensor of shape %s expected" % (k, dt, shape))
        outs[k] = t
    table = (capi.ClipFrame * (B * T))(*[clip_frame(f) for s in samples for f in s])
    link_table = (C.c_int32 * (2 * L))(*[v for l in links for v in l]) if L else None
    ptr = lambda t: None if t is None else _dev_ptr(t)
    rc = state.lib.ArapFlow_AugmentClips(state.handle, W, H, w, h, B, T, L, P, ptr(frames), link_table, ptr(flows), ptr(skip),
                                         ptr(pos), ptr(occ), table, _f3(scale, "scale"), _f3(bias, "bias"), float(tau),
                                         *[ptr(outs.get(k)) for k in CLIP_OUTPUTS])
    if rc == -1:
        raise ValueError("ArapFlow_AugmentClips: bad arguments")
    if rc != 0:
        raise RuntimeError("ArapFlow_AugmentClips failed: %d" % rc)
    return outs


SEG_OUTPUTS = ("idx1", "idx2", "mb1", "mb2", "dist1", "dist2")


def seg_maps(state, masks, flows, tau=1.0, radius=140, M1=None, M2=None, which=SEG_OUTPUTS):
    """the segment maps of a pair (ArapFlow_SegMaps, DESIGN.md "Segment maps").  masks u8[n,H,W] (red channels, 0 =
    object), flows f32[n,H,W,2], the higher index on top; M1, M2: the cameras of a moving background, six floats each, or
    both None (numpy) -> {name: array} of the outputs `which` names: idx1 / idx2 u8[H,W], the object index maps of frame
    1 and frame 2 (0: no object); mb1 / mb2 u8[H,W], 255 where the full forward / backward flow jumps by more than tau
    against a 4-neighbour; dist1 / dist2 u16[H,W], the squared distance to the nearest such pixel where <= radius^2,
    else 65535."""
    masks = np.ascontiguousarray(masks, np.uint8)
    flows = np.ascontiguousarray(flows, np.float32)
    if masks.ndim != 3 or flows.shape != masks.shape + (2,):
        raise ValueError("seg_maps: masks [n,H,W] and flows [n,H,W,2] expected")
    n, H, W = masks.shape
    which = tuple(which)
    if not which or set(which) - set(SEG_OUTPUTS):
        raise ValueError("seg_maps: which: some of %s" % ", ".join(SEG_OUTPUTS))
    if (M1 is None) != (M2 is None):
        raise ValueError("seg_maps: both cameras or neither")
    radius = int(radius)
    if not 0 <= radius <= capi.SEG_MAX_RADIUS or state.lib.ArapFlow_SegMapsScratchBytes(W, H, n) == 0:
        raise ValueError("seg_maps: 1 <= n <= 255, 0 <= radius <= %d, 0 < W * H < 2^31 expected" % capi.SEG_MAX_RADIUS)
    maps = [(None, None), (None, None)] if M1 is None else [(_map6(M1), None), (_map6(M2), None)]
    return _warp_call(state, "SegMaps", (W, H, n),
                      [(masks, np.uint8), (flows, np.float32)] + maps + [(float(tau), None), (radius, None)],
                      [(k, (H, W) if k in which else None, torch.int16 if k.startswith("dist") else torch.uint8)
                       for k in SEG_OUTPUTS], "SegMapsScratchBytes", view={"dist1": np.uint16, "dist2": np.uint16})


def flow_score(state, gt, est, occ=None, dist=None, skip=None, err=False):
    """the error table of an estimated flow against its ground truth (ArapFlow_FlowScore, DESIGN.md "Flow scoring").
    gt, est f32[H,W,2] or f32[n,H,W,2]; occ u8 (non-zero: occluded), dist u16 (ArapFlow_SegMaps' squared distance), skip
    u8 (non-zero: left out), each [H,W] / [n,H,W] or None (numpy) -> {"table": u64[n,10,8]}, rows in the order of
    SCORE_ROWS and fields in that of SCORE_FIELDS (row 9: skipped, gt_nonfinite), and with `err` also {"err": f32[n,H,W]},
    the end-point error of a counted pixel and -1 on every other."""
    gt = np.ascontiguousarray(gt, np.float32)
    est = np.ascontiguousarray(est, np.float32)
    if gt.ndim == 3:
        gt, est = gt[None], est[None] if est.ndim == 3 else est
    if gt.ndim != 4 or gt.shape[3] != 2 or est.shape != gt.shape:
        raise ValueError("flow_score: gt and est [H,W,2] or [n,H,W,2] of one shape expected")
    n, H, W = gt.shape[:3]
    planes = []
    for name, a, dt in (("occ", occ, np.uint8), ("dist", dist, np.uint16), ("skip", skip, np.uint8)):
        if a is not None:
            a = np.ascontiguousarray(a, dt).reshape((-1,) + np.shape(a)[-2:])
            if a.shape != (n, H, W):
                raise ValueError("flow_score: %s of gt's shape without its last axis expected" % name)
            a = a.view(np.int16) if dt is np.uint16 else a       # (torch uploads no unsigned 16-bit arrays)
        planes.append((a, np.int16 if dt is np.uint16 else dt))
    return _warp_call(state, "FlowScore", (W, H, n), [(gt, np.float32), (est, np.float32)] + planes,
                      [("table", (n, len(SCORE_ROWS), len(SCORE_FIELDS)), torch.int64),
                       ("err", (n, H, W) if err else None, torch.float32)], view={"table": np.uint64})


def track_score(state, gt_pos, gt_occ, est_pos, est_occ, scale=(1, 1)):
    """the TAP-Vid table of estimated tracks against their ground truth (ArapFlow_TrackScore, DESIGN.md "Track scoring").
    gt_pos, est_pos f32[F,P,2]; gt_occ, est_occ u8[F,P], non-zero = hidden (a track file's planes, numpy); scale: the
    factors (sx, sy) the error is taken under -> u64[F,3,16], classes in the order of TSCORE_CLASSES and fields in that
    of TSCORE_FIELDS; frame 0 holds the numbers of valid and invalid points."""
    gt_pos = np.ascontiguousarray(gt_pos, np.float32)
    est_pos = np.ascontiguousarray(est_pos, np.float32)
    gt_occ = np.ascontiguousarray(gt_occ, np.uint8)
    est_occ = np.ascontiguousarray(est_occ, np.uint8)
    if gt_pos.ndim != 3 or gt_pos.shape[2] != 2 or est_pos.shape != gt_pos.shape:
        raise ValueError("track_score: gt_pos and est_pos [F,P,2] of one shape expected")
    if gt_occ.shape != gt_pos.shape[:2] or est_occ.shape != gt_occ.shape:
        raise ValueError("track_score: gt_occ and est_occ [F,P] expected")
    F, P = gt_occ.shape
    sx, sy = (float(np.float32(v)) for v in scale)
    return _warp_call(state, "TrackScore", (F, P),
                      [(gt_pos, np.float32), (gt_occ, np.uint8), (est_pos, np.float32), (est_occ, np.uint8), (sx, None), (sy, None)],
                      [("table", (F, len(TSCORE_CLASSES), len(TSCORE_FIELDS)), torch.int64)], view={"table": np.uint64})["table"]


def chain_flows(state, flows, points, bwd=None):
    """estimated tracks by chaining per-link flow estimates (ArapFlow_ChainFlows, DESIGN.md "Track scoring"): flows
    f32[L,H,W,2], link j from sequence frame j to j + 1; bwd the same shape or None, link j from frame j + 1 back to j
    (the forward-backward check of the visibility); points f32[P,2] in frame 0 (numpy) -> (pos f32[L+1,P,2], occ
    u8[L+1,P]), the planes of a track file."""
    flows = np.ascontiguousarray(flows, np.float32)
    points = np.ascontiguousarray(points, np.float32)
    if flows.ndim != 4 or flows.shape[3] != 2:
        raise ValueError("chain_flows: flows [L,H,W,2] expected")
    if points.ndim != 2 or points.shape[1] != 2:
        raise ValueError("chain_flows: points [P,2] expected")
    if bwd is not None:
        bwd = np.ascontiguousarray(bwd, np.float32)
        if bwd.shape != flows.shape:
            raise ValueError("chain_flows: bwd of flows' shape expected")
    L, H, W = flows.shape[:3]
    P = points.shape[0]
    r = _warp_call(state, "ChainFlows", (W, H, L), [(flows, np.float32), (bwd, np.float32), (P, None), (points, np.float32)],
                   [("pos", (L + 1, P, 2), torch.float32), ("occ", (L + 1, P), torch.uint8)])
    return r["pos"], r["occ"]


def interp_frames(state, a, b, fwd, times, bwd=None, want_src=False):
    """estimated in-between frames of a pair from a flow estimate, by flow splatting (ArapFlow_InterpFrames, DESIGN.md
    "Frames from flows"): a, b u8[H,W,3], frame 1 and frame 2; fwd f32[H,W,2], the flow a -> b on a's pixels; bwd the same
    shape or None, the flow b -> a on b's pixels; times: K of them, each in (0, 1) (numpy) -> out u8[K,H,W,3], or with
    `want_src` (out, src u8[K,H,W]): 0 both frames, 1 a only, 2 b only, 3 neither, plus 4 where the flow came from the
    hole fill, 255 a hole."""
    a = np.ascontiguousarray(a, np.uint8)
    b = np.ascontiguousarray(b, np.uint8)
    fwd = np.ascontiguousarray(fwd, np.float32)
    if a.ndim != 3 or a.shape[2] != 3 or b.shape != a.shape:
        raise ValueError("interp_frames: a and b [H,W,3] of one shape expected")
    H, W = a.shape[:2]
    if fwd.shape != (H, W, 2):
        raise ValueError("interp_frames: fwd [H,W,2] of the frames' size expected")
    if bwd is not None:
        bwd = np.ascontiguousarray(bwd, np.float32)
        if bwd.shape != fwd.shape:
            raise ValueError("interp_frames: bwd of fwd's shape expected")
    times = np.ascontiguousarray(times, np.float32).reshape(-1)
    K = times.size
    r = _warp_call(state, "InterpFrames", (W, H),
                   [(a, np.uint8), (b, np.uint8), (fwd, np.float32), (bwd, np.float32), (K, None),
                    (times.ctypes.data_as(C.POINTER(C.c_float)), None)],
                   [("out", (K, H, W, 3), torch.uint8), ("src", (K, H, W) if want_src else None, torch.uint8)],
                   ("InterpScratchBytes", (W, H, K)))
    return (r["out"], r["src"]) if want_src else r["out"]


def frame_score(state, ref, est, occ=None, dist=None, skip=None, obj=None, ssim=False):
    """the PSNR / integer-SSIM table of estimated frames against reference frames (ArapFlow_FrameScore, DESIGN.md "Frame
    scoring").  ref, est u8[H,W,3] or u8[n,H,W,3]; occ u8 (non-zero: occluded), dist u16 (ArapFlow_SegMaps' squared
    distance), skip u8 (non-zero: left out), obj u8 (0: object, non-zero: background), each [H,W] / [n,H,W] or None
    (numpy) -> {"table": u64[n,9,7]}, rows in the order of FSCORE_ROWS and fields in that of FSCORE_FIELDS (row 8: pixels,
    windows), and with `ssim` also {"ssim": f32[n,H,W]}, s at the anchor of a counted window and -2 on every other pixel."""
    ref = np.ascontiguousarray(ref, np.uint8)
    est = np.ascontiguousarray(est, np.uint8)
    if ref.ndim == 3:
        ref, est = ref[None], est[None] if est.ndim == 3 else est
    if ref.ndim != 4 or ref.shape[3] != 3 or est.shape != ref.shape:
        raise ValueError("frame_score: ref and est [H,W,3] or [n,H,W,3] of one shape expected")
    n, H, W = ref.shape[:3]
    planes = []
    for name, a, dt in (("occ", occ, np.uint8), ("dist", dist, np.uint16), ("skip", skip, np.uint8), ("obj", obj, np.uint8)):
        if a is not None:
            a = np.ascontiguousarray(a, dt).reshape((-1,) + np.shape(a)[-2:])
            if a.shape != (n, H, W):
                raise ValueError("frame_score: %s of ref's shape without its last axis expected" % name)
            a = a.view(np.int16) if dt is np.uint16 else a       # (torch uploads no unsigned 16-bit arrays)
        planes.append((a, np.int16 if dt is np.uint16 else dt))
    return _warp_call(state, "FrameScore", (W, H, n), [(ref, np.uint8), (est, np.uint8)] + planes,
                      [("table", (n, len(FSCORE_ROWS), len(FSCORE_FIELDS)), torch.int64),
                       ("ssim", (n, H, W) if ssim else None, torch.float32)], view={"table": np.uint64})


def _score_maps(name, gt, est, skip):
    gt = np.ascontiguousarray(gt, np.uint8)
    est = np.ascontiguousarray(est, np.uint8)
    if gt.ndim == 2:
        gt, est = gt[None], est[None] if est.ndim == 2 else est
    if gt.ndim != 3 or est.shape != gt.shape:
        raise ValueError("%s: gt and est [H,W] or [n,H,W] of one shape expected" % name)
    if skip is not None:
        skip = np.ascontiguousarray(skip, np.uint8).reshape((-1,) + np.shape(skip)[-2:])
        if skip.shape != gt.shape:
            raise ValueError("%s: skip of gt's shape expected" % name)
    return gt, est, skip


def label_score(state, gt, est, L, radius, skip=None):
    """the DAVIS J / F counts of estimated label maps per object (ArapFlow_LabelScore, DESIGN.md "Map scoring").  gt, est
    u8[H,W] or u8[n,H,W], label maps with 0 = no object; skip u8 of that shape or None, non-zero = left out; 1 <= L <= 255
    labels scored; radius 0..254, the tolerance of the boundary match (numpy) -> {"table": u64[n,L+1,8]}: row 0 in the
    order of LSCORE_FRAME_FIELDS, row k of label k in that of LSCORE_FIELDS."""
    gt, est, skip = _score_maps("label_score", gt, est, skip)
    n, H, W = gt.shape
    return _warp_call(state, "LabelScore", (W, H, n), [(gt, np.uint8), (est, np.uint8), (skip, np.uint8)],
                      [("table", (n, max(int(L), 0) + 1, len(LSCORE_FIELDS)), torch.int64)], ("MapScoreScratchBytes", (W, H)),
                      lead=(int(L), int(radius)), view={"table": np.uint64})


def map_score(state, gt, est, skip=None, thr=(), radius=0):
    """the precision / recall counts of estimated occlusion or motion-boundary maps (ArapFlow_MapScore, DESIGN.md "Map
    scoring").  gt u8[H,W] or u8[n,H,W], non-zero = positive; est u8 of that shape, a score 0..255; skip likewise or None;
    thr up to 8 thresholds 1..255 and radius 0..254 for the tolerant boundary match (numpy) -> {"hist": u64[n,2,256],
    "match": u64[n,len(thr),4]}: hist[c][v] the counted pixels of class c = (gt != 0) with est == v, match[j] = (a, b,
    a_hit, b_hit) of A = {gt != 0}, B = {est >= thr[j]}."""
    gt, est, skip = _score_maps("map_score", gt, est, skip)
    n, H, W = gt.shape
    thr = [int(t) for t in thr]
    if any(t < 0 or t >= 1 << 32 for t in thr):
        raise ValueError("map_score: bad threshold")
    m = len(thr)
    r = _warp_call(state, "MapScore", (W, H, n),
                   [(gt, np.uint8), (est, np.uint8), (skip, np.uint8), (m, None), ((C.c_uint * m)(*thr) if m else None, None),
                    (int(radius), None)],
                   [("hist", (n, 2, 256), torch.int64), ("match", (n, m, 4) if m else None, torch.int64)],
                   ("MapScoreScratchBytes", (W, H)), view={"hist": np.uint64, "match": np.uint64})
    r.setdefault("match", np.zeros((n, 0, 4), np.uint64))
    return r


BG_OUTPUTS = ("out_rgb1","out_rgb2", "flow_full", "occ_full", "bwd_full", "occ_bwd_full")


def _map6(m):
    m = np.ascontiguousarray(m, np.float32).reshape(-1)
    if m.shape != (6,):
        raise ValueError("an affine map is six numbers (a, b, c, d, e, f)")
    return (C.c_float * 6)(*m.tolist())


def background_maps(M1, M2, lib=None):
    """the point maps of two sampling maps (ArapFlow_BackgroundMaps, DESIGN.md "Moving background"): (G, Ginv), float32
    [6] each, G = M2^-1 o M1 from frame 1 to frame 2 and Ginv back; the library's own bits.  Host only (no GPU, no
    state)."""
    lib = lib or capi.load()
    g, gi = (C.c_float * 6)(), (C.c_float * 6)()
    if lib.ArapFlow_BackgroundMaps(_map6(M1), _map6(M2), g, gi) != 0:
        raise ValueError("ArapFlow_BackgroundMaps: non-finite or singular maps")
    return np.array(g[:], np.float32), np.array(gi[:], np.float32)


def background(state, bg, M1, M2, rgb1, mask_red, rgb2, cover2, flow, occ=None, bwd=None, occ_bwd=None, want=None):
    """the moving background of a warped pair (ArapFlow_Background, DESIGN.md "Moving background").  bg u8[bgH,bgW,3];
    M1, M2 six floats each; rgb1 / rgb2 u8[H,W,3], mask_red / cover2 u8[H,W] (frame-1 object: mask_red == 0, frame-2
    object: cover2 != 0), flow / bwd f32[H,W,2], occ / occ_bwd u8[H,W] (numpy; any input but bg and the masks may be
    None).  `want`: which of BG_OUTPUTS to compute; by default every one whose input is given.  Returns {name: array}."""
    mask_red = np.ascontiguousarray(mask_red, np.uint8)
    H, W = mask_red.shape
    bg = np.ascontiguousarray(bg, np.uint8)
    if bg.ndim != 3 or bg.shape[2] != 3:
        raise ValueError("background: bg [bgH,bgW,3] expected")
    given = dict(out_rgb1=rgb1, out_rgb2=rgb2, flow_full=flow, occ_full=occ, bwd_full=bwd, occ_bwd_full=occ_bwd)
    if want is None:
        want = [k for k in BG_OUTPUTS if given[k] is not None]
    if set(want) - set(BG_OUTPUTS):
        raise ValueError("background: unknown output in %r" % (want,))
    shape = dict(out_rgb1=(H, W, 3), out_rgb2=(H, W, 3), flow_full=(H, W, 2), occ_full=(H, W), bwd_full=(H, W, 2),
                 occ_bwd_full=(H, W))
    dt = dict(flow_full=torch.float32, bwd_full=torch.float32)
    return _warp_call(state, "Background", (W, H),
                      [(rgb1, np.uint8), (mask_red, np.uint8), (rgb2, np.uint8), (cover2, np.uint8), (flow, np.float32),
                       (occ, np.uint8), (bwd, np.float32), (occ_bwd, np.uint8)],
                      [(k, shape[k] if k in want else None, dt.get(k, torch.uint8)) for k in BG_OUTPUTS],
                      lead=[(bg, np.uint8), bg.shape[1], bg.shape[0], _map6(M1), _map6(M2)])


BG_SEQ_OUTPUTS = ("out_rgb", "flow_full", "occ_full")


def background_seq(state, bg, maps, mask_red, covers, rgbs, flows, occs=None, want=None):
    """the moving background of a sequence of m frames, frame 1 -> in-between frames -> frame 2 (ArapFlow_BackgroundSeq,
    DESIGN.md "Moving background over in-between frames").  bg u8[bgH,bgW,3]; maps [m,6], the frames' sampling maps;
    mask_red u8[H,W], frame 1's own mask (object: == 0); covers: m masks u8[H,W] (object: != 0; entry 0 is not used and may
    be None); rgbs: m frames u8[H,W,3]; flows: m - 1 object-side flows f32[H,W,2], flows[f] in the domain of frame f;
    occs: m - 1 object-side occlusions u8[H,W] (numpy; any entry of rgbs / flows / occs may be None, and so may the
    lists).  `want`: {name: one flag per frame (out_rgb) or per link (flow_full, occ_full)} over BG_SEQ_OUTPUTS, a name
    left out: none of it; by default every output whose input is given.  Returns {name: list}, out_rgb per frame,
    flow_full and occ_full per link, None where an entry was not computed."""
    mask_red = np.ascontiguousarray(mask_red, np.uint8)
    H, W = mask_red.shape
    bg = np.ascontiguousarray(bg, np.uint8)
    if bg.ndim != 3 or bg.shape[2] != 3:
        raise ValueError("background_seq: bg [bgH,bgW,3] expected")
    maps = np.ascontiguousarray(maps, np.float32)
    if maps.ndim != 2 or maps.shape[1] != 6 or len(maps) < 2:
        raise ValueError("background_seq: maps [m,6] with m >= 2 expected")
    m = len(maps)
    fill = lambda a, n: [None] * n if a is None else list(a)
    covers, rgbs, flows, occs = fill(covers, m), fill(rgbs, m), fill(flows, m - 1), fill(occs, m - 1)
    if (len(covers), len(rgbs), len(flows), len(occs)) != (m, m, m - 1, m - 1):
        raise ValueError("background_seq: %d covers and rgbs, %d flows and occs expected" % (m, m - 1))
    given = dict(out_rgb=rgbs, flow_full=flows, occ_full=occs)
    if want is None:
        want = {k: [a is not None for a in given[k]] for k in BG_SEQ_OUTPUTS}
    if set(want) - set(BG_SEQ_OUTPUTS) or any(len(want[k]) != len(given[k]) for k in want):
        raise ValueError("background_seq: bad `want` %r" % (want,))
    shape = dict(out_rgb=(H, W, 3), flow_full=(H, W, 2), occ_full=(H, W))
    outputs = [(k, [shape[k] if w else None for w in want.get(k, [False] * len(given[k]))],
                torch.float32 if k == "flow_full" else torch.uint8) for k in BG_SEQ_OUTPUTS]
    return _warp_call(state, "BackgroundSeq", (W, H),
                      [(mask_red, np.uint8), (covers, np.uint8), (rgbs, np.uint8), (flows, np.float32), (occs, np.uint8)],
                      outputs, lead=[(bg, np.uint8), bg.shape[1], bg.shape[0], m,
                                     maps.ctypes.data_as(C.POINTER(C.c_float))])
