"""The kernel-per-phase PCG path of the frame solver (arap_stream.h, recipe in host_step.h: plan_step_recipe) against the
float32 CPU oracle, bit for bit, at the shapes its kernels branch on: partial last blocks and chunks of one row, heights
below 4, strips of one and of four columns, a single quad, inactive 64x4 tile rows inside a march (stale ring rows in LDS),
an empty slot in a batch, one and two PCG iterations (the lean schedule's lag reads the other half of the p double buffer),
and each of the pairs march2<7> + b4_r, march<5> + b / b4_lean and grid<64,8> + b / b4_lean.

The resident kernel is off in every case and every case asserts, from FrameSolver.stats(), the kernel pair and the strip /
chunk (or tile) counts it was written for: a case cannot drift onto another kernel unnoticed.  Both sides perform one float32
operation list with float64 order-fixed sums (DESIGN.md "Bit-reproducible arithmetic"), so the standard is equality of every
Offset and Angle element and of the cost, in every slot.

That the cases bite was checked once with wrong-value (never wrong-address) changes of the library.  Not staging the halo
row below a workgroup's blocks turned 45 of the 81 items red (every marching case with more than one chunk, and the
drop-in cases); k_gn_update reading the other p buffer for the lagged update turned 22 red (every lean case whose
vertices move, at 25 and at 2 PCG iterations; with one iteration both buffers hold p_0, so those cannot tell).  Dropping
`|| x == W - 1` from the right-halo condition of pcg_a_march_body::issue changes nothing and no case can see it: under
`x + 1 < W` that clause is never true (the last in-image column has no right neighbour), and the compiled kernels are
instruction for instruction the same.  The lists of items are in the commit that added the file.
"""
import numpy as np
import pytest

import helpers
from arap_flow_amd import opt
from test_gpu_solve import _solve_opt

pytestmark = pytest.mark.gpu

S25, S1, S2 = (2, 2, 25), (2, 2, 1), (1, 2, 2)        # (numIter, nIterations, lIterations)

# name, W, H, mask of every slot, ARAPOPT_STREAM_A, phase A, phase B, (strips or 64x8 tiles in x, chunks or tiles in y),
# also the (1, 2, 2) schedule
CASES = [
    # the lean pair: N % 4 == 0 and at least half of the 32x8 tiles active; chunks of 28 rows
    ("68x30", 68, 30, ["full"], None, "march2", "b4_r", (2, 2), True),
    ("64x3", 64, 3, ["full"], None, "march2", "b4_r", (1, 1), False),
    ("4x1", 4, 1, ["full"], None, "march2", "b4_r", (1, 1), False),
    ("63x4", 63, 4, ["full"], None, "march2", "b4_r", (1, 1), False),
    ("64x28", 64, 28, ["full"], None, "march2", "b4_r", (1, 1), False),
    ("64x29", 64, 29, ["full"], None, "march2", "b4_r", (1, 2), False),
    ("132x57", 132, 57, ["full"], None, "march2", "b4_r", (3, 3), True),
    ("128x64-bands", 128, 64, ["bands"], None, "march2", "b4_r", (2, 3), True),
    ("192x84-bands", 192, 84, ["bands"], None, "march2", "b4_r", (3, 3), False),
    ("128x44-batch3", 128, 44, ["full", "noise", "empty"], None, "march2", "b4_r", (2, 2), False),
    # the other default pairs: chunks of 20 rows
    ("65x23", 65, 23, ["full"], None, "march", "b", (2, 2), True),
    ("129x20-a2", 129, 20, ["full"], "2", "march", "b4_lean", (3, 1), False),
    ("129x21-a2", 129, 21, ["full"], "2", "march", "b", (3, 2), False),
    ("130x41-blob", 130, 41, ["blob"], None, "march", "b", (3, 3), False),
    ("256x60-blob", 256, 60, ["blob"], None, "march", "b4_lean", (4, 3), False),
    ("128x44-noise-a2", 128, 44, ["noise"], "2", "march", "b4_lean", (2, 3), False),
    ("128x64-bands-a2", 128, 64, ["bands"], "2", "march", "b4_lean", (2, 4), True),
    ("1x1", 1, 1, ["full"], None, "march", "b", (1, 1), False),
    ("1x9", 1, 9, ["full"], None, "march", "b", (1, 1), False),
    ("9x1", 9, 1, ["full"], None, "march", "b", (1, 1), False),
    # the tiled grid kernel: 64x8 tiles
    ("65x23-a1", 65, 23, ["full"], "1", "grid", "b", (2, 3), True),
    ("132x57-a1", 132, 57, ["full"], "1", "grid", "b4_lean", (3, 8), True),
    ("128x64-bands-a1", 128, 64, ["bands"], "1", "grid", "b4_lean", (2, 8), True),
]


def _items():
    out = []
    for case in CASES:
        runs = [(S25, True), (S25, False), (S1, False)] + ([(S2, False)] if case[-1] else [])
        for sched, pins in runs:
            out.append(pytest.param(case, sched, pins, id="%s-%dx%dx%d-%s" % ((case[0],) + sched + ("pins" if pins else "free",))))
    return out


_inputs_cache, _oracle_cache = {}, {}


def _inputs(W, H):
    """constraints and the five masks (0 = active) of a shape, from default_rng(1000 W + H).  Handles are uniform in the
    frame; a target is its handle +- 3 in each coordinate, + 3 where - 3 would be negative (a negative target is an
    inactive constraint, and the one handle of a 1xN frame would then move nothing)."""
    if (W, H) not in _inputs_cache:
        rng = np.random.default_rng(1000 * W + H)
        n = min(30, max(1, W * H // 40))
        hx, hy = rng.integers(0, W, n), rng.integers(0, H, n)
        sx, sy = rng.integers(0, 2, n) * 2 - 1, rng.integers(0, 2, n) * 2 - 1
        tx = np.where(hx - 3 < 0, hx + 3, hx + 3 * sx)
        ty = np.where(hy - 3 < 0, hy + 3, hy + 3 * sy)
        cons = np.stack([hx, hy, tx, ty], -1).astype(np.int32)
        ys, xs = np.mgrid[0:H, 0:W]
        bands = np.zeros((H, W), bool)
        for y0 in range(8, H, 28):
            bands[y0:y0 + 8] = True
        bands[:, max(0, W // 2 - 3):W // 2 + 2] = True
        noise = rng.random((H, W)) < 0.35
        blob = ((xs - 0.45 * W) / (0.22 * W)) ** 2 + ((ys - 0.55 * H) / (0.30 * H)) ** 2 > 1.0
        masks = dict(full=np.zeros((H, W), bool), bands=bands, noise=noise, blob=blob, empty=np.ones((H, W), bool))
        masks = {k: np.where(m, 255, 0).astype(np.uint8) for k, m in masks.items()}
        for a in [cons] + list(masks.values()):
            a.setflags(write=False)
        _inputs_cache[(W, H)] = cons, masks
    return _inputs_cache[(W, H)]


def _oracle_frame(oracle, W, H, mask_name, sched, pins):
    """the oracle's (Offset, Angle, cost) of one slot: computed once per session, shared by the cases of a shape"""
    key = (W, H, mask_name, sched, pins)
    if key not in _oracle_cache:
        cons, masks = _inputs(W, H)
        O, A, costs = oracle.frame(masks[mask_name], cons, numIter=sched[0], nIterations=sched[1], lIterations=sched[2],
                                   dtype=np.float32, mode=1, trig=1, border_pins=pins)
        O.setflags(write=False); A.setflags(write=False)
        _oracle_cache[key] = O, A, float(costs[-1])
    return _oracle_cache[key]


@pytest.mark.parametrize("case,sched,pins", _items())
def test_stream_kernels_vs_oracle(monkeypatch, oracle, case, sched, pins):
    name, W, H, slots, knob, phase_a, phase_b, geom, _ = case
    cons, masks = _inputs(W, H)
    if knob is None:
        monkeypatch.delenv("ARAPOPT_STREAM_A", raising=False)
    else:
        monkeypatch.setenv("ARAPOPT_STREAM_A", knob)            # read when the state is created
    st, fs = opt.State(), None
    try:
        st.set_resident(False)
        fs = opt.FrameSolver(st, W, H, batch=len(slots))
        for b, m in enumerate(slots):
            fs.set_frame(b, masks[m], cons, border_pins=pins)
        fs.solve(len(slots), *sched)
        got = [fs.results(b, want_rgb=False) for b in range(len(slots))]
        stats = fs.stats()
    finally:
        if fs is not None:
            fs.close()
        st.close()
    # the case ran on the kernels it was written for
    assert stats["resident_launches"] == 0
    assert (stats["phase_a"], stats["phase_b"]) == (phase_a, phase_b), stats
    assert stats["a_args"] == geom + (-(-geom[0] * geom[1] // 8),), stats
    assert stats["lag"] == (sched[2] - 1 if phase_a == "march2" else -1), stats
    assert stats["lean_stream"] == (phase_a == "march2")
    ys, xs = np.mgrid[0:H, 0:W]
    rest = np.stack([xs, ys], -1).astype(np.float32)
    for b, m in enumerate(slots):
        O, A, cost = _oracle_frame(oracle, W, H, m, sched, pins)
        assert np.isfinite(O).all() and np.isfinite(A).all() and np.isfinite(cost), (name, m)
        if not pins and (masks[m] == 0).any():
            assert (O != rest).any(), (name, m)                 # the case computes something
        r = got[b]
        nO, nA = int((r["offset"] != O).sum()), int((r["angle"] != A).sum())
        print("%s slot %d (%s): differing floats Offset %d Angle %d, cost %r vs %r" % (name, b, m, nO, nA, r["cost"], cost))
        assert np.array_equal(r["offset"], O), (name, m, nO)
        assert np.array_equal(r["angle"], A), (name, m, nA)
        assert r["cost"] == cost, (name, m)


@pytest.mark.parametrize("lIter", [1, 25])
@pytest.mark.parametrize("W,H", [(65, 23), (68, 30)])
def test_drop_in_plans_on_the_march_pair_vs_oracle(oracle, W, H, lIter):
    """The Opt_* path with a pixel-grid UrShape and the resident kernel off takes k_pcg_a_march<5> with k_pcg_b (N odd) or
    k_pcg_b4_lean (N % 4 == 0), never the lean pair: two strips, the second one and four columns wide, a partial last
    chunk; a noise mask (quads that mix active and excluded vertices)."""
    pb = helpers.random_problem(W, H, seed=1000 * W + H, generic_urshape=False)
    Or, Ar, costs = oracle.solve(pb["O"], pb["A"], pb["U"], pb["C"], pb["M"], pb["wf"], pb["wr"], 2, lIter,
                                 dtype=np.float32, mode=1, trig=1)
    assert np.isfinite(Or).all() and np.isfinite(Ar).all() and np.isfinite(costs).all()
    assert (Or != pb["O"]).any()
    st = opt.State()
    try:
        st.set_resident(False)
        O, A, cost = _solve_opt(st, pb, 2, lIter)
    finally:
        st.close()
    print("%dx%d L=%d: differing floats Offset %d Angle %d" % (W, H, lIter, int((O != Or).sum()), int((A != Ar).sum())))
    assert np.array_equal(O, Or) and np.array_equal(A, Ar)
    assert cost == costs[-1]
