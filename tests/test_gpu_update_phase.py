"""The update phase of the resident kernel (p = z + beta p on the own cells and on the halo cells, delta += alpha p) at the
shapes it branches on: the number of halo entries a thread holds (three, two, one, none), partial and ragged tiles, the
halo table in registers (up to 8 tile slots) and in LDS (9 slots), the instrumented build.  Every case solves a short
schedule through the resident path and through the kernel-per-phase path (ARAPOPT_NO_RESIDENT=1) and wants the same bits;
the two smallest shapes are also held against the float32 CPU oracle.  The stamp table of the last launch tells what a
shape really covered (tiles and halo cells per workgroup), so that a later change of the deal cannot hollow the cases out.

A solve alone in a launch is widened to 64 workgroups (host_resident.h: resident_deal), hence the tiles per workgroup:
    448x256 full mask    448 tiles  7 per workgroup (the flagship's 7-slot kernel), up to 560 halo cells: three entries
    448x160 full mask    280 tiles  4-5 per workgroup, up to 400 halo cells: two entries
    448x256 DAVIS mask   129 tiles  2-3 ragged tiles per workgroup, at most 240 halo cells: one entry
    96x40 full mask       15 tiles  workgroups with one tile next to workgroups with none (no halo at all)
"""
import numpy as np
import pytest

from arap_flow_amd import opt, synth

pytestmark = pytest.mark.gpu

SCHED = (1, 2, 40)
SHAPES = {
    "full448x256": (448, 256, True),
    "full448x160": (448, 160, True),
    "davis448x256": (448, 256, False),
    "full96x40": (96, 40, True),
}
_frames, _ref = {}, {}


def _frame(name):
    if name not in _frames:
        W, H, full = SHAPES[name]
        _frames[name] = synth.make_frame(W, H, seed=0, full_mask=full)
    return _frames[name]


def _solve(name, stamps=False):
    """one frame, alone in its launches; the environment is read when the plan is made (FrameSolver)"""
    W, H, _ = SHAPES[name]
    f = _frame(name)
    st = opt.State()
    try:
        fs = opt.FrameSolver(st, W, H, batch=1)
        fs.set_frame(0, f["mask_red"], f["constraints"])
        fs.solve(1, *SCHED)
        r = fs.results(0, want_rgb=False)
        launches = fs.stats()["resident_launches"]
        table = None
        if stamps:
            table = np.zeros((512, 16), np.uint64)
            assert st.lib.ArapFlow_SolverStamps(fs.h, table.ctypes.data) == 0
        fs.close()
    finally:
        st.close()
    return {"offset": r["offset"].copy(), "angle": r["angle"].copy(), "cost": r["cost"]}, launches, table


def _reference(name, monkeypatch):
    """the kernel-per-phase solve of a shape: computed once, shared by every case of that shape, never modified"""
    if name not in _ref:
        monkeypatch.setenv("ARAPOPT_NO_RESIDENT", "1")
        ref, launches, _ = _solve(name)
        monkeypatch.delenv("ARAPOPT_NO_RESIDENT")
        assert launches == 0
        for a in (ref["offset"], ref["angle"]):
            a.setflags(write=False)
        _ref[name] = ref
    return _ref[name]


def _same_bits(got, ref):
    assert np.array_equal(got["offset"], ref["offset"]) and np.array_equal(got["angle"], ref["angle"])
    assert got["cost"] == ref["cost"]


@pytest.mark.parametrize("name,ns", [
    ("full448x256", 0), ("full448x160", 0), ("davis448x256", 0), ("full96x40", 0),
    ("full448x256", 8), ("full448x256", 9),        # 9 slots: the halo table is read from LDS
    ("full96x40", 8), ("full96x40", 9),
])
def test_update_phase_equals_the_kernel_per_phase_path(monkeypatch, name, ns):
    ref = _reference(name, monkeypatch)
    if ns:
        monkeypatch.setenv("ARAPOPT_RES_NS", str(ns))
    got, launches, _ = _solve(name)
    assert launches > 0
    _same_bits(got, ref)


@pytest.mark.parametrize("name", ["full96x40", "davis448x256"])
def test_two_smallest_shapes_against_the_float32_oracle(oracle, name):
    """Offset and Angle bit for bit, as everywhere a short schedule is held against the float32 oracle (mode=1, trig=1: the
    kernel's operation list); the cost is a sum over the frame formed in another order: 1e-6 relative, as in T3."""
    f = _frame(name)
    got, launches, _ = _solve(name)
    assert launches > 0
    O, A, costs = oracle.frame(f["mask_red"], f["constraints"], numIter=SCHED[0], nIterations=SCHED[1],
                               lIterations=SCHED[2], dtype=np.float32, mode=1, trig=1)
    assert np.array_equal(got["offset"], O) and np.array_equal(got["angle"], A)
    assert abs(got["cost"] - costs[-1]) <= 1e-6 * costs[-1]


@pytest.mark.parametrize("name", list(SHAPES))
def test_stamped_build_same_bits_and_what_the_shape_covers(monkeypatch, name):
    ref = _reference(name, monkeypatch)
    monkeypatch.setenv("ARAPOPT_STAMPS", "1")
    got, launches, t = _solve(name, stamps=True)
    assert launches > 0
    _same_bits(got, ref)
    used = t[:, 0] > 0                                      # workgroups that ran the loop (phase A ticks)
    tiles = t[used, 5].astype(np.int64)
    halo = (t[used, 6] & np.uint64(0xffffffff)).astype(np.int64)
    print(name, "workgroups", int(used.sum()), "tiles", tiles.min(), tiles.max(), "halo cells", halo.min(), halo.max())
    assert used.sum() == 64                                 # a lone solve is widened to a whole XCD's workgroups
    if name == "full448x256":
        assert tiles.sum() == 448 and tiles.min() == 7 and tiles.max() == 7
        assert (halo[tiles == 7] > 512).any() and halo.max() <= 560          # three entries per thread
    elif name == "full448x160":
        assert tiles.sum() == 280 and tiles.min() == 4 and tiles.max() == 5
        assert 256 < halo.max() <= 512                                       # two entries, the third never used
    elif name == "davis448x256":
        assert tiles.sum() == 129 and tiles.min() == 2 and tiles.max() == 3
        assert 0 < halo.max() <= 256                                         # one entry
    else:
        assert tiles.sum() == 15 and tiles.max() == 1 and tiles.min() == 0
        assert (halo[tiles == 0] == 0).all() and (halo[tiles == 1] > 0).any()
