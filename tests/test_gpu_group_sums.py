"""The resident kernel's group sums add the same operands in the same order whatever instructions carry them: after a short
schedule its Offset / Angle bits equal those of the kernel-per-phase path (ARAPOPT_NO_RESIDENT=1), for eight DAVIS-shaped
854x480 frames (one group of 64 workgroups per XCD: group_sum), for eight frames of three segments, and for 1920x1080
frames (groups that span XCDs: group_sum_h / group_sum_x).  The instrumented build (ARAPOPT_STAMPS=1) computes the same bits and fills both
stamp tables."""
import numpy as np
import pytest

from arap_flow_amd import opt, synth

pytestmark = pytest.mark.gpu


def _solve(st, W, H, frames, sched):
    fs = opt.FrameSolver(st, W, H, batch=len(frames))
    for b, f in enumerate(frames):
        fs.set_frame(b, f["mask_red"], f["constraints"])
    fs.solve(len(frames), *sched)
    res = [fs.results(b, want_rgb=False) for b in range(len(frames))]
    launches = fs.stats()["resident_launches"]
    return fs, res, launches


def _frames(W, H, n, K, fd):
    return [synth.make_frame(W, H, seed=b, K=K, fd=fd) for b in range(n)]


@pytest.mark.parametrize("W,H,n,K,fd,sched", [
    (854, 480, 8, 1, 1, (1, 2, 60)),       # configs[1] shape: eight groups of 64 workgroups, one per XCD
    (854, 480, 8, 3, 2, (1, 2, 40)),       # three segments per frame
    (1920, 1080, 2, 3, 5, (1, 2, 30)),     # groups wider than one XCD
])
def test_resident_group_sums_equal_the_kernel_per_phase_path(monkeypatch, W, H, n, K, fd, sched):
    frames = _frames(W, H, n, K, fd)
    st = opt.State()
    try:
        fs, res, launches = _solve(st, W, H, frames, sched)
        fs.close()
        assert launches > 0
        monkeypatch.setenv("ARAPOPT_NO_RESIDENT", "1")     # read when a plan is created
        fs, ref, launches = _solve(st, W, H, frames, sched)
        fs.close()
        assert launches == 0
    finally:
        st.close()
    for a, b in zip(res, ref):
        assert np.array_equal(a["offset"], b["offset"]) and np.array_equal(a["angle"], b["angle"])
        assert a["cost"] == b["cost"]


def test_stamped_build_same_bits_and_both_tables(monkeypatch):
    W, H, L = 854, 480, 40
    frames = _frames(W, H, 8, 1, 1)
    st = opt.State()
    try:
        fs, res, _ = _solve(st, W, H, frames, (1, 1, L))
        fs.close()
        monkeypatch.setenv("ARAPOPT_STAMPS", "1")
        fs, stamped, launches = _solve(st, W, H, frames, (1, 1, L))
        assert launches > 0
        t1 = np.zeros((512, 16), np.uint64)
        t2 = np.zeros((512, 16), np.uint64)
        assert st.lib.ArapFlow_SolverStamps(fs.h, t1.ctypes.data) == 0
        assert st.lib.ArapFlow_SolverStampParts(fs.h, t2.ctypes.data) == 0
        fs.close()
    finally:
        st.close()
    for a, b in zip(res, stamped):
        assert np.array_equal(a["offset"], b["offset"]) and np.array_equal(a["angle"], b["angle"])
    used = t1[:, 0] > 0
    assert used.sum() > 0
    assert np.array_equal(t2[used, 8], t1[used, 5])                 # tiles, in both tables
    assert (t2[used, 12] == L).all()                                # PCG iterations of the launch
    assert (t2[used, 5] > 0).all() and (t2[used, 6] > 0).all()      # publish times of both sums
    assert (t2[used, 0] > 0).all() and (t2[used, 3] > 0).all()      # wave tree, lane tree
    # every batch slot's group deals all of its tiles: the tiles of its workgroups add up to the same count per slot as
    # the deal of an unstamped launch (ranks 0 .. wgs-1 once each)
    slot = (t2[used, 11] >> 32).astype(np.int64)
    rank = (t2[used, 11] & 0xffff).astype(np.int64)
    wgs = ((t2[used, 11] >> 16) & 0xffff).astype(np.int64)
    for g in np.unique(slot):
        m = slot == g
        assert sorted(rank[m].tolist()) == list(range(int(wgs[m][0])))
