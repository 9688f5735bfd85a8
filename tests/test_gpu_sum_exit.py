"""The exits of the resident kernel's two group sums (arap_resident.h: group_sum's one-trip sweep -- the exit test, the
registers preset for lanes that do not look, one 16-byte load per sweep through a descriptor of the group's granules -- the
publish under lane masks, phase B's accumulator, the branch-free test of the z tags): every case wants the same BITS (Offset,
Angle, cost) from the flat flavour, from the forced `any` flavour (ARAPOPT_RES_SUMS=any) and from the kernel-per-phase path.
No launch may give up a wait (ArapFlow_ResidentFailed == 0): a launch that does is redone on the kernel-per-phase path and
would give the reference's bits, so without that assertion a wrong exit test, lane mask, descriptor range or a load hoisted
out of the spin would pass, only slower.  Every case also asserts the group size it is about (ArapFlow_ResidentDeal).

What the cases reach (frames of at most 128x48, one of 128x64):
  * groups of 1, 2 and 64 workgroups, and 4 (ARAPOPT_RES_GROUPS: equal groups, so its sizes divide 512): a group of 1 has 63
    lanes at or beyond `wgs` and no lane that looks; 64 is the full one-trip sweep and leaves most workgroups without a tile,
  * a group of 3, which the packed deal gives each of 136 one-workgroup solves (64x32, 8 tiles) in one launch: 17 per XCD
    bin, 64 / 17 = 3 -- an odd size that divides neither 64 nor 512, so granule pairs and the descriptor's end stand at
    multiples of 48 bytes, with the 136 groups' granules packed back to back,
  * L = 1, 2, 3 PCG iterations (1 leaves the loop before the update phase, 3 runs it twice),
  * the 1-, 7-, 8- and 9-slot instantiations (ARAPOPT_RES_NS),
  * a batch with an empty slot,
  * a frame whose constraints equal its rest pose: r = 0, rho_0 = 0 and sigma = 0, so alpha and beta must be exactly 0,
  * 128x64 in groups of 4: the workgroups of ranks 1 and 2 hold two whole bands with neighbours above and below (608 halo
    cells: threads with an entry in all three positions), ranks 0 and 3 fewer than 512 (threads with two or one).
"""
import ctypes

import numpy as np
import pytest

from arap_flow_amd import capi, opt, synth

pytestmark = pytest.mark.gpu

_cache = {}


def _frame(W, H, kind, seed=1):
    key = (W, H, kind, seed)
    if key not in _cache:
        ys, xs = np.mgrid[0:H, 0:W]
        if kind == "rest":                                  # every handle stays where it is
            f = dict(mask_red=np.zeros((H, W), np.uint8),
                     constraints=np.asarray([(x, y, x, y) for y in range(8, H, 16) for x in range(8, W, 16)], np.int32))
        elif kind == "none":
            f = dict(mask_red=np.full((H, W), 255, np.uint8), constraints=np.zeros((0, 4), np.int32))
        else:
            if kind == "full":
                labels = np.ones((H, W), np.int32)
            else:                                           # "blob": an ellipse that touches no border
                labels = (((xs - W / 2.0) / (W * 0.4)) ** 2 + ((ys - H / 2.0) / (H * 0.4)) ** 2 <= 1.0).astype(np.int32)
            f = dict(mask_red=np.where(labels != 0, 0, 255).astype(np.uint8), constraints=synth.make_constraints(labels, seed))
        _cache[key] = f
    return _cache[key]


def _widths(frames, w, h):
    """group sizes the host deals these solves (pure host functions of the library; the forced deal is read per call, so
    the environment must be the solve's)"""
    lib = capi.load()
    nt = []
    for f in frames:
        org = np.zeros(4608, np.int32)
        bx = np.zeros((h + 7) // 8, np.int32)
        nt.append(lib.ArapFlow_ResidentTiles(np.ascontiguousarray(f["mask_red"]).ctypes.data, w, h, 1,
                                             org.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 4608,
                                             bx.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
    t = np.asarray(nt, np.int32)
    tab = np.full((1, 512, 4), -7, np.int32)
    n = lib.ArapFlow_ResidentDeal(t.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), len(t),
                                  tab.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 1)
    assert n == 1
    return [int(tab[0][tab[0][:, 0] == b][0, 2]) if (tab[0][:, 0] == b).any() else 0 for b in range(len(frames))]


def _run(monkeypatch, W, H, frames, sched, way, groups=0, ns=0, wgs=None):
    if way == "any":
        monkeypatch.setenv("ARAPOPT_RES_SUMS", "any")
    if groups:
        monkeypatch.setenv("ARAPOPT_RES_GROUPS", str(groups))
    if ns:
        monkeypatch.setenv("ARAPOPT_RES_NS", str(ns))
    st = opt.State()
    try:
        st.set_resident(way != "two")
        fs = opt.FrameSolver(st, W, H, batch=len(frames))
        for b, f in enumerate(frames):
            fs.set_frame(b, f["mask_red"], f["constraints"])
        fs.solve(len(frames), *sched)
        res = []
        for b in range(len(frames)):
            r = fs.results(b, want_rgb=False)
            res.append((r["offset"].copy(), r["angle"].copy(), r["cost"]))
        s = fs.stats()
        assert (s["resident_launches"] > 0) == (way != "two"), s
        assert st.lib.ArapFlow_ResidentFailed(st.handle) == 0            # no wait gave up, no launch was redone
        if way != "two":
            assert s["resident_sums"] == way, s
            if wgs is not None:                                           # the group size the case is about was dealt
                wd = _widths(frames, W, H)
                assert wd == wgs, wd
        fs.close()
    finally:
        st.close()
        for k in ("ARAPOPT_RES_SUMS", "ARAPOPT_RES_GROUPS", "ARAPOPT_RES_NS"):
            monkeypatch.delenv(k, raising=False)
    return res


def _reference(key, monkeypatch, W, H, frames, sched):
    """the kernel-per-phase solve of a case: computed once, shared, never modified"""
    if key not in _cache:
        res = _run(monkeypatch, W, H, frames, sched, "two")
        for o, a, _ in res:
            o.setflags(write=False)
            a.setflags(write=False)
        _cache[key] = res
    return _cache[key]


def _check(monkeypatch, key, W, H, frames, sched, **kw):
    ref = _reference(key, monkeypatch, W, H, frames, sched)
    for way in ("flat", "any"):
        got = _run(monkeypatch, W, H, frames, sched, way, **kw)
        assert len(got) == len(ref)
        for (o, a, c), (ro, ra, rc) in zip(got, ref):
            assert np.array_equal(o, ro) and np.array_equal(a, ra), (way, kw)
            assert c == rc, (way, kw, c, rc)
    return ref


# (workgroups per group, frame): the forced deal wants 512 / groups >= ceil(tiles / 9)
_GROUPS = {1: (64, 32), 2: (128, 32), 4: (128, 48), 64: (128, 48)}


@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("wgs", [1, 2, 4, 64])
def test_group_sizes_and_iteration_counts(monkeypatch, wgs, L):
    W, H = _GROUPS[wgs]
    ref = _check(monkeypatch, ("groups", W, H, L), W, H, [_frame(W, H, "full")], (1, 2, L), groups=512 // wgs, wgs=[wgs])
    ys, xs = np.mgrid[0:H, 0:W]
    assert np.abs(ref[0][0] - np.stack([xs, ys], -1)).max() > 1e-3             # (the handles moved something)


@pytest.mark.parametrize("L", [1, 3])
def test_groups_of_three(monkeypatch, L):
    """136 solves of 8 tiles in one launch of the packed deal: 17 to a bin, each a group of 64 / 17 = 3 workgroups holding
    3, 3 and 2 tiles"""
    W, H, n = 64, 32, 136
    frames = [_frame(W, H, "full", 1 + b % 4) for b in range(n)]
    _check(monkeypatch, ("three", L), W, H, frames, (1, 2, L), wgs=[3] * n)


@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("ns", [1, 7, 8, 9])
def test_slot_counts(monkeypatch, ns, L):
    W, H = 128, 48
    frames = [_frame(W, H, "full"), _frame(W, H, "blob", 2)]
    _check(monkeypatch, ("slots", L), W, H, frames, (1, 2, L), ns=ns, wgs=[64, 64])


def test_batch_with_an_empty_slot(monkeypatch):
    W, H = 128, 48
    frames = [_frame(W, H, "full"), _frame(W, H, "none"), _frame(W, H, "blob", 2)]
    ref = _check(monkeypatch, "empty slot", W, H, frames, (1, 2, 3))
    assert ref[1][2] == 0.0


@pytest.mark.parametrize("wgs", [1, 64])
def test_rest_pose_gives_exact_zeros(monkeypatch, wgs):
    """r = 0: rho_0 = 0 and sigma = 0, so alpha = beta = 0 (the guards), delta = 0 and the unknowns stay bit for bit"""
    W, H = _GROUPS[wgs]
    ref = _check(monkeypatch, ("rest", W, H), W, H, [_frame(W, H, "rest")], (1, 2, 3), groups=512 // wgs, wgs=[wgs])
    ys, xs = np.mgrid[0:H, 0:W]
    assert np.array_equal(ref[0][0], np.stack([xs, ys], -1).astype(np.float32))
    assert not ref[0][1].any() and ref[0][2] == 0.0


@pytest.mark.parametrize("L", [2, 3])
def test_halo_entries_in_one_two_and_three_positions(monkeypatch, L):
    W, H = 128, 64
    _check(monkeypatch, ("halo3", L), W, H, [_frame(W, H, "full")], (1, 2, L), groups=128, wgs=[4])
