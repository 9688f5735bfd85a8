"""The memory traffic around the resident kernel's second group sum (arap_resident.h): the border z that waves 1-3 export
under the sum, trip by trip of 192 threads, and the neighbours' z that every thread fetches behind it for its halo entries --
one 16-byte load per entry (both granules, each tag checked on its own), in the first look and in the bounded re-look.
Nothing here changes an operation, an operand or an order of additions, so every case wants the same BITS -- Offset, Angle
and cost -- from the resident path as dealt (flat), with ARAPOPT_RES_SUMS=any and from the kernel-per-phase path
(ArapFlow_SetResident(state, 0)); one case is also held against the float32 CPU oracle.  No launch may give up a wait
(ArapFlow_ResidentFailed == 0): a tag that never arrives, or a barrier one wave misses, ends there.

Export trip counts (192 exporting threads, 160 granules per tile; masks of 160x96 and 64x64):

    tiles per workgroup   granules   deal
    1                     160        60 tiles for 64 workgroups: fewer granules than exporting threads; workgroups with no tile
    2                     320        60 for 32: second trip partial
    4                     640        60 for 16
    6                     960        48 for 8: exactly five full trips
    7                     1 120      55 for 8 (one workgroup has six: fewer tiles than slots), 7 for 1: last trip partial
    9                     1 440      36 for 4: the 9-slot kernel (its halo entries come from the LDS table)

Threads own 0 or 1 halo entries (one tile per workgroup), 2 (four tiles) and 3 (seven and nine tiles); groups of 1, 4, 8, 16, 32
and 64 workgroups; PCG loops of 1 (the loads behind the second sum are issued and never looked at), 2, 3 and 30 iterations;
launches with more slots than any workgroup has tiles (ARAPOPT_RES_NS)."""
import ctypes

import numpy as np
import pytest

from arap_flow_amd import capi, opt, synth

pytestmark = pytest.mark.gpu

_cache = {}
W, H = 160, 96


def _frame_from_labels(labels, seed):
    return dict(mask_red=np.where(labels != 0, 0, 255).astype(np.uint8), constraints=synth.make_constraints(labels, seed))


def _frames():
    """160x96 (five tile columns, twelve bands): the full mask (60 tiles), rows 0 .. 87 (55), nine bands and three tiles of the
    tenth (48), seven bands and one tile of the eighth (36)"""
    if "frames" not in _cache:
        ys, xs = np.mgrid[0:H, 0:W]
        t48 = ((ys < 72) | ((ys < 80) & (xs < 96))).astype(np.int32)
        t36 = ((ys < 56) | ((ys < 64) & (xs < 32))).astype(np.int32)
        _cache["frames"] = dict(full=_frame_from_labels(np.ones((H, W), np.int32), 1),
                                rows88=_frame_from_labels((ys < 88).astype(np.int32), 5),
                                t48=_frame_from_labels(t48, 6), t36=_frame_from_labels(t36, 7))
    return _cache["frames"]


def _widths(frames, w, h):
    """group sizes the host deals these solves and their tile counts (pure host functions of the library; the forced deal
    is read per call)"""
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
    return [int(tab[0][tab[0][:, 0] == b][0, 2]) for b in range(len(frames))], nt


def _run(monkeypatch, w, h, frames, sched, way, ns=0, groups=0):
    """results of one solve of `frames` (slots 0 ..), the flavour its launches reported, launches per step, the most tiles
    any workgroup held and the group sizes.  `way`: "flat" (as dealt), "any" (ARAPOPT_RES_SUMS=any) or "two" (kernel-per-phase
    path).  The environment is read when the state and its plans are made."""
    if way == "any":
        monkeypatch.setenv("ARAPOPT_RES_SUMS", "any")
    if ns:
        monkeypatch.setenv("ARAPOPT_RES_NS", str(ns))
    if groups:
        monkeypatch.setenv("ARAPOPT_RES_GROUPS", str(groups))
    st = opt.State()
    try:
        st.set_resident(way != "two")
        fs = opt.FrameSolver(st, w, h, batch=len(frames))
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
        most, wd = None, None
        if way != "two":
            wd, nt = _widths(frames, w, h)
            most = max(-(-n // g) for n, g in zip(nt, wd))
        fs.close()
    finally:
        st.close()
        for k in ("ARAPOPT_RES_SUMS", "ARAPOPT_RES_NS", "ARAPOPT_RES_GROUPS"):
            monkeypatch.delenv(k, raising=False)
    return res, s["resident_sums"], s["resident_launches_per_step"], most, wd


def _reference(key, monkeypatch, w, h, frames, sched):
    """the kernel-per-phase solve of a case: computed once, shared by every case that needs it, never modified"""
    if key not in _cache:
        res, sums, per_step, _, _ = _run(monkeypatch, w, h, frames, sched, "two")
        assert sums == "" and per_step == 0
        for o, a, _ in res:
            o.setflags(write=False)
            a.setflags(write=False)
        _cache[key] = res
    return _cache[key]


def _same_bits(got, ref):
    assert len(got) == len(ref)
    for (o, a, c), (ro, ra, rc) in zip(got, ref):
        assert np.array_equal(o, ro) and np.array_equal(a, ra)
        assert c == rc


def _three_ways(monkeypatch, key, w, h, frames, sched, ns=0, groups=0, most=None, wgs=None):
    ref = _reference(key, monkeypatch, w, h, frames, sched)
    for way in ("flat", "any"):
        res, sums, per_step, m, wd = _run(monkeypatch, w, h, frames, sched, way, ns=ns, groups=groups)
        assert sums == way and per_step == 1
        if most is not None:
            assert m == most, m
        if wgs is not None:
            assert wd == [wgs] * len(frames), wd
        _same_bits(res, ref)
    return ref


# (mask, forced groups, workgroups per group, most tiles per workgroup)
_DEALS = {1: ("full", 8, 64, 1), 2: ("full", 16, 32, 2), 4: ("full", 32, 16, 4), 6: ("t48", 64, 8, 6),
          7: ("rows88", 64, 8, 7), 9: ("t36", 128, 4, 9)}


@pytest.mark.parametrize("tiles", [1, 2, 4, 6, 7, 9])
def test_export_trip_counts(monkeypatch, tiles):
    """every trip count of the export, three iterations (the carried state is read twice)"""
    name, groups, wgs, most = _DEALS[tiles]
    ref = _three_ways(monkeypatch, "%s L3" % name, W, H, [_frames()[name]], (1, 2, 3), groups=groups, most=most, wgs=wgs)
    assert np.abs(ref[0][0] - np.stack(np.mgrid[0:H, 0:W][::-1], -1)).max() > 0.0       # (the solve moves something)


@pytest.mark.parametrize("L", [1, 2, 30])
@pytest.mark.parametrize("tiles", [1, 7])
def test_loop_lengths(monkeypatch, tiles, L):
    """one iteration: the loads issued behind the second sum are never looked at; two: one update phase; thirty: tags far
    from their first values.  Groups of 64 workgroups (0 or 1 halo entries per thread) and of 8 (3 entries)"""
    name, groups, wgs, most = _DEALS[tiles]
    _three_ways(monkeypatch, "%s L%d" % (name, L), W, H, [_frames()[name]], (1, 2, L), groups=groups, most=most, wgs=wgs)


@pytest.mark.parametrize("ns", [8, 9])
def test_more_slots_than_tiles(monkeypatch, ns):
    """four tiles per workgroup (two halo entries per thread) in the 8- and 9-slot kernels: the entries in registers and
    from the LDS table, slots without a tile"""
    _three_ways(monkeypatch, "full L3", W, H, [_frames()["full"]], (1, 2, 3), ns=ns, groups=32, most=4, wgs=16)


def test_two_solves_share_a_launch(monkeypatch):
    """two groups of 8 workgroups side by side (seven and six tiles per workgroup): each reads its own solve's export"""
    f = _frames()
    _three_ways(monkeypatch, "rows88+t48 L3", W, H, [f["rows88"], f["t48"]], (1, 2, 3), groups=64, most=7, wgs=8)


def test_one_workgroup_and_oracle(monkeypatch):
    """64x64, a 64x24 block and a 32x8 one below it: 7 tiles, one workgroup holds them all (a group of one: its sums see
    nobody else's granules, its halo entries are its own export); and the CPU oracle"""
    from oracle import oracle as orc
    w = h = 64
    mask = np.full((h, w), 255, np.uint8)
    mask[16:40, :] = 0
    mask[40:48, :32] = 0
    cons = np.asarray([(16, 20, 19, 22), (48, 20, 45, 23), (16, 44, 19, 41), (40, 36, 43, 38)], np.int32)
    frame = dict(mask_red=mask, constraints=cons)
    ref = _three_ways(monkeypatch, "64x64 seven", w, h, [frame], (1, 2, 50), groups=512, most=7, wgs=1)
    O, A, costs = orc.frame(mask, cons, numIter=1, nIterations=2, lIterations=50, dtype=np.float32, mode=1, trig=1)
    act = mask == 0
    grid = np.stack(np.mgrid[0:h, 0:w][::-1], -1).astype(np.float32)
    err = np.sqrt(((ref[0][0] - O)[act] ** 2).sum() / ((O - grid)[act] ** 2).sum())
    assert err < 1e-4, err                                                             # (the bound of smoke())
