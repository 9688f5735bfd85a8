"""The resident kernel's LDS cells (arap_resident.h): one 16-byte cell {px, py, cos, sin} per vertex of a halo'd tile, read
whole by phase A, its first half rewritten by the update phase; and the three-word staging of the border z, from which
the exporter forms even granules {z_x, low half of z_y} and odd ones {z_alpha, high half of z_y}.  Neither changes the
value of an operation or an order of additions, so every case wants the same BITS -- Offset, Angle and cost -- from the resident
path as dealt (flat), with ARAPOPT_RES_SUMS=any and from the kernel-per-phase path (ArapFlow_SetResident(state, 0)); one
case is also held against the float32 CPU oracle.

Shapes: 160x96 (full, rows88, thin, holes), 64x64 and 150x90 (right tiles 22 columns wide, last band 2 rows high: cells
beyond the image stay zero); slot counts either side of the gates that decide whether the own cell is read from LDS
(1, 6, 7, 8, 9), launches with more slots than any workgroup has tiles among them; PCG loops of 1, 2 and 3 iterations and
a schedule of (1, 2, 40); deals in which a thread owns 0-1, 2 and 3 halo entries; borders shared by two workgroups (the
border z travels through the granules) and by two slots of one workgroup; handles on tile corners and borders."""
import ctypes

import numpy as np
import pytest

import resident_cells_masks as masks
from arap_flow_amd import capi, opt

pytestmark = pytest.mark.gpu

_cache = {}
W, H = masks.W, masks.H


def _frames():
    if "frames" not in _cache:
        _cache["frames"] = masks.frames_160x96()
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
    """results of one solve of `frames` (slots 0 ..), the flavour its launches reported, launches per step, and the most
    tiles any workgroup held.  `way`: "flat" (as dealt), "any" (ARAPOPT_RES_SUMS=any) or "two" (kernel-per-phase path).
    The environment is read when the state and its plans are made."""
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
        most = None
        if way != "two":
            wd, nt = _widths(frames, w, h)
            most = max(-(-n // g) for n, g in zip(nt, wd))
        fs.close()
    finally:
        st.close()
        for k in ("ARAPOPT_RES_SUMS", "ARAPOPT_RES_NS", "ARAPOPT_RES_GROUPS"):
            monkeypatch.delenv(k, raising=False)
    return res, s["resident_sums"], s["resident_launches_per_step"], most


def _reference(key, monkeypatch, w, h, frames, sched):
    """the kernel-per-phase solve of a case: computed once, shared by every case that needs it, never modified"""
    if key not in _cache:
        res, sums, per_step, _ = _run(monkeypatch, w, h, frames, sched, "two")
        assert sums == "" and per_step == 0
        for o, a, _ in res:
            o.setflags(write=False)
            a.setflags(write=False)
            assert np.isfinite(o).all() and np.isfinite(a).all()
        _cache[key] = res
    return _cache[key]


def _same_bits(got, ref):
    assert len(got) == len(ref)
    for (o, a, c), (ro, ra, rc) in zip(got, ref):
        assert np.array_equal(o, ro) and np.array_equal(a, ra)
        assert c == rc


def _both_flavours(monkeypatch, key, w, h, frames, sched, ns=0, groups=0, most=None):
    ref = _reference(key, monkeypatch, w, h, frames, sched)
    for way in ("flat", "any"):
        res, sums, per_step, m = _run(monkeypatch, w, h, frames, sched, way, ns=ns, groups=groups)
        assert sums == way and per_step == 1
        if most is not None:
            assert m == most, m
        _same_bits(res, ref)
    return ref


def _moved(ref, w, h):
    return np.abs(ref[0][0] - np.stack(np.mgrid[0:h, 0:w][::-1], -1)).max() > 0.0


@pytest.mark.parametrize("ns", [1, 6, 7, 8, 9])
def test_slot_counts_on_holes_and_thin(monkeypatch, ns):
    """either side of the gates that keep the own p and the own (cos, sin) in registers: up to 7 slots the own cell is never
    read, at 8 and 9 it is one 16-byte read; the solves need fewer slots than 6 .. 9: slots without a tile.  `holes` has
    degrees 0 .. 4, excluded neighbours on every side (never-written cells), handles on tile corners and on each border"""
    f = _frames()
    ref = _both_flavours(monkeypatch, "holes+thin L3", W, H, [f["holes"], f["thin"]], (1, 2, 3), ns=ns)
    assert _moved(ref, W, H)


@pytest.mark.parametrize("ns", [7, 8])
@pytest.mark.parametrize("L", [1, 2])
def test_short_loops(monkeypatch, L, ns):
    """one iteration: phase A reads the prologue's cells only; two: every cell's first half has been rewritten once"""
    f = _frames()
    ref = _both_flavours(monkeypatch, "holes+thin L%d" % L, W, H, [f["holes"], f["thin"]], (1, 2, L), ns=ns)
    assert _moved(ref, W, H)                                                            # (even one iteration moves something)


def test_schedule_1_2_40(monkeypatch):
    f = _frames()
    _both_flavours(monkeypatch, "full+rows88 L40", W, H, [f["full"], f["rows88"]], (1, 2, 40))


@pytest.mark.parametrize("L", [1, 3])
def test_one_tile_per_workgroup(monkeypatch, L):
    """one solve alone in its bin: 64 workgroups for 60 tiles, one tile (80 halo cells at most: a thread owns 0 or 1) or none
    each -- every shared border lies between two workgroups, its z travels through the granules"""
    f = _frames()
    _both_flavours(monkeypatch, "full L%d" % L, W, H, [f["full"]], (1, 2, L), most=1)


def test_four_tiles_per_workgroup(monkeypatch):
    """16 workgroups, four tiles each (the last ones three): 256 < halo cells <= 320, two entries per thread; borders between
    slots of one workgroup and between workgroups"""
    f = _frames()
    _both_flavours(monkeypatch, "full L3", W, H, [f["full"]], (1, 2, 3), groups=32, most=4)


@pytest.mark.parametrize("L", [2, 3])
def test_seven_tiles_per_workgroup(monkeypatch, L):
    """55 tiles for 8 workgroups: seven each (one has six); a workgroup whose seven tiles lie inside the mask has
    7 x 80 - 16 = 544 halo cells: threads 0 .. 31 own three"""
    f = _frames()
    _both_flavours(monkeypatch, "rows88 L%d" % L, W, H, [f["rows88"]], (1, 2, L), groups=64, most=7)


@pytest.mark.parametrize("ns,groups,most", [(0, 0, 1), (7, 32, 4), (0, 64, 8)])
def test_partial_tiles_150x90(monkeypatch, ns, groups, most):
    """right tiles 22 columns wide, last band 2 rows high: the cells beyond the image are never written and read as zeros;
    one tile per workgroup; sixteen workgroups of four tiles in the 7-slot kernel (own cell in registers); eight workgroups
    of seven or eight tiles (60 tiles) in the 8-slot kernel (own cell read from LDS)"""
    c = masks.frame_150x90()
    ref = _both_flavours(monkeypatch, "150x90 L3", c["w"], c["h"], [c["frame"]], (1, 2, 3), ns=ns, groups=groups, most=most)
    assert _moved(ref, c["w"], c["h"])


@pytest.mark.parametrize("groups,most", [(0, 1), (256, 8)])
def test_64x64_full(monkeypatch, groups, most):
    """16 tiles: one per workgroup, and eight in each of two workgroups (the 8-slot kernel with every slot in use)"""
    c = masks.frame_64x64()
    _both_flavours(monkeypatch, "64x64 full L3", c["w"], c["h"], [c["frame"]], (1, 2, 3), groups=groups, most=most)


def test_borders_inside_one_workgroup_and_oracle(monkeypatch):
    """7 tiles in one workgroup (ARAPOPT_RES_GROUPS=512): both sides of every shared border are slots of the same workgroup;
    handles on a tile corner and on a left, top, right and bottom border; and the CPU oracle"""
    from oracle import oracle as orc
    c = masks.frame_seven_tiles()
    w, h, frame = c["w"], c["h"], c["frame"]
    ref = _both_flavours(monkeypatch, "64x64 seven", w, h, [frame], (1, 2, 50), groups=512, most=7)
    O, A, costs = orc.frame(frame["mask_red"], frame["constraints"], numIter=1, nIterations=2, lIterations=50, dtype=np.float32,
                            mode=1, trig=1)
    act = frame["mask_red"] == 0
    grid = np.stack(np.mgrid[0:h, 0:w][::-1], -1).astype(np.float32)
    err = np.sqrt(((ref[0][0] - O)[act] ** 2).sum() / ((O - grid)[act] ** 2).sum())
    assert err < 1e-4, err                                                             # (the bound of smoke())
