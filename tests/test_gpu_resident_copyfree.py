"""The resident kernel's loop-carried registers (arap_resident.h): the own search direction updated in place, the own
(cos, sin) read once in the prologue (up to 7 slots), and the p of a thread's halo cells carried from one iteration's store
to the next iteration's update (up to 7 slots in the flat flavour, 6 in the other).  None of them changes an operation, an
operand or an order of additions, so every case wants the same BITS -- Offset, Angle and cost -- from the resident path as
dealt (flat), with ARAPOPT_RES_SUMS=any and from the kernel-per-phase path (ArapFlow_SetResident(state, 0)); one case is
also held against the float32 CPU oracle.

Shapes (160x96 and 64x64): slot counts either side of every gate (1, 4, 6, 7, 8, 9); PCG loops of 1 iteration (the epilogue's
delta += alpha p takes the prologue's p, no halo register is ever rewritten), 2 (one in-place update) and 3 (the carried halo
p is read twice); deals in which a thread owns 0 or 1 halo entries (64 workgroups, at most one tile each: 80 halo cells for
256 threads), 2 (four tiles per workgroup) and 3 (seven tiles, more than 512 halo cells); the `holes` mask (vertices of
degree 0 .. 4 in one tile, handles on tile corners and borders: halo cells that start from a non-zero p0 and from zero);
launches with more slots than any workgroup has tiles."""
import ctypes

import numpy as np
import pytest

from arap_flow_amd import capi, opt, synth

pytestmark = pytest.mark.gpu

_cache = {}
W, H = 160, 96


def _frame_from_labels(labels, seed, extra=()):
    cons = synth.make_constraints(labels, seed)
    if len(extra):
        cons = np.concatenate([cons.reshape(-1, 4), np.asarray(extra, np.int32)]).astype(np.int32)
    return dict(mask_red=np.where(labels != 0, 0, 255).astype(np.uint8), constraints=cons)


def _frames():
    """160x96: the full mask (60 tiles), `rows88` (rows 0 .. 87: 55 tiles, seven to a workgroup when eight share them), a
    blob with a one-vertex-wide stripe, and `holes`: one-vertex-wide vertical and horizontal stripes, a block with
    single-vertex holes, isolated vertices; its bands start at x = 8, and it has handles on corners and borders of its
    tiles next to the lattice ones (the masks of test_gpu_resident_regs.py)"""
    if "frames" not in _cache:
        ys, xs = np.mgrid[0:H, 0:W]
        thin = (((xs - 50) / 30.0) ** 2 + ((ys - 48) / 25.0) ** 2 <= 1.0).astype(np.int32)
        thin[10:71, 100] = 1
        rows88 = (ys < 88).astype(np.int32)
        holes = np.zeros((H, W), np.int32)
        holes[4:45, 8:72] = (xs[4:45, 8:72] % 2 == 0)                                   # vertical stripes: 2 edges, 1 at the ends
        holes[50:65, 8:72] = (ys[50:65, 8:72] % 2 == 0)                                 # horizontal stripes
        holes[4:61, 72:151] = ~((xs[4:61, 72:151] % 5 == 0) & (ys[4:61, 72:151] % 4 == 0))   # block with holes: 3 and 4 edges
        holes[70:91, 8:150] = (xs[70:91, 8:150] % 3 == 2) & (ys[70:91, 8:150] % 3 == 1)     # isolated vertices: no edge
        # tile corners (8, 8), (40, 8), (103, 15), (104, 16), (135, 23); borders: left (104, 20), bottom (120, 23), top (91, 8)
        extra = [(x, y, x + 3, y + 2) for x, y in [(8, 8), (40, 8), (103, 15), (104, 16), (135, 23), (104, 20), (120, 23), (91, 8)]]
        assert all(holes[y, x] for x, y, _, _ in extra)
        deg = sum(np.roll(holes, s, a) for s, a in [(1, 0), (-1, 0), (1, 1), (-1, 1)]) * holes
        assert all(((deg == d) & (holes != 0))[8:16, 72:104].any() for d in (3, 4)) and ((deg == 0) & (holes != 0)).any()
        assert all(((deg == d) & (holes != 0))[40:48, 8:40].any() for d in (1, 2))
        # a halo cell that starts from zero and one that does not: active vertices either side of the tile border x = 103 | 104,
        # one of them a handle (its residual, so its p0, is not zero), and a hole next to that border
        assert holes[16, 103] and holes[16, 104] and not holes[16, 105]
        _cache["frames"] = dict(full=_frame_from_labels(np.ones((H, W), np.int32), 1), rows88=_frame_from_labels(rows88, 5),
                                thin=_frame_from_labels(thin, 3), holes=_frame_from_labels(holes, 4, extra))
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


@pytest.mark.parametrize("ns", [6, 7, 8])
@pytest.mark.parametrize("L", [1, 2, 3])
def test_short_loops_on_holes(monkeypatch, L, ns):
    """degrees 0 .. 4, handles on tile corners and borders; the solves need fewer slots than `ns`: slots without a tile"""
    f = _frames()
    ref = _both_flavours(monkeypatch, "holes+thin L%d" % L, W, H, [f["holes"], f["thin"]], (1, 2, L), ns=ns)
    assert np.abs(ref[0][0] - np.stack(np.mgrid[0:H, 0:W][::-1], -1)).max() > 0.0       # (even one iteration moves something)


@pytest.mark.parametrize("ns", [1, 9])
def test_slot_counts_beyond_the_gates(monkeypatch, ns):
    f = _frames()
    _both_flavours(monkeypatch, "holes+thin L3", W, H, [f["holes"], f["thin"]], (1, 2, 3), ns=ns)


@pytest.mark.parametrize("L", [1, 3, 30])
def test_at_most_one_halo_entry_per_thread(monkeypatch, L):
    """one solve alone in its bin: 64 workgroups for 60 tiles, one tile (80 halo cells at most) or none each"""
    f = _frames()
    _both_flavours(monkeypatch, "full L%d" % L, W, H, [f["full"]], (1, 2, L), most=1)


def test_two_halo_entries_per_thread(monkeypatch):
    """16 workgroups, four tiles each (the last ones three): 256 < halo cells <= 320"""
    f = _frames()
    _both_flavours(monkeypatch, "full L3", W, H, [f["full"]], (1, 2, 3), groups=32, most=4)


@pytest.mark.parametrize("L", [2, 3, 30])
def test_three_halo_entries_per_thread(monkeypatch, L):
    """55 tiles for 8 workgroups: seven each (one has six), and a workgroup whose seven tiles lie inside the mask has
    7 x 80 - 16 = 544 halo cells: threads 0 .. 31 own three"""
    f = _frames()
    _both_flavours(monkeypatch, "rows88 L%d" % L, W, H, [f["rows88"]], (1, 2, L), groups=64, most=7)


def test_seven_tiles_in_one_workgroup_and_oracle(monkeypatch):
    """64x64, a 64x24 block and a 32x8 one below it: 7 tiles, one workgroup holds them all (ARAPOPT_RES_GROUPS=512); and the
    CPU oracle"""
    from oracle import oracle as orc
    w = h = 64
    mask = np.full((h, w), 255, np.uint8)
    mask[16:40, :] = 0
    mask[40:48, :32] = 0
    cons = np.asarray([(16, 20, 19, 22), (48, 20, 45, 23), (16, 44, 19, 41), (40, 36, 43, 38)], np.int32)
    frame = dict(mask_red=mask, constraints=cons)
    ref = _both_flavours(monkeypatch, "64x64 seven", w, h, [frame], (1, 2, 50), groups=512, most=7)
    O, A, costs = orc.frame(mask, cons, numIter=1, nIterations=2, lIterations=50, dtype=np.float32, mode=1, trig=1)
    act = mask == 0
    grid = np.stack(np.mgrid[0:h, 0:w][::-1], -1).astype(np.float32)
    err = np.sqrt(((ref[0][0] - O)[act] ** 2).sum() / ((O - grid)[act] ** 2).sum())
    assert err < 1e-4, err                                                             # (the bound of smoke())
