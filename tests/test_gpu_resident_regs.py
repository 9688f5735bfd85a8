"""The resident kernel's register forms (arap_resident.h): kept weights as one VGPR each (and all five of them at 8 and 9
slots), the own search direction and z in registers up to 7 slots in the flat flavour, and the flat flavour's one-trip sweep
of a group's granules.  None of them changes an operation, an operand or an order of additions, so every case wants the same
BITS -- Offset, Angle and cost -- from the resident path as dealt (flat), with ARAPOPT_RES_SUMS=any and from the
kernel-per-phase path (ArapFlow_SetResident(state, 0)); one case is also held against the CPU oracle.

Shapes (160x96 = 60 tiles of 32x8, and 64x64): the slot counts either side of every gate (1, 6, 7, 8, 9); PCG loops of 1, 2
and 3 iterations (1: the loop leaves before any update, the epilogue's delta += alpha p takes the prologue's p; 2: one update,
beta from the first rho); a mask whose vertices have 0, 1, 2, 3 and 4 valid edges inside one tile, handles on tile corners and
borders, unused slots; groups of 64, of odd widths below 64, of 8 and of 1 workgroups for the one-trip sweep."""
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
    """160x96: the full mask, a blob cut by the left and the top border, a blob with a one-vertex-wide stripe (the frames
    of test_gpu_sum_flavour.py), and `holes`: one-vertex-wide vertical and horizontal stripes, a block with single-vertex
    holes, isolated vertices; its bands start at x = 8, so its tiles are [8 + 32 k, 8 + 32 k + 31] x [8 m, 8 m + 7], and it
    has handles on corners and borders of those tiles next to the lattice ones"""
    if "frames" not in _cache:
        ys, xs = np.mgrid[0:H, 0:W]
        cut = (((xs - 20) / 70.0) ** 2 + ((ys - 10) / 50.0) ** 2 <= 1.0).astype(np.int32)
        thin = (((xs - 50) / 30.0) ** 2 + ((ys - 48) / 25.0) ** 2 <= 1.0).astype(np.int32)
        thin[10:71, 100] = 1
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
        _cache["frames"] = dict(full=_frame_from_labels(np.ones((H, W), np.int32), 1), cut=_frame_from_labels(cut, 2),
                                thin=_frame_from_labels(thin, 3), holes=_frame_from_labels(holes, 4, extra))
    return _cache["frames"]


def _widths(frames, w, h, env_groups):
    """group sizes the host deals these solves (pure host functions of the library; the forced deal is read per call)"""
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
    """results of one solve of `frames` (slots 0 ..) and the flavour its launches reported.  `way`: "flat" (as dealt), "any"
    (ARAPOPT_RES_SUMS=any) or "two" (kernel-per-phase path).  The environment is read when the state and its plans are made."""
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
        widths = _widths(frames, w, h, groups)[0] if way != "two" else None
        fs.close()
    finally:
        st.close()
        for k in ("ARAPOPT_RES_SUMS", "ARAPOPT_RES_NS", "ARAPOPT_RES_GROUPS"):
            monkeypatch.delenv(k, raising=False)
    return res, s["resident_sums"], s["resident_launches_per_step"], widths


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


def _both_flavours(monkeypatch, key, w, h, frames, sched, ns=0, groups=0, widths=None):
    ref = _reference(key, monkeypatch, w, h, frames, sched)
    for way in ("flat", "any"):
        res, sums, per_step, wd = _run(monkeypatch, w, h, frames, sched, way, ns=ns, groups=groups)
        assert sums == way and per_step == 1
        if widths is not None:
            assert widths(wd), wd
        _same_bits(res, ref)
    return ref


@pytest.mark.parametrize("ns", [1, 6, 7, 8, 9])
def test_slot_counts(monkeypatch, ns):
    f = _frames()
    _both_flavours(monkeypatch, "full+cut 30", W, H, [f["full"], f["cut"]], (1, 2, 30), ns=ns)


@pytest.mark.parametrize("L", [1, 2, 3])
def test_short_pcg_loops(monkeypatch, L):
    f = _frames()
    ref = _both_flavours(monkeypatch, "full+cut L%d" % L, W, H, [f["full"], f["cut"]], (1, 2, L), ns=7)
    assert np.abs(ref[0][0] - np.stack(np.mgrid[0:H, 0:W][::-1], -1)).max() > 0.0       # (even one iteration moves something)


@pytest.mark.parametrize("ns", [6, 7, 8, 9])
def test_zero_weights_and_unused_slots(monkeypatch, ns):
    """every degree 0 .. 4 inside one tile, the fit weight on and off within one wave, and (the solves need fewer slots
    than `ns`) slots without a tile"""
    f = _frames()
    ref = _both_flavours(monkeypatch, "holes+thin", W, H, [f["holes"], f["thin"]], (1, 2, 30), ns=ns)
    assert np.isfinite(ref[0][0]).all() and np.isfinite(ref[0][1]).all() and np.isfinite(ref[0][2])


def test_one_solve_alone_in_its_bin(monkeypatch):
    f = _frames()
    _both_flavours(monkeypatch, "full alone", W, H, [f["full"]], (1, 2, 30), widths=lambda wd: wd[0] == 64)


def test_solves_of_different_sizes_share_bins(monkeypatch):
    """19 solves in 8 bins: groups of 14, 16, 19, 34 and 44 workgroups (three solves to a bin have to share it)"""
    f = _frames()
    frames = [f["full"]] + [f["cut"], f["thin"], f["holes"]] * 6
    _both_flavours(monkeypatch, "nineteen", W, H, frames, (1, 2, 30),
                   widths=lambda wd: max(wd) < 64 and len(set(wd)) >= 3 and any(x % 2 for x in wd))


def test_groups_of_eight_workgroups(monkeypatch):
    f = _frames()
    _both_flavours(monkeypatch, "full alone", W, H, [f["full"]], (1, 2, 30), groups=64, widths=lambda wd: wd == [8])


def test_group_of_one_workgroup_and_oracle(monkeypatch):
    """a 64x32 block of a 64x64 frame: 8 tiles, one workgroup holds them all (ARAPOPT_RES_GROUPS=512); and the CPU oracle"""
    from oracle import oracle as orc
    w = h = 64
    mask = np.full((h, w), 255, np.uint8)
    mask[16:48, :] = 0
    cons = np.asarray([(16, 20, 19, 22), (48, 20, 45, 23), (16, 44, 19, 41), (48, 44, 51, 46)], np.int32)
    frame = dict(mask_red=mask, constraints=cons)
    ref = _both_flavours(monkeypatch, "64x64 block", w, h, [frame], (1, 2, 50), groups=512, widths=lambda wd: wd == [1])
    O, A, costs = orc.frame(mask, cons, numIter=1, nIterations=2, lIterations=50, dtype=np.float32, mode=1, trig=1)
    act = mask == 0
    grid = np.stack(np.mgrid[0:h, 0:w][::-1], -1).astype(np.float32)
    err = np.sqrt(((ref[0][0] - O)[act] ** 2).sum() / ((O - grid)[act] ** 2).sum())
    assert err < 1e-4, err                                                             # (the bound of smoke())
