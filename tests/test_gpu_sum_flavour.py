"""The group-sum flavours of the resident kernel (arap_resident.h: RES_SUMS_FLAT carries only the flat sum, RES_SUMS_ANY
all three).  A launch takes the flat flavour exactly when every group dealt to it has <= 64 workgroups; ARAPOPT_RES_SUMS=any
forces the other.  Both perform the same operations in the same order, so every case wants the same BITS from the flat
flavour, from the forced `any` flavour and from the kernel-per-phase path (ArapFlow_SetResident(state, 0)), and
FrameSolver.stats()["resident_sums"] must say which flavour ran.

Shapes: a 64x64 solve (one tile slot); the 7-, 8- and 9-slot instantiations forced on 160x96 frames (60 tiles: a full mask,
and a blob cut by the image border, whose outer halo cells belong to nobody); three slots of which one is empty and one
has a one-vertex-wide component (groups of different sizes in one launch); a launch that mixes a solve wider than one XCD
with two narrow ones (`any`), and the same solver then dealt narrow solves only (`flat`: the captured graph of the step
is replayed across a change of flavour only if the flavour is part of its key).
"""
import numpy as np
import pytest

from arap_flow_amd import opt, synth

pytestmark = pytest.mark.gpu

_cache = {}


def _frame_from_labels(labels, seed):
    return dict(mask_red=np.where(labels != 0, 0, 255).astype(np.uint8), constraints=synth.make_constraints(labels, seed))


def _small_frames():
    """160x96: the full mask (5 x 12 = 60 tiles), a blob cut by the left and the top border, a blob with a one-vertex-wide
    stripe next to it, and a mask that excludes every vertex"""
    if "small" not in _cache:
        W, H = 160, 96
        ys, xs = np.mgrid[0:H, 0:W]
        cut = (((xs - 20) / 70.0) ** 2 + ((ys - 10) / 50.0) ** 2 <= 1.0).astype(np.int32)          # reaches x = 0 and y = 0
        assert cut[0].any() and cut[:, 0].any() and not cut[:, -1].any()
        thin = (((xs - 50) / 30.0) ** 2 + ((ys - 48) / 25.0) ** 2 <= 1.0).astype(np.int32)
        thin[10:71, 100] = 1                                                                       # x = 100: on the handle lattice
        _cache["small"] = dict(full=_frame_from_labels(np.ones((H, W), np.int32), 1), cut=_frame_from_labels(cut, 2),
                               thin=_frame_from_labels(thin, 3),
                               none=dict(mask_red=np.full((H, W), 255, np.uint8), constraints=np.zeros((0, 4), np.int32)))
        assert len(_cache["small"]["thin"]["constraints"]) > 0 and len(_cache["small"]["cut"]["constraints"]) > 0
    return _cache["small"]


def _run(monkeypatch, W, H, batch, deals, sched, way, ns=0):
    """One solver, one solve per entry of `deals` (each a list of frames for slots 0 ..): the results of every solve and
    the flavour its launches reported.  `way`: "flat" (as dealt), "any" (ARAPOPT_RES_SUMS=any) or "two" (two-kernel path).
    The environment is read when the state and its plans are made."""
    if way == "any":
        monkeypatch.setenv("ARAPOPT_RES_SUMS", "any")
    if ns:
        monkeypatch.setenv("ARAPOPT_RES_NS", str(ns))
    st = opt.State()
    try:
        st.set_resident(way != "two")
        fs = opt.FrameSolver(st, W, H, batch=batch)
        out = []
        for frames in deals:
            for b, f in enumerate(frames):
                fs.set_frame(b, f["mask_red"], f["constraints"])
            fs.solve(len(frames), *sched)
            res = []
            for b in range(len(frames)):
                r = fs.results(b, want_rgb=False)
                res.append((r["offset"].copy(), r["angle"].copy(), r["cost"]))
            s = fs.stats()
            assert (s["resident_launches"] > 0) == (way != "two"), s
            out.append((res, s["resident_sums"], s["resident_launches_per_step"]))
        fs.close()
    finally:
        st.close()
        monkeypatch.delenv("ARAPOPT_RES_SUMS", raising=False)
        monkeypatch.delenv("ARAPOPT_RES_NS", raising=False)
    return out


def _reference(key, monkeypatch, *args):
    """the two-kernel solve(s) of a case: computed once, shared by every case that needs it, never modified"""
    if key not in _cache:
        out = _run(monkeypatch, *args, "two")
        for res, sums, per_step in out:
            assert sums == "" and per_step == 0
            for o, a, _ in res:
                o.setflags(write=False)
                a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def _same_bits(got, ref):
    assert len(got) == len(ref)
    for (o, a, c), (ro, ra, rc) in zip(got, ref):
        assert np.array_equal(o, ro) and np.array_equal(a, ra)
        assert c == rc


def test_small_solve_one_slot(monkeypatch):
    W = H = 64
    frame = dict(mask_red=np.zeros((H, W), np.uint8),
                 constraints=np.asarray([(16, 16, 19, 19), (48, 16, 45, 19), (16, 48, 19, 45), (48, 48, 51, 51)], np.int32))
    args = (W, H, 1, [[frame]], (1, 2, 50))
    ref = _reference("64x64", monkeypatch, *args)
    for way in ("flat", "any"):
        (res, sums, per_step), = _run(monkeypatch, *args, way)
        assert sums == way and per_step == 1
        _same_bits(res, ref[0][0])
    assert np.abs(ref[0][0][0][0] - np.stack(np.mgrid[0:H, 0:W][::-1], -1)).max() > 0.5        # (the handles moved something)


@pytest.mark.parametrize("ns", [7, 8, 9])
def test_wide_kernels_on_a_small_frame(monkeypatch, ns):
    f = _small_frames()
    args = (160, 96, 2, [[f["full"], f["cut"]]], (1, 2, 30))
    ref = _reference("160x96 wide", monkeypatch, *args)
    for way in ("flat", "any"):
        (res, sums, per_step), = _run(monkeypatch, *args, way, ns=ns)
        assert sums == way and per_step == 1
        _same_bits(res, ref[0][0])


def test_batch_of_three_with_an_empty_slot(monkeypatch):
    f = _small_frames()
    args = (160, 96, 3, [[f["full"], f["none"], f["thin"]]], (1, 2, 30))
    ref = _reference("160x96 three", monkeypatch, *args)
    for way in ("flat", "any"):
        (res, sums, per_step), = _run(monkeypatch, *args, way)
        assert sums == way and per_step == 1
        _same_bits(res, ref[0][0])
    assert ref[0][0][1][2] == 0.0                                  # nothing to solve in the empty slot


def test_mixed_launch_then_flavour_change_on_replay(monkeypatch):
    """a mask == 0 solve at 854x480 (1620 tiles: four XCDs, two-level sums) next to two DAVIS-shaped ones: one launch of the
    `any` flavour; then the same solver with a DAVIS-shaped frame in slot 0: one launch again, now `flat`"""
    W, H = 854, 480
    wide = synth.make_frame(W, H, seed=60, full_mask=True)
    narrow = [synth.make_frame(W, H, seed=61 + s) for s in range(3)]
    args = (W, H, 3, [[wide, narrow[0], narrow[1]], [narrow[2], narrow[0], narrow[1]]], (1, 1, 10))
    ref = _reference("854x480 mixed", monkeypatch, *args)
    got = _run(monkeypatch, *args, "flat")
    assert [g[1] for g in got] == ["any", "flat"] and [g[2] for g in got] == [1, 1]
    for g, r in zip(got, ref):
        _same_bits(g[0], r[0])
    forced = _run(monkeypatch, *args, "any")
    assert [g[1] for g in forced] == ["any", "any"]
    for g, r in zip(forced, ref):
        _same_bits(g[0], r[0])
