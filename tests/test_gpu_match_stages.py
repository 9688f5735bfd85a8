"""The matcher stage by stage (tests/match_ref.py): every kernel of arapmatch.hip after the descriptors is checked on
the matcher's OWN output of the stage before it, so that nothing is left to near-tie slack -- level 0 against a float64
sum within the float32 summation bound, the levels above within the ulp bound of the power, the match rows bit for
bit -- at the smallest frames at which each branch of the kernels is taken.

The CPU half proves that the checks have teeth: the oracle plays the matcher (every check passes), then plays it with
one fault at a time (the check of that stage fails, at the shape that was chosen for it)."""
import numpy as np
import pytest

import match_ref as mr
from oracle import dm_oracle as dm
from test_match import _translated_pair

# W, H, ngh_rad                       r    why
CASES = [
    (270, 18, 24),                  # 12   gw = 33: a second k_corr0 column holding one patch; gh = 2, w % 4 = 3, h % 4 = 1; partial placement tile (NP = 152)
    (280, 200, 32),                 # 16   gw = 35, gh = 25, five levels (S = 33, 17, 9, 5, 3): every k_bt_step depth
    (96, 66, 18),                   # 9    odd r: o = 1 from level 0 to level 1
    (32, 300, 20),                  # 10   gh = 37, gw = 4; odd centre higher up (c = 5 at level 1): o = 1 from level 1 to level 2
    (64, 32, 2),                    # 1    S = 3, S2 = 1: the pyramid stops at level 1; one cell per map in k_argmax; z-split per = 2 of 3 rows
    (64, 32, 0),                    # 1    clamped from 0: the same result as the case above
    (272, 32, 400),                 # 96   clamped from 200: largest LDS ring, S = 193, most of every window in the padding; gw = 34
]
KINDS = ["texture", "random", "flat"]
GEOMETRY = {                        # written out by hand from the rules in dm_oracle's docstring: (nh, nw, S, c) per level
    (270, 18, 24): [(2, 33, 25, 12), (1, 32, 13, 6)],
    (280, 200, 32): [(25, 35, 33, 16), (24, 34, 17, 8), (11, 16, 9, 4), (5, 7, 5, 2), (2, 3, 3, 1)],
    (96, 66, 18): [(8, 12, 19, 9), (7, 11, 9, 4), (3, 5, 5, 2), (1, 2, 3, 1)],
    (32, 300, 20): [(37, 4, 21, 10), (36, 3, 11, 5), (17, 1, 5, 2)],
    (64, 32, 2): [(4, 8, 3, 1), (3, 7, 1, 0)],
    (64, 32, 0): [(4, 8, 3, 1), (3, 7, 1, 0)],
    (272, 32, 400): [(4, 34, 193, 96), (3, 33, 97, 48), (1, 16, 49, 24)],
}

# Largest float32 distance allowed between k_level_up's powf and the correctly rounded float64 power.  The ROCm
# installation documents no accuracy figure for powf, so the largest distance from the float64 reference seen in one
# run of all 21 (case, input) pairs below on an MI355X was recorded -- 1 ulp, at every level of every textured and
# random pair (numpy's float32 power on the CPU: also 1) -- and one ulp is added.  Level 0 in the same run: at most
# 15.8 u relative, against the bound of 145 u.
POW_ULP_SEEN = 1
POW_ULP = POW_ULP_SEEN + 1


def pair(kind, W, H):
    if kind == "texture":
        return _translated_pair(W, H, 2, -2, seed=W + H)
    if kind == "random":
        rng = np.random.default_rng(1000 * W + H)
        return rng.integers(0, 256, (H, W, 3), np.uint8), rng.integers(0, 256, (H, W, 3), np.uint8)
    flat = np.full((H, W, 3), 77, np.uint8)
    return flat, flat.copy()


def _ids(v):
    return "%dx%d-rad%d" % v if isinstance(v, tuple) else None


# ----------------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_hip_matcher_stage_by_stage(case, kind):
    from arap_flow_amd import match
    W, H, rad = case
    a, b = pair(kind, W, H)
    mt = match.Matcher(W, H, rad)
    try:
        rows = mt.run(a, b)
        geo = mt.levels()
        failures, stats = mr.chain(mt, rows, rad, POW_ULP)
    finally:
        mt.close()
    print("%dx%d rad %d %s: %r" % (W, H, rad, kind, stats))
    assert geo == GEOMETRY[case]
    assert not failures, "\n".join(failures)
    assert len(rows) > 0 and np.array_equal(rows[:, 5], np.arange(len(rows)))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_radius_clamped_from_zero_is_radius_one(kind):
    """ngh_rad = 0 and ngh_rad = 2 both search r = 1: every map and every row byte for byte the same"""
    from arap_flow_amd import match
    a, b = pair(kind, 64, 32)
    out = []
    for rad in (2, 0):
        mt = match.Matcher(64, 32, rad)
        try:
            rows = mt.run(a, b)
            out.append((mt.levels(), [mt.level_maps(k).tobytes() for k in range(len(mt.levels()))], rows.tobytes()))
        finally:
            mt.close()
    assert out[0][0][0][3] == 1 and out[0] == out[1]


@pytest.mark.gpu
def test_matcher_reuse_resets_its_buffers():
    """A, B, A on one matcher: the third result is the first, B's is that of a fresh matcher (best, bins and the entry
    buffers carry nothing over).  B is flat: every patch matches, so nothing A wrote may survive; A after B likewise."""
    from arap_flow_amd import match
    W, H, rad = 96, 66, 18
    A, B = pair("texture", W, H), pair("flat", W, H)
    mt = match.Matcher(W, H, rad)
    fresh = match.Matcher(W, H, rad)
    try:
        r1, rb, r3 = mt.run(*A), mt.run(*B), mt.run(*A)
        fb = fresh.run(*B)
    finally:
        mt.close()
        fresh.close()
    assert len(r1) > 0 and r1.tobytes() == r3.tobytes()
    assert len(fb) > 0 and rb.tobytes() == fb.tobytes() and rb.tobytes() != r1.tobytes()


@pytest.mark.gpu
def test_run_with_a_small_cap_returns_the_full_count_and_writes_cap_rows():
    from arap_flow_amd import match
    W, H, rad = 96, 66, 18
    a, b = pair("texture", W, H)
    mt = match.Matcher(W, H, rad)
    try:
        full = mt.run(a, b)
        cap = len(full) // 2
        assert cap >= 8
        guard = np.uint32(0xDEADBEEF)
        out = np.full((len(full) + 4, 6), guard, np.uint32)
        n = mt.lib.ArapMatch_Run(mt.h, a.ctypes.data, b.ctypes.data, out.ctypes.data, cap)
        zero = mt.lib.ArapMatch_Run(mt.h, a.ctypes.data, b.ctypes.data, out[cap:].ctypes.data, 0)
    finally:
        mt.close()
    assert n == len(full) and zero == len(full)
    assert np.array_equal(out[:cap], full[:cap].view(np.uint32))
    assert (out[cap:] == guard).all()


@pytest.mark.gpu
def test_frames_smaller_than_16_are_refused():
    from arap_flow_amd import match
    lib = match.load()
    assert lib.ArapMatch_Create(15, 64, 100) is None and lib.ArapMatch_Create(64, 15, 100) is None
    h = lib.ArapMatch_Create(16, 16, 100)
    assert h is not None
    lib.ArapMatch_Free(h)


# ----------------------------------------------------------------------------------------------------------------------
# CPU: the oracle plays the matcher
# ----------------------------------------------------------------------------------------------------------------------
_played = {}


def played(case, kind):
    """one clean oracle run per (case, kind), shared and never modified: (matcher, rows)"""
    if (case, kind) not in _played:
        om = mr.OracleMatcher(*case)
        rows = om.run(*pair(kind, *case[:2]))
        for l in om.lv:
            l["maps"].setflags(write=False)
        rows.setflags(write=False)
        _played[(case, kind)] = (om, rows)
    return _played[(case, kind)]


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_geometry_of_every_case_is_the_one_it_was_chosen_for(case):
    W, H, rad = case
    assert mr.pyramid_geometry(H // 2, W // 2, mr.clamped_r(rad)) == GEOMETRY[case]


# r = 96 costs the float32 oracle 3 s per pair: one kind of input there (the GPU test runs all three)
@pytest.mark.parametrize("case,kind", [(c, k) for c in CASES for k in KINDS if c[2] != 400 or k == "random"], ids=lambda v: _ids(v) or v)
def test_positive_control_the_oracle_passes_every_check(case, kind):
    om, rows = played(case, kind)
    failures, stats = mr.chain(om, rows, case[2], POW_ULP)
    assert not failures, "\n".join(failures)
    assert om.levels() == GEOMETRY[case] and stats["matches"] == len(rows) > 0


def test_helpers_compose_to_the_oracle():
    """merge is the second half of dm.matches; pyramid_geometry is dm.pyramid's loop; flat frames give the descriptor
    (0, ..., 0, 1) and therefore nothing but ties"""
    case = (96, 66, 18)
    for kind in KINDS:
        om, rows = played(case, kind)
        assert np.array_equal(rows, dm.matches(*pair(kind, *case[:2]), ngh_rad=case[2]))
        assert om.levels() == mr.pyramid_geometry(33, 48, 9)
    om, rows = played(case, "flat")
    assert np.array_equal(om.descriptors(0), np.broadcast_to(np.eye(9, dtype=np.float32)[8], (33, 48, 9)))
    m0 = om.level_maps(0)
    assert set(np.unique(m0)) == {np.float32(k / 16.0) for k in (0, 1, 2, 3, 4, 6, 8, 9, 12, 16)}     # (rows inside) * (columns inside) / 16
    assert 0 < len(rows) < 8 * 12 and len(np.unique(rows[:, 4])) == 1                                 # contested bins, one score


# ---- negative controls: one fault each -------------------------------------------------------------------------------
def _pyramid_from(m0, r, level_up=dm.level_up):
    """dm.pyramid's loop on given level-0 maps"""
    levels = [dict(maps=m0, c=r, kids=None, o=None)]
    while True:
        up = level_up(levels[-1]["maps"], len(levels) - 1, levels[-1]["c"])
        if up is None or up[0].shape[-1] < 1:
            break
        levels.append(dict(maps=up[0], c=up[3], kids=up[1], o=up[2]))
        if up[0].shape[-1] == 1:
            break
    return levels


def _level0_replicated(d1, d2, r):
    """FAULT: dm.level0 with frame 2 continued by its edge pixels instead of zeros"""
    h, w = d1.shape[:2]
    gh, gw = h // 4, w // 4
    pad = np.pad(d2, ((r, r), (r, r), (0, 0)), mode="edge")
    out = np.zeros((gh, gw, 2 * r + 1, 2 * r + 1), np.float32)
    a = d1[:gh * 4, :gw * 4]
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            dots = (a * pad[r + dy:r + dy + gh * 4, r + dx:r + dx + gw * 4]).sum(-1, dtype=np.float32)
            out[:, :, dy + r, dx + r] = dots.reshape(gh, 4, gw, 4).sum((1, 3), dtype=np.float32) * np.float32(1.0 / 16.0)
    return out


def _level_up_o0(m, level, c):
    """FAULT: dm.level_up pooling around cell 2k instead of 2k + o (the geometry of the level above unchanged)"""
    up = dm.level_up(m, level, c)
    if up is None:
        return None
    maps, kids, o, c2 = up
    pooled = dm.maxpool(m, 0)[..., :maps.shape[-1], :maps.shape[-1]]
    acc = np.zeros(maps.shape, np.float32)
    for q in range(4):
        acc = acc + pooled[kids[q][..., 0], kids[q][..., 1]]
    return np.power(np.maximum(acc * np.float32(0.25), np.float32(0)), dm.LAMBDA, dtype=np.float32), kids, o, c2


def _level_up_sloppy_power(m, level, c):
    """FAULT: dm.level_up with a power that is POW_ULP + 1 float32 steps too large wherever it is not 0"""
    up = dm.level_up(m, level, c)
    if up is None:
        return None
    bits = up[0].view(np.int32) + np.where(up[0] > 0, POW_ULP + 1, 0).astype(np.int32)
    return (bits.view(np.float32),) + up[1:]


def _backtrack(levels, entry_last=False, step_last=False):
    """dm.backtrack, sequentially, with two FAULTS to switch on: the last maximum instead of the first as entry point,
    and in the 3x3 step"""
    gh, gw, S0, _ = levels[0]["maps"].shape
    cand = {}
    for top in range(1, len(levels)):
        m = levels[top]["maps"]
        nh, nw, S, _ = m.shape
        for J in range(nh):
            for I in range(nw):
                flat = m[J, I].ravel()
                k = S * S - 1 - int(flat[::-1].argmax()) if entry_last else int(flat.argmax())
                cur = [(J, I, k // S, k % S, flat[k])]
                for lv in range(top, 0, -1):
                    kids, o, below = levels[lv]["kids"], levels[lv]["o"], levels[lv - 1]["maps"]
                    Sb, nxt = below.shape[-1], []
                    for (j, i, ky, kx, s) in cur:
                        for q in range(4):
                            cj, ci = kids[q][j, i]
                            bv, by, bx = np.float32(-np.inf), 0, 0
                            for u in (-1, 0, 1):
                                for v in (-1, 0, 1):
                                    y, x = 2 * ky + o + u, 2 * kx + o + v
                                    if 0 <= y < Sb and 0 <= x < Sb:
                                        val = below[cj, ci, y, x]
                                        if val > bv or (step_last and val == bv):
                                            bv, by, bx = val, y, x
                            nxt.append((cj, ci, by, bx, np.float32(s + bv)))
                    cur = nxt
                for (j, i, ky, kx, s) in cur:
                    key = (s, -(ky * S0 + kx))                           # ties: the smaller cell index
                    if s > 0 and ((j, i) not in cand or key > cand[(j, i)]):
                        cand[(j, i)] = key
    best = np.zeros((gh, gw), np.float32)
    cell = np.zeros((gh, gw, 2), np.int32)
    for (j, i), (s, code) in cand.items():
        best[j, i], cell[j, i] = s, divmod(-code, S0)
    return best, cell


class Faulty(mr.OracleMatcher):
    def __init__(self, case, fault):
        super().__init__(*case)
        self.fault = fault

    def pyramid(self, d1, d2):
        f, r = self.fault, self.r
        if f == "shift32":                                              # patches i >= 32 one cell off in dx
            m0 = dm.level0(d1, d2, r)
            m0[:, 32:] = np.roll(m0[:, 32:], 1, axis=-1)
            return _pyramid_from(m0, r)
        if f == "replicate":
            return _pyramid_from(_level0_replicated(d1, d2, r), r)
        if f == "sloppy_power":
            return _pyramid_from(dm.level0(d1, d2, r), r, _level_up_sloppy_power)
        if f == "pool_o0":
            return _pyramid_from(dm.level0(d1, d2, r), r, _level_up_o0)
        return dm.pyramid(d1, d2, r)

    def backtrack(self, levels):
        f = self.fault
        if f == "step_o0":                                              # the 3x3 window around 2k instead of 2k + o
            return dm.backtrack([dict(l, o=0 if l["o"] is not None else None) for l in levels])
        if f in ("entry_last", "step_last"):
            return _backtrack(levels, entry_last=f == "entry_last", step_last=f == "step_last")
        return dm.backtrack(levels)

    def merge(self, best, cell, c0, h2, w2):
        if self.fault != "bin_larger":
            return mr.merge(best, cell, c0, h2, w2)
        # FAULT: mr.merge with the patches met in descending order, the first one met keeping a tied bin: the LARGER
        # patch index wins; rows in the order of the atomic patches as always
        gh, gw = best.shape
        win = {}
        for p in range(gh * gw - 1, -1, -1):
            j, i = divmod(p, gw)
            x2, y2 = 4 * i + 2 + int(cell[j, i, 1]) - c0, 4 * j + 2 + int(cell[j, i, 0]) - c0
            if best[j, i] <= 0 or not (0 <= x2 < w2 and 0 <= y2 < h2):
                continue
            key = (y2 // 4, x2 // 4)
            if key not in win or best[j, i] > win[key][0]:
                win[key] = (best[j, i], p, x2, y2)
        out = [(2 * (4 * (p % gw) + 2), 2 * (4 * (p // gw) + 2), 2 * x2, 2 * y2, s, n)
               for n, (s, p, x2, y2) in enumerate(sorted(win.values(), key=lambda t: t[1]))]
        return np.asarray(out, np.float32).reshape(-1, 6)


def _fails(case, kind, fault):
    """stage names whose check rejects the oracle playing with `fault`, and that run's rows"""
    fm = Faulty(case, fault)
    rows = fm.run(*pair(kind, *case[:2]))
    failures, _ = mr.chain(fm, rows, case[2], POW_ULP)
    return [f.split(":")[0] for f in failures], fm, rows


def test_sequential_backtrack_without_faults_is_the_oracles():
    for kind in KINDS:
        om, _ = played((96, 66, 18), kind)
        b0, c0 = dm.backtrack(om.lv)
        b1, c1 = _backtrack(om.lv)
        assert np.array_equal(b0, b1) and np.array_equal(c0[b0 > 0], c1[b0 > 0])


def test_negative_control_second_corr0_column_shifted():
    """only level 0 is wrong (everything above is built on the shifted maps), and only at gw > 32: the same fault at
    gw = 12 changes nothing, which is why 270 x 18 is in the list"""
    case = (270, 18, 24)
    for kind in ("texture", "random"):
        stages, fm, _ = _fails(case, kind, "shift32")
        assert stages == ["level0"]
        assert not np.array_equal(fm.level_maps(0)[:, 32], played(case, kind)[0].level_maps(0)[:, 32])
    assert _fails((96, 66, 18), "texture", "shift32")[0] == []


def test_negative_control_edge_replication_instead_of_zero_padding():
    for case in ((270, 18, 24), (64, 32, 2)):
        for kind in KINDS:
            stages, fm, _ = _fails(case, kind, "replicate")
            assert stages == ["level0"], (case, kind, stages)
            assert not np.array_equal(fm.level_maps(0), played(case, kind)[0].level_maps(0))


def test_negative_control_power_a_few_ulp_off():
    """every level above level 0 is rejected, by the ulp bound and, on flat frames (pre-power value 1), by exactness;
    the rows, backtracked on those very maps, are not"""
    for kind in KINDS:
        stages, _, _ = _fails((96, 66, 18), kind, "sloppy_power")
        assert stages == ["level1", "level2", "level3"], (kind, stages)


def test_negative_control_subsampling_offset_forced_to_zero():
    """odd r: o = 1 between level 0 and level 1 (96 x 66); odd centre at level 1: o = 1 between level 1 and level 2
    (32 x 300).  With o = 0 in the pooling the level above is wrong; with o = 0 in the backtracking step alone the rows
    are.  At even r and even centres all the way up (280 x 200) neither fault can show."""
    for case, level in (((96, 66, 18), "level1"), ((32, 300, 20), "level2")):
        assert [l["o"] for l in played(case, "texture")[0].lv[1:]][int(level[-1]) - 1] == 1
        for kind in ("texture", "random"):
            stages, fm, _ = _fails(case, kind, "pool_o0")
            assert stages == [level], (case, kind, stages)
            stages, _, rows = _fails(case, kind, "step_o0")
            assert stages == ["matches"], (case, kind, stages)
            assert rows.tobytes() != played(case, kind)[1].tobytes()
    assert [l["o"] for l in played((280, 200, 32), "texture")[0].lv[1:]] == [0, 0, 0, 0]


def test_negative_control_last_maximum_instead_of_first():
    """flat frames: every cell inside the frame ties, so the rows depend on nothing but the tie rules.  (At r = 1 the
    maps above level 0 have one cell: only the 3x3 step has a choice there.)"""
    for case, fault in (((96, 66, 18), "entry_last"), ((96, 66, 18), "step_last"), ((64, 32, 2), "step_last")):
        stages, _, rows = _fails(case, "flat", fault)
        assert stages == ["matches"], (case, fault, stages)
        assert rows.tobytes() != played(case, "flat")[1].tobytes()


def test_negative_control_larger_patch_wins_a_bin_tie():
    """flat frames: neighbouring patches along the frame borders reach for the same first cells of frame 2 with equal
    scores, so bins are tied and the rows say which patch a tie went to"""
    for case in ((96, 66, 18), (270, 18, 24)):
        stages, _, rows = _fails(case, "flat", "bin_larger")
        assert stages == ["matches"], (case, stages)
        assert rows.tobytes() != played(case, "flat")[1].tobytes()
