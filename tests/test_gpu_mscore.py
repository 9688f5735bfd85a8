"""GPU: ArapFlow_LabelScore / ArapFlow_MapScore (opt.label_score, opt.map_score; DESIGN.md "Map scoring") byte for byte
against the numpy twin tests/mscore_ref.py: at the shapes the kernels branch on (less than a wave, maps misaligned for the
16-byte groups, one pixel past a wave row, more rows than the column pass has runs, a staged window wider than the frame at
radius 254), every radius, label count and threshold count edge, maps of one and of two values (every count of a block in
one bin), many maps, more maps than grid rows; the properties that need no twin; launch counts, garbage-filled outputs,
determinism, misaligned buffers and every refusal against sentinel-filled outputs."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mscore_ref
from arap_flow_amd import opt

pytestmark = pytest.mark.gpu
U8 = np.uint8
SHAPES = [(5, 3, 1), (71, 9, 3), (64, 4, 1), (65, 4, 1), (7, 5, 1), (130, 70, 1)]


@functools.lru_cache(maxsize=None)
def case(W, H, n, seed=0):
    """label maps in blocks of 0..4 and 9 with an estimate that is the ground truth moved, with noise and labels of its
    own; a binary map with a score on every value the thresholds test; a sparse skip plane; read-only"""
    rng = np.random.default_rng([W, H, n, seed])
    cells = rng.choice(np.array([0, 0, 1, 2, 3, 4, 9], U8), size=(n, (H + 4) // 5, (W + 6) // 7))
    gt = np.kron(cells, np.ones((5, 7), U8))[:, :H, :W]
    est = np.roll(gt, (1, 2), axis=(1, 2))
    noise = rng.random((n, H, W)) < 0.05
    est = np.where(noise, rng.choice(np.array([0, 1, 2, 3, 200, 255], U8), size=(n, H, W)), est).astype(U8)
    occ = np.where(gt >= 2, rng.choice(np.array([1, 255], U8), size=(n, H, W)), 0).astype(U8)
    score = np.where(np.roll(occ, 1, axis=2) != 0, rng.choice(np.array([63, 64, 128, 254, 255], U8), size=(n, H, W)),
                     rng.choice(np.array([0, 0, 0, 1, 63, 255], U8), size=(n, H, W))).astype(U8)
    skip = rng.choice(np.array([0] * 9 + [2, 255], U8), size=(n, H, W))
    out = dict(gt=np.ascontiguousarray(gt), est=est, occ=occ, score=score, skip=skip)
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def want_label(W, H, n, L, radius, skip):
    c = case(W, H, n)
    return mscore_ref.label_ref(c["gt"], c["est"], L, radius, c["skip"] if skip else None)["table"]


@functools.lru_cache(maxsize=None)
def want_map(W, H, n, thr, radius, skip):
    c = case(W, H, n)
    return mscore_ref.map_ref(c["occ"], c["score"], c["skip"] if skip else None, thr, radius)


def same(got, ref):
    assert got.dtype == np.uint64 and got.shape == ref.shape
    assert np.array_equal(got, ref), (got != ref).nonzero()


def label(st, W, H, n, L, radius, skip):
    c = case(W, H, n)
    return opt.label_score(st, c["gt"], c["est"], L, radius, skip=c["skip"] if skip else None)["table"]


def maps(st, W, H, n, thr, radius, skip):
    c = case(W, H, n)
    return opt.map_score(st, c["occ"], c["score"], skip=c["skip"] if skip else None, thr=thr, radius=radius)


# ---- against the twin ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skip", [False, True], ids=["noskip", "skip"])
@pytest.mark.parametrize("W,H,n", SHAPES)
def test_tables_equal_the_twin(gpu_state, W, H, n, skip):
    """5x3: less than a wave; 71x9x3: W * H is odd, maps 1 and 2 start off the 16-byte groups; 64x4, 65x4: a wave row and
    one pixel more; 7x5; 130x70: more rows than the column pass has runs, three blocks across"""
    same(label(gpu_state, W, H, n, 3, 8, skip), want_label(W, H, n, 3, 8, skip))
    r = maps(gpu_state, W, H, n, (64, 255), 8, skip)
    w = want_map(W, H, n, (64, 255), 8, skip)
    same(r["hist"], w["hist"])
    same(r["match"], w["match"])
    t = want_label(W, H, n, 3, 8, skip)
    assert (t[:, 0, 0] + t[:, 0, 1] == W * H).all() and (w["hist"].sum(axis=(1, 2)) + t[:, 0, 1] == W * H).all()
    if W * H > 500:
        s = t.sum(axis=0)
        assert (s[0, :5] > 0)[[0, 2, 3, 4]].all() and (s[1:, :7] > 0).all()
        assert (w["match"].sum(axis=0) > 0).all() and bool(s[0, 1]) == skip


@pytest.mark.parametrize("skip", [False, True], ids=["noskip", "skip"])
def test_radius_254_on_a_frame_narrower_than_the_window(gpu_state, skip):
    """300x6: the staged window of 64 + 508 columns spans all five blocks of a row and passes both frame edges"""
    same(label(gpu_state, 300, 6, 1, 3, 254, skip), want_label(300, 6, 1, 3, 254, skip))
    r, w = maps(gpu_state, 300, 6, 1, (128,), 254, skip), want_map(300, 6, 1, (128,), 254, skip)
    same(r["hist"], w["hist"])
    same(r["match"], w["match"])


@pytest.mark.parametrize("radius", [0, 1, 8, 254])
def test_every_radius(gpu_state, radius):
    same(label(gpu_state, 71, 9, 3, 3, radius, True), want_label(71, 9, 3, 3, radius, True))
    same(maps(gpu_state, 71, 9, 3, (1, 128), radius, True)["match"], want_map(71, 9, 3, (1, 128), radius, True)["match"])
    if radius == 0:                       # a hit is the same pixel
        c = case(71, 9, 3)
        k = c["skip"] == 0
        A, B = mscore_ref.bmap(c["gt"] == 2) & k, mscore_ref.bmap(c["est"] == 2) & k
        assert (want_label(71, 9, 3, 3, 0, True)[:, 2, 5] == (A & B).sum(axis=(1, 2))).all()


@pytest.mark.parametrize("L", [1, 3, 255])
def test_label_counts_with_labels_above_L(gpu_state, L):
    """the case has the labels 4, 9, 200 and 255: above L = 1 and 3, rows of their own at 255"""
    same(label(gpu_state, 23, 11, 2, L, 2, True), want_label(23, 11, 2, L, 2, True))
    t = want_label(23, 11, 2, L, 2, True)
    assert (t[:, 0, 3].sum() > 0 and t[:, 0, 4].sum() > 0) == (L < 255)
    if L == 255:
        assert t[:, 255, 1].sum() > 0 and t[:, 200, 4].sum() > 0 and t[:, 9, 0].sum() > 0


@pytest.mark.parametrize("thr", [(), (255,), (1, 2, 63, 64, 65, 128, 254, 255)], ids=["m0", "m1", "m8"])
def test_threshold_counts(gpu_state, thr):
    r, w = maps(gpu_state, 71, 9, 3, thr, 1, True), want_map(71, 9, 3, thr, 1, True)
    same(r["hist"], w["hist"])
    same(r["match"], w["match"])
    assert r["match"].shape == (3, len(thr), 4)
    if len(thr) == 8:
        b = w["match"][:, :, 1].sum(axis=0)
        assert b[0] > b[1] == b[2] > b[3] > b[4] == b[5] > b[6] > b[7] > 0        # est >= thr at v - 1, v, v + 1 for v = 64


# ---- contention and overflow ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("values", [1, 2])
def test_854x480_of_one_and_of_two_values(gpu_state, values):
    """409 920 counts in one bin, or in two: every lane of every wave adds to the same word"""
    W, H = 854, 480
    gt = np.full((H, W), 2, U8)
    est = np.full((H, W), 2, U8)
    if values == 2:
        gt[:, 300:] = 0
        est[:, 310:] = 0
    same(opt.label_score(gpu_state, gt, est, 2, 8)["table"], mscore_ref.label_ref(gt, est, 2, 8)["table"])
    occ = (gt != 0).astype(U8) * 255
    sc = (est != 0).astype(U8) * 255
    r, w = opt.map_score(gpu_state, occ, sc, thr=(128,), radius=8), mscore_ref.map_ref(occ, sc)
    same(r["hist"], w["hist"])
    assert w["hist"][0, 1, 255] == (W * H if values == 1 else 300 * H)
    # (sets of whole regions are beyond the twin's explicit minimum: 300 columns against 310, the last 2 further than 8)
    assert r["match"][0, 0].tolist() == ([W * H, W * H, W * H, W * H] if values == 1 else [300 * H, 310 * H, 300 * H, 308 * H])


def count_fields(gt, est, L):
    """row 0 and the fields 0..2 of a label table without a skip plane, all maps at once"""
    n = len(gt)
    t = np.zeros((n, L + 1, 8), np.uint64)
    t[:, 0, 0] = gt[0].size
    t[:, 0, 2] = (gt == est).sum(axis=(1, 2))
    t[:, 0, 3], t[:, 0, 4] = (gt > L).sum(axis=(1, 2)), (est > L).sum(axis=(1, 2))
    for k in range(1, L + 1):
        t[:, k, 0], t[:, k, 1] = (gt == k).sum(axis=(1, 2)), (est == k).sum(axis=(1, 2))
        t[:, k, 2] = ((gt == k) & (est == k)).sum(axis=(1, 2))
    return t


def test_2048_maps_in_the_count_kernels(gpu_state):
    c = case(54, 38, 2048)
    r, w = maps(gpu_state, 54, 38, 2048, (), 0, True), want_map(54, 38, 2048, (), 0, True)
    same(r["hist"], w["hist"])
    got = opt.label_score(gpu_state, c["gt"], c["est"], 1, 0)["table"]
    ref = count_fields(c["gt"], c["est"], 1)
    A, B = mscore_ref.bmap(c["gt"] == 1), mscore_ref.bmap(c["est"] == 1)          # radius 0: a hit is the same pixel
    ref[:, 1, 3], ref[:, 1, 4] = A.sum(axis=(1, 2)), B.sum(axis=(1, 2))
    ref[:, 1, 5] = ref[:, 1, 6] = (A & B).sum(axis=(1, 2))
    same(got, ref)
    for i in (0, 2047):
        same(got[i], mscore_ref.label_ref(c["gt"][i], c["est"][i], 1, 0)["table"][0])


def test_more_maps_than_grid_rows(gpu_state):
    """3x1 x 65540: the maps lie on the grid's second dimension, which holds 65535"""
    n = 65540
    rng = np.random.default_rng(9)
    gt, est = rng.integers(0, 3, (n, 1, 3)).astype(U8), rng.integers(0, 3, (n, 1, 3)).astype(U8)
    hist = opt.map_score(gpu_state, gt, est)["hist"]
    assert hist.shape == (n, 2, 256) and (hist.sum(axis=(1, 2)) == 3).all()
    for c in (0, 1):
        for v in (0, 1, 2):
            assert np.array_equal(hist[:, c, v], (((gt != 0) == bool(c)) & (est == v)).sum(axis=(1, 2)))
    ref = count_fields(gt, est, 1)
    A, B = mscore_ref.bmap(gt == 1), mscore_ref.bmap(est == 1)
    ref[:, 1, 3], ref[:, 1, 4] = A.sum(axis=(1, 2)), B.sum(axis=(1, 2))
    ref[:, 1, 5] = ref[:, 1, 6] = (A & B).sum(axis=(1, 2))
    same(opt.label_score(gpu_state, gt, est, 1, 0)["table"], ref)


# ---- properties that need no twin -------------------------------------------------------------------------------------------
def test_a_perfect_estimate_and_swapped_roles(gpu_state):
    c = case(130, 70, 1)
    t = opt.label_score(gpu_state, c["gt"], c["gt"], 4, 3, skip=c["skip"])["table"][0]
    assert (t[1:, 0] == t[1:, 1]).all() and (t[1:, 0] == t[1:, 2]).all() and t[1:, 0].min() > 0
    assert (t[1:, 3] == t[1:, 4]).all() and (t[1:, 5] == t[1:, 3]).all() and (t[1:, 6] == t[1:, 4]).all() and t[1:, 3].min() > 0
    assert t[0, 2] == t[0, 0] and t[0, 3] == t[0, 4] > 0
    a = opt.label_score(gpu_state, c["gt"], c["est"], 4, 3, skip=c["skip"])["table"][0]
    b = opt.label_score(gpu_state, c["est"], c["gt"], 4, 3, skip=c["skip"])["table"][0]
    assert np.array_equal(a[:, [1, 0, 2, 4, 3, 6, 5, 7]][1:], b[1:]) and np.array_equal(a[0, [0, 1, 2, 4, 3]], b[0, :5])
    r = opt.map_score(gpu_state, c["occ"], c["score"], skip=c["skip"])
    assert int(r["hist"].sum()) + int((c["skip"] != 0).sum()) == 130 * 70 and r["match"].shape == (1, 0, 4)
    one = opt.label_score(gpu_state, c["gt"][0], c["est"][0], 4, 3)["table"]
    assert one.shape == (1, 5, 8)
    with pytest.raises(ValueError):
        opt.label_score(gpu_state, c["gt"], c["est"][:, :5], 4, 3)
    with pytest.raises(ValueError):
        opt.map_score(gpu_state, c["occ"], c["score"], skip=c["skip"][:, :5])
    for bad in (dict(L=0), dict(L=256), dict(radius=255)):
        with pytest.raises(ValueError):
            opt.label_score(gpu_state, c["gt"], c["est"], **{"L": 3, "radius": 3, **bad})
    for bad in (dict(thr=(0,)), dict(thr=(256,)), dict(thr=(1,) * 9), dict(thr=(5,), radius=255)):
        with pytest.raises(ValueError):
            opt.map_score(gpu_state, c["occ"], c["score"], **bad)


def test_without_thresholds_no_set_and_no_distance_pass_is_launched(gpu_state):
    st = gpu_state
    count = lambda k: (st.kernel_time(k) or (0.0, 0))[1]
    names = ("k_mscore_hist", "k_mscore_labels", "k_mscore_sets", "k_seg_cols", "k_seg_rows", "k_mscore_hits")
    try:
        st.set_kernel_timing(True)
        maps(st, 71, 9, 3, (), 0, True)
        assert [count(k) for k in names] == [1, 0, 0, 0, 0, 0]
        st.set_kernel_timing(True)                  # clears the records
        maps(st, 71, 9, 3, (64, 128), 1, True)
        assert [count(k) for k in names] == [1, 0, 6, 12, 12, 6]
        st.set_kernel_timing(True)
        label(st, 71, 9, 3, 3, 1, False)
        assert [count(k) for k in names] == [0, 1, 9, 18, 18, 9]
    finally:
        st.set_kernel_timing(False)


# ---- the calls themselves, on device tensors ----------------------------------------------------------------------------------
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + off)


def raw_label(st, W, H, n, L, radius, gt, est, skip, table, scratch, state=True):
    torch.cuda.synchronize()
    rc = st.lib.ArapFlow_LabelScore(st.handle if state else None, W, H, n, L, radius, gt, est, skip, table, scratch)
    torch.cuda.synchronize()
    return rc


def raw_map(st, W, H, n, gt, est, skip, thr, radius, hist, match, scratch, m=None):
    torch.cuda.synchronize()
    arr = (C.c_uint * len(thr))(*thr) if thr else None
    rc = st.lib.ArapFlow_MapScore(st.handle, W, H, n, gt, est, skip, len(thr or ()) if m is None else m, arr, radius, hist, match, scratch)
    torch.cuda.synchronize()
    return rc


def test_garbage_in_outputs_and_scratch_two_calls_and_buffers_off_the_alignment(gpu_state):
    st, (W, H, n) = gpu_state, (71, 9, 3)
    c = case(W, H, n)
    N = n * W * H
    sb = int(st.lib.ArapFlow_MapScoreScratchBytes(W, H))
    assert sb % 256 == 0 and sb == int(st.lib.ArapFlow_MapScoreScratchBytes(W, H))
    wl, wm = want_label(W, H, n, 3, 8, True), want_map(W, H, n, (64, 255), 8, True)
    gt, est, skip, occ, score = (dev(c[k]) for k in ("gt", "est", "skip", "occ", "score"))
    runs = []
    for fill in (0xA5, 0x3C):
        table = torch.full((n, 4, 8), -1, dtype=torch.int64, device="cuda")
        hist = torch.full((n, 2, 256), -7, dtype=torch.int64, device="cuda")
        match = torch.full((n, 2, 4), -9, dtype=torch.int64, device="cuda")
        scratch = torch.full((sb,), fill, dtype=torch.uint8, device="cuda")
        assert raw_label(st, W, H, n, 3, 8, ptr(gt), ptr(est), ptr(skip), ptr(table), ptr(scratch)) == 0
        assert raw_map(st, W, H, n, ptr(occ), ptr(score), ptr(skip), (64, 255), 8, ptr(hist), ptr(match), ptr(scratch)) == 0
        runs.append([t.cpu().numpy().view(np.uint64) for t in (table, hist, match)])
        same(runs[-1][0], wl)
        same(runs[-1][1], wm["hist"])
        same(runs[-1][2], wm["match"])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*runs))
    # every plane one byte off: the one-pixel path, the same bytes
    off = [torch.zeros(N + 1, dtype=torch.uint8, device="cuda") for _ in range(5)]
    for t, k in zip(off, ("gt", "est", "skip", "occ", "score")):
        t[1:] = dev(c[k]).reshape(-1)
    table = torch.full((n, 4, 8), -1, dtype=torch.int64, device="cuda")
    hist = torch.full((n, 2, 256), -7, dtype=torch.int64, device="cuda")
    match = torch.full((n, 2, 4), -9, dtype=torch.int64, device="cuda")
    scratch = torch.empty(sb, dtype=torch.uint8, device="cuda")
    assert raw_label(st, W, H, n, 3, 8, ptr(off[0], 1), ptr(off[1], 1), ptr(off[2], 1), ptr(table), ptr(scratch)) == 0
    assert raw_map(st, W, H, n, ptr(off[3], 1), ptr(off[4], 1), ptr(off[2], 1), (64, 255), 8, ptr(hist), ptr(match), ptr(scratch)) == 0
    same(table.cpu().numpy().view(np.uint64), wl)
    same(hist.cpu().numpy().view(np.uint64), wm["hist"])
    same(match.cpu().numpy().view(np.uint64), wm["match"])
    # one plane off, the others not; and no scratch without thresholds
    assert raw_map(st, W, H, n, ptr(occ), ptr(off[4], 1), None, (), 0, ptr(hist), None, None) == 0
    same(hist.cpu().numpy().view(np.uint64), want_map(W, H, n, (), 0, False)["hist"])


def test_every_refusal_leaves_sentinel_filled_outputs_alone(gpu_state):
    st, (W, H, n) = gpu_state, (16, 4, 2)
    N = n * W * H
    sb = int(st.lib.ArapFlow_MapScoreScratchBytes(W, H))
    pool = torch.full((16384 + sb,), 0xEE, dtype=torch.uint8, device="cuda")           # inputs, outputs and scratch, all sentinel
    at = lambda off: ptr(pool, off)
    GT, EST, SKIP, OUT, MATCH, SCR = at(0), at(256), at(512), at(1024), at(1024 + 8192), at(16384)

    def lab(W=W, H=H, n=n, L=3, radius=8, gt=GT, est=EST, skip=SKIP, table=OUT, scratch=SCR, state=True):
        return raw_label(st, W, H, n, L, radius, gt, est, skip, table, scratch, state)

    def mp(W=W, H=H, n=n, gt=GT, est=EST, skip=SKIP, thr=(64, 128), radius=8, hist=OUT, match=MATCH, scratch=SCR, m=None):
        return raw_map(st, W, H, n, gt, est, skip, thr, radius, hist, match, scratch, m)

    assert lab(state=False) == -1 and st.lib.ArapFlow_MapScore(None, W, H, n, GT, EST, SKIP, 0, None, 0, OUT, None, None) == -1
    for call in (lab, mp):
        assert call(gt=None) == -1 and call(est=None) == -1
        assert call(n=0) == -1 and call(W=0) == -1 and call(H=0) == -1
        assert call(W=1 << 16, H=1 << 15) == -1 and call(W=1 << 15, H=1 << 15, n=2) == -1
        assert call(radius=255) == -1
        assert call(scratch=at(512 + N - 1)) == -1 and call(scratch=at(1024 + 8)) == -1 and call(gt=at(16384 + sb - 1)) == -1
    assert lab(table=None) == -1 and lab(scratch=None) == -1 and lab(L=0) == -1 and lab(L=256) == -1
    assert lab(table=at(256 + N - 1)) == -1 and lab(table=at(1024), skip=at(1024 + 2 * 4 * 64 - 1)) == -1
    assert mp(hist=None) == -1 and mp(m=9, thr=(1,) * 9) == -1 and mp(thr=(64, 0)) == -1 and mp(thr=(256,)) == -1
    assert mp(thr=None, m=1) == -1 and mp(match=None) == -1 and mp(scratch=None) == -1
    assert mp(hist=at(N - 1)) == -1 and mp(match=at(1024 + 8192 - 8)) == -1 and mp(match=at(16384 - 8)) == -1
    assert bool((pool == 0xEE).all())
    # and the same buffers are accepted once nothing is wrong (the maps are all 0xEE)
    assert lab() == 0
    t = pool[1024:1024 + n * 4 * 64].cpu().numpy().view(np.uint64).reshape(n, 4, 8)
    assert (t[:, 0, :5] == [0, W * H, 0, 0, 0]).all() and not t[:, 1:].any()         # every pixel skipped
    assert mp() == 0 and not pool[1024:1024 + 8192 + 128].any()


PLAIN_CHILD = r'''
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import test_gpu_mscore as T
from arap_flow_amd import opt
st = opt.State()
for W, H, n in ((71, 9, 3), (130, 70, 1)):
    r, w = T.maps(st, W, H, n, (), 0, True), T.want_map(W, H, n, (), 0, True)
    assert np.array_equal(r["hist"], w["hist"])
st.close()
print("plain ok")
'''


def test_the_plain_variant_of_the_histogram_kernel_counts_the_same(tmp_path):
    """ARAPOPT_MSCORE_PLAIN=1, the form the aggregation is measured against (profiles/map_score): a knob of the state, so
    a fresh process"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    child = tmp_path / "plain.py"
    child.write_text(PLAIN_CHILD % (root, os.path.join(root, "tests")))
    r = subprocess.run([sys.executable, str(child)], env=dict(os.environ, ARAPOPT_MSCORE_PLAIN="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "plain ok" in r.stdout, r.stdout[-1000:] + r.stderr[-2000:]
