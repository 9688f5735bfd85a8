"""GPU: ArapFlow_FlowScore / opt.flow_score (DESIGN.md "Flow scoring") byte for byte against the numpy twin
tests/score_ref.py: at the shapes the kernel branches on (less than a wave, pairs misaligned for its wide loads, a block
edge, many blocks a pair, several groups a lane, more pairs than grid rows), with every combination of planes it has a path
for, on pixels crafted at every edge of the definition, on pixels a contracting build gets wrong, with sums beyond 32 bits;
the call's own clearing of the table, its determinism and its refusals."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import score_ref
from arap_flow_amd import opt, pipeline

pytestmark = pytest.mark.gpu
F = np.float32
ulp = score_ref.ulp
FIELD = {k: i for i, k in enumerate(pipeline.SCORE_FIELDS)}
ROW = {k: i for i, k in enumerate(pipeline.SCORE_ROWS)}


@functools.lru_cache(maxsize=None)
def case(W, H, n, seed=0):
    """random pairs with every class populated: speeds around both edges, errors around every threshold, a few
    non-finite values on both sides; read-only"""
    rng = np.random.default_rng([W, H, n, seed])
    gt = (rng.normal(size=(n, H, W, 2)) * rng.choice([3.0, 15.0, 40.0], size=(n, H, W, 1))).astype(F)
    est = (gt + rng.normal(size=gt.shape) * rng.choice([0.3, 1.5, 4.0], size=(n, H, W, 1))).astype(F)
    bad = rng.random((n, H, W))
    est[bad < 0.01] = np.nan
    est[(bad >= 0.01) & (bad < 0.02), 0] = np.inf
    gt[(bad >= 0.02) & (bad < 0.03), 1] = -np.inf
    gt[(bad >= 0.03) & (bad < 0.04)] = np.nan
    occ = rng.choice(np.array([0, 0, 1, 255], np.uint8), size=(n, H, W))
    dist = rng.choice(np.array([0, 50, 99, 100, 2000, 3599, 3600, 10000, 19599, 19600, 40000, 65535], np.uint16), size=(n, H, W))
    skip = rng.choice(np.array([0, 0, 0, 0, 0, 0, 0, 2, 255], np.uint8), size=(n, H, W))
    out = dict(gt=gt, est=est, occ=occ, dist=dist, skip=skip)
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def want(W, H, n, planes):
    c = case(W, H, n)
    return score_ref.score_ref(c["gt"], c["est"], **{k: c[k] for k in planes})


def same(got, ref, err=True):
    assert got["table"].dtype == np.uint64 and got["table"].shape == ref["table"].shape
    assert np.array_equal(got["table"], ref["table"]), (got["table"] != ref["table"]).nonzero()
    if err:
        assert got["err"].dtype == F and np.array_equal(got["err"].view(np.uint32), ref["err"].view(np.uint32))


PLANES = [(), ("occ",), ("dist",), ("skip",), ("occ", "dist", "skip")]
SHAPES = [(5, 3, 1), (71, 9, 3), (64, 4, 1), (65, 4, 1)]


@pytest.mark.parametrize("planes", PLANES, ids=lambda p: "+".join(p) or "none")
@pytest.mark.parametrize("W,H,n", SHAPES)
def test_table_and_err_equal_the_twin(gpu_state, W, H, n, planes):
    """5x3: less than a wave; 71x9x3: W * H odd, pairs 1 and 2 start 1 and 2 pixels off the 4-pixel groups; 64x4 / 65x4: one
    full block of groups and one pixel more"""
    c = case(W, H, n)
    ref = want(W, H, n, planes)
    same(opt.flow_score(gpu_state, c["gt"], c["est"], err=True, **{k: c[k] for k in planes}), ref)
    same(opt.flow_score(gpu_state, c["gt"], c["est"], **{k: c[k] for k in planes}), ref, err=False)     # without the map
    assert ref["table"][:, ROW["all"], FIELD["count"]].min() > 0
    if planes == PLANES[-1] and W * H > 100:
        t = ref["table"].sum(axis=0)
        assert (t[:9, FIELD["count"]] > 0).all() and (t[9, :2] > 0).all() and t[0, FIELD["nonfinite"]] > 0


@pytest.mark.parametrize("planes", [PLANES[0], PLANES[-1]], ids=["none", "all"])
@pytest.mark.parametrize("W,H,n", [(854, 480, 2), (54, 38, 2048), (3, 1, 65540)])
def test_many_blocks_many_groups_many_pairs(gpu_state, W, H, n, planes):
    """854x480x2: 401 blocks a pair meet in the table's atomics; 54x38x2048: one block a pair and three groups a lane;
    3x1x65540: more pairs than grid rows, all of them head and tail"""
    c = case(W, H, n)
    same(opt.flow_score(gpu_state, c["gt"], c["est"], err=True, **{k: c[k] for k in planes}), want(W, H, n, planes))


def test_a_single_pair_without_the_leading_axis(gpu_state):
    c = case(71, 9, 3)
    got = opt.flow_score(gpu_state, c["gt"][1], c["est"][1], occ=c["occ"][1], err=True)
    ref = score_ref.score_ref(c["gt"][1], c["est"][1], occ=c["occ"][1])
    same(got, ref)
    assert got["table"].shape == (1, 10, 8) and got["err"].shape == (1, 9, 71)
    with pytest.raises(ValueError):
        opt.flow_score(gpu_state, c["gt"], c["est"][:2])
    with pytest.raises(ValueError):
        opt.flow_score(gpu_state, c["gt"], c["est"], occ=c["occ"][:2])


# ---- crafted pixels --------------------------------------------------------------------------------------------------------
def hit_e2(target, gt=(0.0, 0.0)):
    """an est whose e2 against gt is exactly the float32 `target`, by search over representable est"""
    gx, gy, t = F(gt[0]), F(gt[1]), F(target)
    r = np.sqrt(np.float64(t))
    ex = gx + (np.linspace(0.3, 0.9, 8001) * r).astype(F)
    du = ex - gx
    dv0 = np.sqrt(np.maximum(np.float64(t) - du.astype(np.float64) ** 2, 0.0)).astype(F)
    for k in range(-3, 4):
        ey = ulp(gy + dv0, k)
        dv = ey - gy
        idx = np.flatnonzero(du * du + dv * dv == t)
        if len(idx):
            return float(ex[idx[0]]), float(ey[idx[0]])
    raise AssertionError("no est with e2 = %r against %r" % (target, gt))


def crafted():
    """[(gt, est, occ, dist, skip)] at every edge of the definition"""
    px = []
    add = lambda gt, est, occ=0, dist=65535, skip=0: px.append((gt, est, occ, dist, skip))
    for t in (1.0, 9.0, 25.0):                                  # e2 at, one ulp below and above each outlier threshold
        for k in (-1, 0, 1):
            add((0.0, 0.0), hit_e2(ulp(F(t), k)))
    add((6.0, 8.0), (6.0, 8.0)); add((24.0, 32.0), (24.0, 32.0))           # g2 exactly 100 and 1600
    add((6.0, float(ulp(F(8), -1))), (6.0, 8.0)); add((24.0, float(ulp(F(32), -1))), (24.0, 32.0))       # and just below
    for d in (0, 99, 100, 3599, 3600, 19599, 19600, 65534, 65535):
        add((1.0, 1.0), (1.5, 1.0), dist=d, occ=d & 1)
    g = (240.0, 320.0)                                          # g2 = 160000: Fl's relative bound is near e2 = 400
    thr = F(0.0025) * (F(g[0]) * F(g[0]) + F(g[1]) * F(g[1]))
    for k in (-1, 0, 1):
        add(g, hit_e2(ulp(thr, k), g))
    add(g, (g[0] + 3.5, g[1]))                                  # beyond 3 px but within 5 %: n3, no fl
    for k in (-1, 0, 1):                                        # e just below, at and above the cap
        add((0.0, 0.0), (float(ulp(F(4096), k)), 0.0))
    add((0.0, 0.0), (1e30, 0.0)); add((0.0, 0.0), (3e38, 3e38))             # e2 overflows
    nan, inf = float("nan"), float("inf")
    for est in ((nan, 0.0), (0.0, nan), (inf, 0.0), (-inf, 1.0), (inf, -inf), (-0.0, -0.0), (1e-40, 0.0), (1e-20, 0.0),
                (1e-45, 1e-45), (2e-19, 1e-19)):
        add((0.0, 0.0), est)
    add((1e-40, 0.0), (0.0, -1e-40))                            # a denormal difference
    for gt in ((nan, 0.0), (0.0, inf), (-inf, nan), (3e38, 0.0)):           # the last: finite, but g2 is not
        add(gt, (0.0, 0.0)); add(gt, gt)
    add((nan, nan), (1.0, 1.0), skip=1); add((0.0, 0.0), (nan, 0.0), skip=255); add((2.0, 2.0), (2.0, 2.0), skip=7)
    return px


def test_crafted_pixels_at_every_edge(gpu_state):
    px = crafted()
    W, H = 13, 5
    assert len(px) <= W * H
    c = case(W, H, 1, seed=3)
    gt, est, occ, dist, skip = (c[k].copy() for k in ("gt", "est", "occ", "dist", "skip"))
    for i, (g, e, o, d, s) in enumerate(px):
        gt[0].reshape(-1, 2)[i], est[0].reshape(-1, 2)[i] = g, e
        occ[0].reshape(-1)[i], dist[0].reshape(-1)[i], skip[0].reshape(-1)[i] = o, d, s
    same(opt.flow_score(gpu_state, gt, est, occ=occ, dist=dist, skip=skip, err=True), score_ref.score_ref(gt, est, occ, dist, skip))
    # and each crafted pixel alone, read against the definition's words
    one = lambda k: score_ref.score_ref(np.array([[px[k][0]]], F), np.array([[px[k][1]]], F), *(np.array([[v]]) for v in px[k][2:]))["table"][0]
    t = [one(k) for k in range(len(px))]
    n = lambda k, f: int(t[k][0, FIELD[f]])
    assert [n(k, "n1") for k in range(3)] == [0, 0, 1] and [n(k, "n3") for k in range(3, 6)] == [0, 0, 1]
    assert [n(k, "n5") for k in range(6, 9)] == [0, 0, 1]
    assert [int(t[k][ROW["s10-40"], 0]) for k in (9, 11)] == [1, 0] and [int(t[k][ROW["s40+"], 0]) for k in (10, 12)] == [1, 0]
    rows = [int(np.flatnonzero(t[13 + k][3:6, 0])[0]) if t[13 + k][3:6, 0].any() else -1 for k in range(9)]
    assert rows == [0, 0, 1, 1, 2, 2, -1, -1, -1]
    assert [n(22 + k, "fl") for k in range(4)] == [0, 0, 1, 0] and [n(22 + k, "n3") for k in range(4)] == [1, 1, 1, 1]
    # (one ulp below 4096 px is 2^24 - 1 units, and + 0.5f rounds that to even: q is the cap from there on, never above it)
    assert [n(26 + k, "max") for k in range(3)] == [score_ref.CAP, score_ref.CAP, score_ref.CAP]
    assert [n(26 + k, "nonfinite") for k in range(5)] == [0, 0, 0, 1, 1]
    assert all(tuple(t[k][9, :2]) == (1, 0) and t[k][:9].sum() == 0 for k in range(len(px) - 3, len(px)))      # skipped, nothing else


def test_a_contracting_build_fails_on_n3(gpu_state):
    """du * du + dv * dv rounded product by product is <= 9 where either fused form is > 9: a build without
    -ffp-contract=off counts these pixels in n3"""
    d = score_ref.contraction_pixels(24)
    assert len(d) >= 16
    c = case(71, 9, 1, seed=4)
    gt, est = c["gt"].copy(), c["est"].copy()
    gt[0, 4, 10:10 + len(d)] = 0
    est[0, 4, 10:10 + len(d)] = d
    alone = score_ref.score_ref(np.zeros((1, len(d), 2), F), d[None])
    assert alone["table"][0, 0, FIELD["n3"]] == 0 and alone["table"][0, 0, FIELD["n1"]] == len(d)
    same(opt.flow_score(gpu_state, np.zeros((1, len(d), 2), F), d[None], err=True), alone)
    same(opt.flow_score(gpu_state, gt, est, err=True), score_ref.score_ref(gt, est))


def test_sums_beyond_32_bits(gpu_state):
    """a 854x480 estimate that is NaN everywhere: every pixel is capped, an outlier and non-finite"""
    W, H = 854, 480
    gt = np.zeros((H, W, 2), F)
    est = np.full((H, W, 2), np.nan, F)
    t = opt.flow_score(gpu_state, gt, est, err=True)
    N = W * H
    row = [N, N << 24, N, N, N, N, N, 1 << 24]
    assert (N << 24) > 1 << 32
    want_t = np.zeros((10, 8), np.uint64)
    want_t[ROW["all"]] = want_t[ROW["s0-10"]] = row
    assert np.array_equal(t["table"][0], want_t) and np.isnan(t["err"]).all()


# ---- the call itself: clearing, determinism, refusals ------------------------------------------------------------------------
def raw(state, W, H, n, gt, est, occ, dist, skip, table, err):
    """ArapFlow_FlowScore on device pointers: tensors, integers (addresses) or None"""
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr() if isinstance(t, torch.Tensor) else int(t))
    rc = state.lib.ArapFlow_FlowScore(state.handle, W, H, n, *[p(t) for t in (gt, est, occ, dist, skip, table, err)])
    torch.cuda.synchronize()
    return rc


def dev(c, keys=("gt", "est", "occ", "dist", "skip")):
    return [torch.from_numpy(c[k].view(np.int16) if k == "dist" else np.ascontiguousarray(c[k])).cuda() for k in keys]


def test_two_calls_identical_and_the_table_cleared(gpu_state):
    W, H, n = 71, 9, 3
    c = case(W, H, n)
    bufs = dev(c)
    ref = want(W, H, n, PLANES[-1])
    tables = []
    for fill in (-1, 0x5a5a5a5a5a5a5a5a):
        table = torch.full((n, 10, 8), fill, dtype=torch.int64, device="cuda")
        assert raw(gpu_state, W, H, n, *bufs, table, None) == 0
        tables.append(table.cpu().numpy().view(np.uint64))
    assert tables[0].tobytes() == tables[1].tobytes() == ref["table"].tobytes()


def test_buffers_off_the_wide_loads_alignment(gpu_state):
    """flows that start 8 bytes, planes that start 1 and 2 bytes into their allocations: the one-pixel path, same bytes"""
    W, H, n = 71, 9, 3
    c = case(W, H, n)
    ref = want(W, H, n, PLANES[-1])
    off = lambda a, lead: torch.from_numpy(np.concatenate([np.zeros(lead, a.dtype), a.reshape(-1)])).cuda()
    gt, est = off(c["gt"], 2), off(c["est"], 2)
    occ, dist, skip = off(c["occ"], 1), off(c["dist"].view(np.int16), 1), off(c["skip"], 1)
    table = torch.full((n, 10, 8), -1, dtype=torch.int64, device="cuda")
    err = torch.full((n * H * W + 1,), 7.0, dtype=torch.float32, device="cuda")
    assert raw(gpu_state, W, H, n, gt.data_ptr() + 8, est.data_ptr() + 8, occ.data_ptr() + 1, dist.data_ptr() + 2, skip.data_ptr() + 1,
               table, err.data_ptr() + 4) == 0
    assert np.array_equal(table.cpu().numpy().view(np.uint64), ref["table"])
    e = err.cpu().numpy()
    assert e[0] == 7.0 and np.array_equal(e[1:].view(np.uint32), ref["err"].reshape(-1).view(np.uint32))


def test_refusals_leave_everything_untouched(gpu_state):
    W, H, n = 64, 4, 1
    c = case(W, H, n)
    gt, est = dev(c, ("gt", "est"))
    sentinel = lambda: torch.full((n, 10, 8), 0x0123456789abcdef, dtype=torch.int64, device="cuda")
    table = sentinel()
    untouched = lambda: (np.array_equal(table.cpu().numpy(), sentinel().cpu().numpy()) and
                         np.array_equal(gt.cpu().numpy().view(np.uint32), c["gt"].view(np.uint32)) and
                         np.array_equal(est.cpu().numpy().view(np.uint32), c["est"].view(np.uint32)))
    assert raw(gpu_state, W, H, n, gt, est, None, None, None, est.data_ptr() + 64, None) == -1 and untouched()      # table inside est
    assert raw(gpu_state, W, H, n, gt, est, None, None, None, est.data_ptr() + W * H * 8 - 8, None) == -1 and untouched()     # its last bytes
    assert raw(gpu_state, W, H, n, gt, est, None, None, None, table, gt.data_ptr() + W * H * 4) == -1 and untouched()          # err inside gt
    assert raw(gpu_state, W, H, n, gt, est, None, None, None, table, table) == -1 and untouched()                              # err on the table
    assert raw(gpu_state, 1 << 16, 1 << 15, 1, gt, est, None, None, None, table, None) == -1 and untouched()                   # n * W * H = 2^31
    assert raw(gpu_state, 1 << 15, 1 << 15, 2, gt, est, None, None, None, table, None) == -1 and untouched()
    for bad in ((0, H, n), (W, 0, n), (W, H, 0)):
        assert raw(gpu_state, *bad, gt, est, None, None, None, table, None) == -1 and untouched()
    assert raw(gpu_state, W, H, n, None, est, None, None, None, table, None) == -1 and untouched()
    assert raw(gpu_state, W, H, n, gt, None, None, None, None, table, None) == -1 and untouched()
    assert raw(gpu_state, W, H, n, gt, est, None, None, None, None, None) == -1 and untouched()
    assert raw(gpu_state, W, H, n, gt, est, None, None, None, table, None) == 0                 # and the same buffers are fine
    assert np.array_equal(table.cpu().numpy().view(np.uint64), want(W, H, n, ())["table"])


def test_kernel_timing_sees_the_launch(gpu_state):
    c = case(64, 4, 1)
    gpu_state.set_kernel_timing(True)
    try:
        opt.flow_score(gpu_state, c["gt"], c["est"])
        opt.flow_score(gpu_state, c["gt"], c["est"], occ=c["occ"])
        ms, launches = gpu_state.kernel_time("k_flow_score")
    finally:
        gpu_state.set_kernel_timing(False)
    assert launches == 2 and ms > 0
