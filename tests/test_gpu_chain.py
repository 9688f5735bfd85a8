"""GPU: ArapFlow_ChainFlows / opt.chain_flows (DESIGN.md "Track scoring") byte for byte against the numpy twin
tests/tscore_ref.py: two frame sizes, one to eight links, the block edge in P, every kind of point (integer, border,
sub-pixel, leaving mid-chain, NaN, a NaN flow sample), the closed form of constant flows, the forward-backward check on,
below and above its bound, the chain of a track state scored against that state's tracks, and the refusals."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import layers_step_ref as sref
import tscore_ref as R
from arap_flow_amd import opt

pytestmark = pytest.mark.gpu
F = np.float32


def same(got, ref):
    (pos, occ), (rpos, rocc) = got, ref
    assert pos.dtype == F and occ.dtype == np.uint8 and pos.shape == rpos.shape and occ.shape == rocc.shape
    # bit for bit; a NaN that arithmetic made (a NaN flow sample) is a NaN in both, its sign and payload are no part of IEEE 754
    bits = lambda a: np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32))
    assert np.array_equal(bits(pos), bits(rpos)), (bits(pos) != bits(rpos)).nonzero()
    assert np.array_equal(occ, rocc), (occ != rocc).nonzero()


@functools.lru_cache(maxsize=None)
def case(W, H, L, P, seed=0):
    """smooth flows of a few pixels on the 2^-6 lattice (every fma of the twin is exact on the first link), one NaN sample;
    points of every kind"""
    rng = np.random.default_rng([W, H, L, seed])
    ys, xs = np.mgrid[0:H, 0:W]
    flows = np.zeros((L, H, W, 2), F)
    for j in range(L):
        a, b = rng.uniform(-2, 2, 2)
        flows[j, ..., 0] = a + 1.5 * np.sin(xs / 5.0 + j) + rng.normal(size=(H, W)) * 0.2
        flows[j, ..., 1] = b + 1.0 * np.cos(ys / 3.0 - j) + rng.normal(size=(H, W)) * 0.2
    flows = (np.round(flows * 64) / 64).astype(F)
    flows[0, H // 2, W // 2] = np.nan
    bwd = (-flows + (rng.normal(size=flows.shape) * rng.choice([0.0, 0.05, 1.0], size=(L, H, W, 1)))).astype(F)
    bwd[0, 1, 1] = np.nan
    kinds = [np.stack([rng.integers(0, W, P), rng.integers(0, H, P)], -1).astype(F),                   # integer points
             np.stack([np.full(P, W - 1), rng.uniform(0, H - 1, P)], -1).astype(F),                    # the right border
             np.stack([rng.uniform(0, W - 1, P), np.full(P, H - 1)], -1).astype(F),                    # the bottom border
             (rng.uniform(0, 1, (P, 2)) * [W - 1, H - 1]).astype(F),                                    # sub-pixel
             (np.round(rng.uniform(0, 1, (P, 2)) * [W - 1, H - 1] * 4) / 4).astype(F)]                  # the quarter lattice
    pts = np.stack([kinds[k % len(kinds)][k] for k in range(P)])
    if P > 8:
        pts[3] = (np.nan, 1.0); pts[4] = (1.0, np.nan); pts[5] = (-0.25, 2.0); pts[6] = (W - 0.5, 1.0); pts[7] = (np.inf, 0.0)
        pts[8] = (W // 2, H // 2)                                # lands on the NaN sample
    for a in (flows, bwd, pts):
        a.setflags(write=False)
    return flows, bwd, pts


@pytest.mark.parametrize("with_bwd", [False, True], ids=["fwd", "fwd+bwd"])
@pytest.mark.parametrize("W,H,L,P", [(33, 17, 1, 255), (33, 17, 3, 256), (33, 17, 8, 257), (64, 8, 1, 257), (64, 8, 3, 255),
                                     (64, 8, 8, 256)])
def test_equals_the_twin(gpu_state, W, H, L, P, with_bwd):
    flows, bwd, pts = case(W, H, L, P)
    ref = R.chain_ref(flows, pts, bwd if with_bwd else None)
    same(opt.chain_flows(gpu_state, flows, pts, bwd=bwd if with_bwd else None), ref)
    pos, occ = ref
    assert (occ[0] == 255).sum() >= 5 and (occ[0] == 0).any() and np.isnan(pos[1][8]).all() and occ[1][8] == 255
    if L == 8:
        left = (occ[1] == 0) & (occ[-1] == 255)                  # left mid-chain ...
        assert left.any()
        if not with_bwd:                                         # ... and stays lost, where it left
            first = np.argmax(occ == 255, axis=0)
            for k in np.flatnonzero(left):
                assert (occ[first[k]:, k] == 255).all() and (pos[first[k]:, k].view(np.uint32) == pos[first[k], k].view(np.uint32)).all()
    if with_bwd:
        vis = occ[1:] == 0
        assert vis.any() and (R.chain_ref(flows, pts)[1][1:][~vis] == 0).any()         # the check hides points the frame test keeps


def test_integer_points_return_the_sample_itself(gpu_state):
    flows = np.nan_to_num(case(33, 17, 1, 255)[0])              # (fx = 0 still multiplies the right neighbour: no NaN sample here)
    ys, xs = np.mgrid[0:17, 0:33]
    pts = np.stack([xs.ravel(), ys.ravel()], -1).astype(F)
    pos, occ = opt.chain_flows(gpu_state, flows, pts)
    want = pts + flows[0].reshape(-1, 2)
    assert np.array_equal(pos[1].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(occ[1] == 0, R.in_frame(want, 33, 17))


def test_constant_dyadic_flows_add_up_exactly(gpu_state):
    W, H, L = 64, 8, 8
    steps = np.array([[1.5, 0.25], [-0.75, 0.5], [2.0, -0.125], [0.25, 0.25], [3.5, 0.0], [-1.25, 0.375], [0.5, -0.5], [4.0, 0.125]], F)
    flows = np.broadcast_to(steps[:, None, None, :], (L, H, W, 2)).copy()
    rng = np.random.default_rng(2)
    pts = (np.round(rng.uniform(0, 1, (257, 2)) * [63, 7] * 16) / 16).astype(F)
    pos, occ = opt.chain_flows(gpu_state, flows, pts)
    total = np.concatenate([np.zeros((1, 2), F), np.cumsum(steps, axis=0)])
    want = pts[None] + total[:, None, :]
    inside = np.logical_and.accumulate(R.in_frame(want, W, H), axis=0)
    assert inside[-1].any() and (~inside[-1]).any()
    assert np.array_equal(pos[inside], want[inside]) and (occ[inside] == 0).all() and (occ[~inside] == 255).all()
    same((pos, occ), R.chain_ref(flows, pts))


def test_forward_backward_check(gpu_state):
    """a consistent constant pair keeps every point visible, an inconsistent one hides them all, and a pair exactly on the
    bound is visible, one ulp beyond it hidden"""
    W, H = 33, 17
    pts = np.stack([np.arange(20) + 0.5, np.full(20, 3.25)], -1).astype(F)
    const = lambda v: np.broadcast_to(np.array(v, F), (1, H, W, 2)).copy()
    f = const([3.0, 1.0])
    pos, occ = opt.chain_flows(gpu_state, f, pts, bwd=const([-3.0, -1.0]))
    assert (occ == 0).all() and np.array_equal(pos[1], pts + F([3.0, 1.0]))
    pos, occ = opt.chain_flows(gpu_state, f, pts, bwd=const([0.0, 3.0]))
    assert (occ[0] == 0).all() and (occ[1] == 255).all() and np.array_equal(pos[1], pts + F([3.0, 1.0]))
    # on the bound: f = (0.25, 3), g = (-0.25, gy) has s = (0, 3 + gy) exactly; at this gy d2 == fmaf(0.01f, m2, 0.5f) in
    # float32 (found by search, asserted here), one ulp of gy nearer zero d2 is beyond the bound, one ulp away within it
    f, gy = F([0.25, 3.0]), F(-2.2002129554748535)
    for k, hidden in ((0, 0), (1, 0), (-1, 255)):
        g = np.array([-0.25, R.ulp(gy, k)], F)
        sy = f[1] + g[1]
        d2 = F(0) * F(0) + sy * sy
        m2 = (f[0] * f[0] + f[1] * f[1]) + (g[0] * g[0] + g[1] * g[1])
        bound = R.fma(F(0.01), m2, F(0.5))
        assert (d2 == bound, d2 < bound, d2 > bound)[k], (k, d2, bound)
        pos, occ = opt.chain_flows(gpu_state, const(f), pts[:4], bwd=const(g))
        assert (occ[1] == hidden).all(), (k, hidden)
        same((pos, occ), R.chain_ref(const(f), pts[:4], const(g)))


def test_chain_of_a_track_state_scores_within_a_pixel(gpu_state):
    """end to end: the tracks of one layer's state at its integer object pixels, that state's flow chained over one link,
    the chain scored against the tracks -- byte for byte the twins', and every visible point within one pixel"""
    W, H, n, seed, overlap = sref.MULTI[3]
    _, masks, fa, _ = sref.two_state_layers(W, H, n, seed, overlap=overlap)
    layer = 1
    mask, flow = masks[layer:layer + 1], fa[layer:layer + 1]
    # the object pixels the mesh moves: corners of a rasterised quad (a quad whose four corners are object).  An object pixel
    # of no such quad has no owner and its track stays at p by definition (DESIGN.md "Point tracks"), so no flow chain meets it
    obj = mask[0] == 0
    quad = obj[:-1, :-1] & obj[1:, :-1] & obj[:-1, 1:] & obj[1:, 1:]
    moved = np.zeros_like(obj)
    for dy in (0, 1):
        for dx in (0, 1):
            moved[dy:H - 1 + dy, dx:W - 1 + dx] |= quad
    assert moved.sum() > 256 and (obj & ~moved).any()
    ys, xs = np.nonzero(moved)
    pts = np.stack([xs, ys], -1).astype(F)
    trk = opt.track_points(gpu_state, mask, flow[None], pts)
    gt_pos = np.concatenate([pts[None], trk["pos"]])
    gt_occ = np.concatenate([np.zeros((1, len(pts)), np.uint8), trk["occ"]])
    est = opt.chain_flows(gpu_state, flow, pts)
    same(est, R.chain_ref(flow, pts))
    table = opt.track_score(gpu_state, gt_pos, gt_occ, *est)
    assert np.array_equal(table, R.track_score_ref(gt_pos, gt_occ, *est))
    assert table[0, 0, 0] == len(pts) and table[1, 0, R.GT_VIS] > 0
    assert table[1, 0, R.WITHIN] == table[1, 0, R.GT_VIS]


def test_refusals(gpu_state):
    W, H, L, P = 33, 17, 3, 256
    flows, bwd, pts = case(W, H, L, P)
    d_f, d_b, d_p = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (flows, bwd, pts))
    pos = torch.full((L + 1, P, 2), 7.0, dtype=torch.float32, device="cuda")
    occ = torch.full((L + 1, P), 9, dtype=torch.uint8, device="cuda")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr() if isinstance(t, torch.Tensor) else int(t))

    def call(W, H, L, f, b, P, q, op, oo):
        rc = gpu_state.lib.ArapFlow_ChainFlows(gpu_state.handle, W, H, L, p(f), p(b), P, p(q), p(op), p(oo))
        torch.cuda.synchronize()
        return rc
    untouched = lambda: bool((pos == 7.0).all()) and bool((occ == 9).all()) and np.array_equal(d_p.cpu().numpy().view(np.uint32), pts.view(np.uint32))
    assert call(W, H, L, None, d_b, P, d_p, pos, occ) == -1 and untouched()
    assert call(W, H, L, d_f, d_b, P, None, pos, occ) == -1 and untouched()
    assert call(W, H, L, d_f, d_b, P, d_p, None, occ) == -1 and untouched()
    assert call(W, H, L, d_f, d_b, P, d_p, pos, None) == -1 and untouched()
    for bad_l in (0, 64):
        assert call(W, H, bad_l, d_f, d_b, P, d_p, pos, occ) == -1 and untouched()
    for bad_p in (0, (1 << 24) + 1):
        assert call(W, H, L, d_f, d_b, bad_p, d_p, pos, occ) == -1 and untouched()
    for w, h in ((0, H), (W, 0), (1 << 16, 1 << 15)):
        assert call(w, h, L, d_f, d_b, P, d_p, pos, occ) == -1 and untouched()
    assert call(W, H, L, d_f, d_b, P, d_p, d_f, occ) == -1 and untouched()                          # pos on the flows
    assert call(W, H, L, d_f, d_b, P, d_p, pos, d_b.data_ptr() + 16) == -1 and untouched()          # occ inside bwd
    assert call(W, H, L, d_f, d_b, P, d_p, pos, d_p.data_ptr() + P * 8 - 1) == -1 and untouched()   # occ on the points' last byte
    assert call(W, H, L, d_f, d_b, P, d_p, pos, pos.data_ptr() + 8) == -1 and untouched()           # occ inside pos
    assert call(W, H, L, d_f, None, P, d_p, pos, occ) == 0                                          # bwd may be NULL
    same((pos.cpu().numpy(), occ.cpu().numpy()), R.chain_ref(flows, pts))
    with pytest.raises(ValueError):
        opt.chain_flows(gpu_state, flows, pts, bwd=bwd[:2])
    with pytest.raises(ValueError):
        opt.chain_flows(gpu_state, flows[0], pts)
