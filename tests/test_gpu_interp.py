"""GPU: ArapFlow_InterpFrames (opt.interp_frames) against the numpy twin tests/interp_ref.py, byte for byte, at the sizes its
two kernels branch on -- a single pixel, a single row and column, a row shorter than a gather block, one that crosses a
block boundary with a ragged tail, a width below the fill distance -- with crafted flows that reach every branch of the
definition (DESIGN.md "Frames from flows")."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import interp_ref as R
import tscore_ref as tr
from arap_flow_amd import opt

pytestmark = pytest.mark.gpu
F = np.float32
NONE = R.NONE
ALL_TIMES = tuple(float(F(i) / F(33)) for i in range(1, 33))           # K = 32: the ramp of an n = 33 line


def same(got, ref):
    (out, src), (rout, rsrc) = got, ref
    assert out.dtype == np.uint8 and src.dtype == np.uint8 and out.shape == rout.shape and src.shape == rsrc.shape
    assert np.array_equal(src, rsrc), (src != rsrc).nonzero()
    assert np.array_equal(out, rout), (out != rout).nonzero()


@functools.lru_cache(maxsize=None)
def case(W, H, seed=0):
    """(A, B, fwd, bwd): textured frames with a flat patch (equal costs), flows on the 2^-6 lattice -- smooth motion,
    noise, an expanding stretch u.x = i (one-pixel holes, targets leaving the frame, t * u on x.5), a stretch of invalid
    flows (NaN, inf, 1e9) wider than twice the fill distance where the width allows, flows far out of the frame -- and
    backward flows that agree with the forward ones in places and not in others"""
    rng = np.random.default_rng([W, H, seed])
    ys, xs = np.mgrid[0:H, 0:W]
    A = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    B = np.roll(A, (1, 2), (0, 1))
    B = np.where(rng.random((H, W, 1)) < 0.3, rng.integers(0, 256, (H, W, 3)), B).astype(np.uint8)
    A[:, W // 2:W // 2 + 9], B[:, W // 2:W // 2 + 11] = 90, 90              # flat: every cost in it is equal
    fwd = np.zeros((H, W, 2), F)
    noisy = (ys >= H // 2) & (H > 1)                                         # the upper rows move smoothly
    fwd[..., 0] = (2 + np.where(noisy, 1.5 * np.sin(xs / 5.0), 0.5 * np.sin(xs / 20.0)) + rng.normal(size=(H, W)) * rng.choice([0.0, 0.1, 2.0], size=(H, W)) * noisy) * (W > 1)
    fwd[..., 1] = (1 + np.cos(ys / 3.0) + rng.normal(size=(H, W)) * rng.choice([0.0, 0.1, 2.0], size=(H, W)) * noisy) * (H > 1)
    fwd = (np.round(fwd * 64) / 64).astype(F)
    if H > 1:
        fwd[0, :, 0], fwd[0, :, 1] = xs[0], 0                               # row 0 expands: pixel i moves by i
    bwd = (-fwd + rng.normal(size=fwd.shape) * rng.choice([0.0, 0.0, 0.05, 1.5], size=(1, W // 8 + 1, 1)).repeat(8, 1)[:, :W]).astype(F)
    bwd = (np.round(bwd * 64) / 64).astype(F)
    bad = np.array([np.nan, np.inf, -np.inf, 1e9, -1e9, 2e9], F)
    lo, hi = W // 5, W // 5 + min(60, W // 3)                               # the invalid stretch, on all rows but the last
    if hi > lo:
        fwd[:max(H - 1, 1), lo:hi] = rng.choice(bad, (max(H - 1, 1), hi - lo, 2))
        bwd[:max(H - 1, 1), lo:hi + 3] = rng.choice(bad, (max(H - 1, 1), min(hi + 3, W) - lo, 2))
    far = rng.random((H, W)) < 0.01
    fwd[far] = rng.choice(np.array([-300, 40.5, 1000, -7.25], F), (int(far.sum()), 2))
    for a in (A, B, fwd, bwd):
        a.setflags(write=False)
    return A, B, fwd, bwd


SHAPES = [(1, 1), (17, 1), (1, 40), (70, 9), (300, 5), (13, 6), (257, 2), (256, 3)]


@pytest.mark.parametrize("with_bwd", [False, True], ids=["fwd", "fwd+bwd"])
@pytest.mark.parametrize("W,H", SHAPES)
def test_equals_the_twin(gpu_state, W, H, with_bwd):
    A, B, fwd, bwd = case(W, H)
    bw = bwd if with_bwd else None
    for times in ((0.5,), (0.25, float(F(9) / F(19)), 0.875)):
        same(opt.interp_frames(gpu_state, A, B, fwd, times, bwd=bw, want_src=True), R.interp_ref(A, B, fwd, times, bw))


@pytest.mark.parametrize("W,H", [(70, 9), (300, 5), (1, 1)])
def test_thirty_two_times_in_one_call(gpu_state, W, H):
    A, B, fwd, bwd = case(W, H)
    ref = R.interp_ref(A, B, fwd, ALL_TIMES, bwd)
    got = opt.interp_frames(gpu_state, A, B, fwd, ALL_TIMES, bwd=bwd, want_src=True)
    same(got, ref)
    again = opt.interp_frames(gpu_state, A, B, fwd, ALL_TIMES, bwd=bwd, want_src=True)           # two runs, identical bytes
    assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1])
    only = opt.interp_frames(gpu_state, A, B, fwd, ALL_TIMES, bwd=bwd)                          # src NULL
    assert isinstance(only, np.ndarray) and np.array_equal(only, ref[0])


def test_crafted_case_reaches_every_branch(gpu_state):
    """on the twin: every src value occurs, with and without bwd as far as the definition allows; collisions, holes of one
    pixel, a gap beyond the fill distance, equidistant fill sources, targets out of the frame all occur at 300 x 5"""
    A, B, fwd, bwd = case(300, 5)
    times = (0.5, 0.25)
    out, src = R.interp_ref(A, B, fwd, times, bwd)
    assert set(np.unique(src)) == {0, 1, 2, 3, 4, 5, 6, 7, 255}
    _, src_f = R.interp_ref(A, B, fwd, times)
    assert set(np.unique(src_f)) >= {0, 2, 3, 4, 6, 7, 255}
    keys = R.splat_keys(A, B, fwd, times, bwd)
    has = keys != NONE
    assert ((keys >> np.uint64(31)) & np.uint64(1))[has].any() and not ((keys >> np.uint64(31)) & np.uint64(1))[has].all()
    ii, jj = R.grid(300, 5)
    u = fwd.reshape(-1, 2)
    ok = R.valid(u)
    with np.errstate(all="ignore"):
        p = np.stack([tr.fma(F(0.5), u[:, 0], ii.astype(F)), tr.fma(F(0.5), u[:, 1], jj.astype(F))], -1)
    inside = ok & tr.in_frame(p, 300, 5)
    assert (ok & ~inside).sum() > 20                                                     # targets leaving the frame
    r = R.nearest(p[inside, 1], 4) * 300 + R.nearest(p[inside, 0], 299)
    assert (np.bincount(r, minlength=1500) > 1).sum() > 50                               # several sources on one target
    assert ((p[inside, 0] % 1) == 0.5).sum() > 20                                        # t * u on x.5
    h0 = has[0]
    single = ~h0[:, 1:-1] & h0[:, :-2] & h0[:, 2:]                                       # a one-pixel hole: equidistant sources
    assert single.sum() > 20 and (src[0] == 255).sum() > 20
    run = np.zeros(5, int)
    widest = 0
    for x in range(300):
        run = np.where(h0[:, x], 0, run + 1)
        widest = max(widest, run.max())
    assert widest > 2 * R.FILL + 1                                                       # a gap no fill closes
    same(opt.interp_frames(gpu_state, A, B, fwd, times, bwd=bwd, want_src=True), (out, src))


def flat(W, H, v=90):
    return np.full((H, W, 3), v, np.uint8)


def test_the_minimum_is_cost_then_side_then_index(gpu_state):
    W, H, t = 12, 1, (0.5,)
    rng = np.random.default_rng(4)
    nan = np.full((H, W, 2), np.nan, F)
    # two sources on target 2: pixel 0 moves by 4, pixel 2 stays
    fwd = nan.copy()
    fwd[0, 0], fwd[0, 2] = (4, 0), (0, 0)
    A = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    for cheap in (0, 2):                                        # different costs: the cheaper one wins, whichever index it has
        B = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
        B[0, 4 if cheap == 0 else 2] = A[0, cheap]              # cost 0 for it
        key = R.splat_keys(A, B, fwd, t)[0, 0, 2]
        assert int(key) == cheap
        same(opt.interp_frames(gpu_state, A, B, fwd, t, want_src=True), R.interp_ref(A, B, fwd, t))
    # equal costs: the lower index
    assert int(R.splat_keys(flat(W, H), flat(W, H), fwd, t)[0, 0, 2]) == 0
    same(opt.interp_frames(gpu_state, flat(W, H), flat(W, H), fwd, t, want_src=True), R.interp_ref(flat(W, H), flat(W, H), fwd, t))
    # equal costs across the sides: side A, though side B's source has the lower index
    fwd = nan.copy()
    fwd[0, 6] = (0, 0)
    bwd = nan.copy()
    bwd[0, 2] = (8, 0)                                          # lands on 6 at s = .5
    key = int(R.splat_keys(flat(W, H), flat(W, H), fwd, t, bwd)[0, 0, 6])
    assert key == 6
    assert int(R.splat_keys(flat(W, H), flat(W, H), nan, t, bwd)[0, 0, 6]) == (1 << 31) | 2
    for f in (fwd, nan):
        same(opt.interp_frames(gpu_state, flat(W, H), flat(W, H), f, t, bwd=bwd, want_src=True), R.interp_ref(flat(W, H), flat(W, H), f, t, bwd))


def test_fill_distance_and_the_left_source_at_equal_distance(gpu_state):
    """one keyed pixel every 34: the 16 pixels on either side take its key, the one between two fills stays a hole; one
    every 2: every hole is equidistant and takes the left key; on both sides of a gather block's boundary"""
    t = (0.5,)
    for W, step in ((300, 34), (300, 2), (600, 33), (40, 34), (15, 20)):
        H = 2
        rng = np.random.default_rng(W + step)
        A, B = (rng.integers(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(2))
        fwd = np.full((H, W, 2), np.nan, F)
        fwd[0, ::step] = 0
        fwd[1, (step // 2)::step] = 0
        # every other keyed pixel carries a flow of half a pixel (it still lands on itself), so the colour of a filled pixel
        # tells which key it took
        fwd[0, ::step, 0] = ((np.arange(0, W, step) // step) % 2 * 0.5).astype(F)
        fwd[1, (step // 2)::step, 0] = ((np.arange(step // 2, W, step) // step) % 2 * -0.5).astype(F)
        out, src = R.interp_ref(A, B, fwd, t)
        has = ~np.isnan(fwd[..., 0])
        xs = np.arange(W)
        for y in range(H):
            keyed = xs[has[y]]
            d = np.abs(xs[:, None] - keyed[None]).min(axis=1)
            assert np.array_equal(src[0, y] == 255, d > R.FILL) and np.array_equal(src[0, y] >= 4, d > 0)
        if step == 2:
            key, _ = R.fill(R.splat_keys(A, B, fwd, t)[0])
            assert np.array_equal(key[0, 1:W - 1:2], key[0, 0:W - 2:2])                  # the left one
        same(opt.interp_frames(gpu_state, A, B, fwd, t, want_src=True), (out, src))


GY = F(-2.2002129554748535)          # with f = (0.25, 3), g = (-0.25, GY): d2 == fmaf(0.01f, m2, 0.5f) exactly (asserted below)


def on_the_bound(k):
    """(f, g, side of the bound) with g.y k ulps from GY: on the bound, within it (k = 1), beyond it (k = -1)"""
    f, g = F([0.25, 3.0]), np.array([-0.25, tr.ulp(GY, k)], F)
    sy = f[1] + g[1]
    d2 = F(0) * F(0) + sy * sy
    m2 = (f[0] * f[0] + f[1] * f[1]) + (g[0] * g[0] + g[1] * g[1])
    bound = tr.fma(F(0.01), m2, F(0.5))
    assert (d2 == bound, d2 < bound, d2 > bound)[k], (k, d2, bound)
    return f, g


@pytest.mark.parametrize("k,holds", [(0, True), (1, True), (-1, False)], ids=["on", "within", "beyond"])
def test_both_forward_backward_tests_at_their_threshold(gpu_state, k, holds):
    f, g = on_the_bound(k)
    W, H, t = 9, 14, (0.5,)
    const = lambda v: np.broadcast_to(np.array(v, F), (H, W, 2)).copy()
    # the test of B: flat frames, so every key is side A's and stands for f; bwd is g everywhere
    out, src = R.interp_ref(flat(W, H), flat(W, H), const(f), t, const(g))
    inner = src[0, 4:9, 1:8]
    assert (inner == (0 if holds else 1)).all()
    same(opt.interp_frames(gpu_state, flat(W, H), flat(W, H), const(f), t, bwd=const(g), want_src=True), (out, src))
    # the test of A: one side-B key, u = -g, cheaper than side A's key on its target (4, 7); fwd is f everywhere
    rng = np.random.default_rng(9)
    A, B = (rng.integers(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(2))
    B[8, 4] = A[6, 4]                                           # the cost of B's (4, 8), which lands nearest (4, 6), is 0
    bwd = np.full((H, W, 2), np.nan, F)
    bwd[8, 4] = g
    key = int(R.splat_keys(A, B, const(f), t, bwd)[0, 7, 4])
    assert key == (1 << 31) | (8 * W + 4)
    out, src = R.interp_ref(A, B, const(f), t, bwd)
    assert src[0, 7, 4] == (1 if holds else 3)                  # (bwd around b1 is NaN: the test of B fails either way)
    same(opt.interp_frames(gpu_state, A, B, const(f), t, bwd=bwd, want_src=True), (out, src))


def test_anchors_on_the_device(gpu_state):
    rng = np.random.default_rng(6)
    H, W = 16, 31
    a, b = (rng.integers(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(2))
    z = np.zeros((H, W, 2), F)
    for bwd in (None, z):                                       # zero flows between equal frames: the frame, at every time
        out, src = opt.interp_frames(gpu_state, a, a, z, ALL_TIMES, bwd=bwd, want_src=True)
        assert (out == a[None]).all() and not src.any()
    bad = np.full((H, W, 2), 1e9, F)                            # no valid flow at t = .5: the blend baseline's frame
    bad[::2, :, 0], bad[1::2, :, 1] = np.nan, -np.inf
    out, src = opt.interp_frames(gpu_state, a, b, bad, [0.5], bwd=bad, want_src=True)
    assert np.array_equal(out[0], ((a.astype(np.uint16) + b + 1) >> 1).astype(np.uint8)) and (src == 255).all()
    ys, xs = np.mgrid[0:H, 0:W]
    for d in ((3, 0), (-2, 1), (5, 2)):                         # an even translation at t = .5: half of it
        b2 = np.roll(a, (2 * d[1], 2 * d[0]), (0, 1))
        fwd = np.broadcast_to(np.array([2 * d[0], 2 * d[1]], F), (H, W, 2))
        out, src = opt.interp_frames(gpu_state, a, b2, fwd, [0.5], want_src=True)
        ok = (xs - d[0] >= 0) & (xs - d[0] < W) & (xs + d[0] >= 0) & (xs + d[0] < W) & \
             (ys - d[1] >= 0) & (ys - d[1] < H) & (ys + d[1] >= 0) & (ys + d[1] < H)
        assert np.array_equal(out[0][ok], a[ys[ok] - d[1], xs[ok] - d[0]]) and (src[0][ok] == 0).all()


def test_unaligned_sub_buffers_src_null_and_refusals(gpu_state):
    """every buffer an odd number of bytes (the flows: of floats) into a larger allocation, whose other bytes stay as they
    were; then the argument sets the call refuses, nothing written"""
    W, H, K = 70, 9, 3
    N = W * H
    A, B, fwd, bwd = case(W, H)
    times = np.array([0.25, 0.5, 0.75], F)
    ref = R.interp_ref(A, B, fwd, times, bwd)
    lib = gpu_state.lib
    up = lambda a, off, dt: torch.cat([torch.zeros(off, dtype=dt), torch.from_numpy(np.ascontiguousarray(a).reshape(-1))]).cuda()
    dA, dB = up(A, 1, torch.uint8), up(B, 3, torch.uint8)
    dF, dG = up(fwd, 1, torch.float32), up(bwd, 3, torch.float32)
    pad = 5
    out = torch.full((pad + K * N * 3 + pad,), 7, dtype=torch.uint8, device="cuda")
    src = torch.full((pad + K * N + pad,), 9, dtype=torch.uint8, device="cuda")
    need = int(lib.ArapFlow_InterpScratchBytes(W, H, K))
    assert need == (K * N * 8 + 255) // 256 * 256
    scratch = torch.zeros(need + 8, dtype=torch.uint8, device="cuda")
    tp = times.ctypes.data_as(C.POINTER(C.c_float))
    p = lambda v: None if v is None else C.c_void_p(int(v))
    good = dict(W=W, H=H, A=dA.data_ptr() + 1, B=dB.data_ptr() + 3, fwd=dF.data_ptr() + 4, bwd=dG.data_ptr() + 12, K=K, times=tp,
                out=out.data_ptr() + pad, src=src.data_ptr() + pad, scratch=scratch.data_ptr() + 8)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.ArapFlow_InterpFrames(gpu_state.handle, a["W"], a["H"], p(a["A"]), p(a["B"]), p(a["fwd"]), p(a["bwd"]), a["K"],
                                       a["times"], p(a["out"]), p(a["src"]), p(a["scratch"]))
        torch.cuda.synchronize()
        return rc
    untouched = lambda: bool((out == 7).all()) and bool((src == 9).all()) and not bool(scratch.any())
    tm = lambda *v: (C.c_float * len(v))(*v)
    for bad in (dict(A=None), dict(B=None), dict(fwd=None), dict(times=None), dict(out=None), dict(scratch=None), dict(K=0), dict(K=33),
                dict(W=0), dict(H=0), dict(W=1 << 16, H=1 << 15), dict(W=1 << 15, H=1 << 15, K=2),
                dict(times=tm(0.25, 0.0, 0.5)), dict(times=tm(0.25, 0.5, 1.0)), dict(times=tm(float("nan"), 0.5, 0.75)),
                dict(times=tm(0.25, float("inf"), 0.75)), dict(times=tm(0.25, 0.5, -0.75)),
                dict(out=good["A"] + 8), dict(out=good["fwd"] + N * 8 - 1), dict(src=good["bwd"]), dict(src=good["out"] + K * N * 3 - 1),
                dict(scratch=good["out"] + 64), dict(scratch=good["B"] - need + 1), dict(out=good["scratch"] + need - 5), dict(src=good["scratch"] + 100)):
        assert call(**bad) == -1 and untouched(), bad
    assert call() == 0
    o, s = out.cpu().numpy(), src.cpu().numpy()
    assert (o[:pad] == 7).all() and (o[-pad:] == 7).all() and (s[:pad] == 9).all() and (s[-pad:] == 9).all()
    same((o[pad:-pad].reshape(K, H, W, 3), s[pad:-pad].reshape(K, H, W)), ref)
    out.fill_(7)
    assert call(src=None, bwd=None) == 0                        # both optional buffers NULL
    assert np.array_equal(out.cpu().numpy()[pad:-pad].reshape(K, H, W, 3), R.interp_ref(A, B, fwd, times)[0]) and bool((src[pad:-pad] != 9).any())
    for kw in (dict(times=[0.5, 1.0]), dict(times=[]), dict(times=[0.5] * 33)):
        with pytest.raises(ValueError):
            opt.interp_frames(gpu_state, A, B, fwd, **kw)
    with pytest.raises(ValueError):
        opt.interp_frames(gpu_state, A, B, fwd[:-1], [0.5])
    with pytest.raises(ValueError):
        opt.interp_frames(gpu_state, A, B[:, :-1], fwd, [0.5])
    with pytest.raises(ValueError):
        opt.interp_frames(gpu_state, A, B, fwd, [0.5], bwd=bwd[1:])
