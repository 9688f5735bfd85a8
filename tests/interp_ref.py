"""The numpy twin of ArapFlow_InterpFrames (DESIGN.md "Frames from flows"): float32 arithmetic operator by operator for
the positions and the two forward-backward tests (tscore_ref.fma, tscore_ref.sample), integers for everything stored.
Written for clarity: the splat is a minimum over 64-bit keys, the hole fill a search by growing distance.  Test helper; no
GPU."""
import numpy as np

import tscore_ref as tr

F = np.float32
MAX_TIMES, FILL = 32, 16
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def valid(u):
    """both components finite and below 1e9 in magnitude"""
    with np.errstate(invalid="ignore"):
        return (np.abs(u[..., 0]) < F(1e9)) & (np.abs(u[..., 1]) < F(1e9))


def nearest(v, hi):
    with np.errstate(invalid="ignore"):
        return np.minimum(np.floor(v + F(0.5)).astype(np.int64), hi)


def grid(W, H):
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return ii.reshape(-1), jj.reshape(-1)


def side_terms(I, J, flow):
    """(ok, cost) of every source pixel of one side: I the side's own frame, J the other one"""
    H, W = I.shape[:2]
    ii, jj = grid(W, H)
    u = np.asarray(flow, F).reshape(-1, 2)
    ok = valid(u)
    with np.errstate(all="ignore"):
        e = np.stack([ii.astype(F) + u[:, 0], jj.astype(F) + u[:, 1]], -1)
    assert e.dtype == F
    inside = ok & tr.in_frame(e, W, H)
    cost = np.full(W * H, 766, np.uint64)
    qx, qy = nearest(e[inside, 0], W - 1), nearest(e[inside, 1], H - 1)
    diff = np.abs(I.reshape(-1, 3)[inside].astype(np.int64) - J[qy, qx].astype(np.int64)).sum(-1)
    cost[inside] = diff.astype(np.uint64)
    return ok, cost


def splat(key, flow, ok, cost, tt, side):
    """the minima of one side at one time into key u64[H*W]"""
    H, W = flow.shape[:2]
    ii, jj = grid(W, H)
    u = np.asarray(flow, F).reshape(-1, 2)
    with np.errstate(all="ignore"):
        p = np.stack([tr.fma(tt, u[:, 0], ii.astype(F)), tr.fma(tt, u[:, 1], jj.astype(F))], -1)
    put = np.nonzero(ok & tr.in_frame(p, W, H))[0]
    r = nearest(p[put, 1], H - 1) * W + nearest(p[put, 0], W - 1)
    kv = (cost[put] << np.uint64(32)) | np.uint64(side << 31) | put.astype(np.uint64)
    np.minimum.at(key, r, kv)


def fill(key):
    """key u64[H,W] -> (key with the holes of up to FILL pixels filled along the rows, bool[H,W] of the filled ones)"""
    H, W = key.shape
    has = key != NONE
    out, filled = key.copy(), np.zeros((H, W), bool)
    xs = np.arange(W)
    for d in range(1, FILL + 1):
        for sign in (-1, 1):                                   # the left one first
            x = xs + sign * d
            inside = (x >= 0) & (x < W)
            xc = np.clip(x, 0, W - 1)
            take = ~has & ~filled & inside[None] & has[:, xc]
            out[take] = key[:, xc][take]
            filled |= take
    return out, filled


def colour(I, a):
    """C(I, a) at the points a f32[P,2] inside the frame of I u8[H,W,3] -> int64[P,3]"""
    H, W = I.shape[:2]
    x0f, y0f = np.floor(a[:, 0]), np.floor(a[:, 1])
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    wx = ((a[:, 0] - x0f) * F(256) + F(0.5)).astype(np.int64)[:, None]
    wy = ((a[:, 1] - y0f) * F(256) + F(0.5)).astype(np.int64)[:, None]
    assert (a[:, 0] - x0f).dtype == F
    P = I.astype(np.int64)
    return ((256 - wx) * (256 - wy) * P[y0, x0] + wx * (256 - wy) * P[y0, x1] + (256 - wx) * wy * P[y1, x0] + wx * wy * P[y1, x1])


def agree(d, first, second):
    """the forward-backward test, false on NaN"""
    with np.errstate(all="ignore"):
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
        m2 = (first[:, 0] * first[:, 0] + first[:, 1] * first[:, 1]) + (second[:, 0] * second[:, 0] + second[:, 1] * second[:, 1])
        assert d2.dtype == m2.dtype == F
        return d2 <= tr.fma(F(0.01), m2, F(0.5))


def splat_keys(A, B, fwd, times, bwd=None):
    """step 1 alone: the key images u64[K,H,W] before the hole fill"""
    A, B, fwd = np.asarray(A, np.uint8), np.asarray(B, np.uint8), np.asarray(fwd, F)
    bwd = None if bwd is None else np.asarray(bwd, F)
    times = np.asarray(times, F).reshape(-1)
    H, W = A.shape[:2]
    okA, costA = side_terms(A, B, fwd)
    if bwd is not None:
        okB, costB = side_terms(B, A, bwd)
    keys = np.full((times.size, H * W), NONE, np.uint64)
    for k, t in enumerate(times):
        splat(keys[k], fwd, okA, costA, t, 0)
        if bwd is not None:
            splat(keys[k], bwd, okB, costB, F(1.0) - t, 1)
    return keys.reshape(times.size, H, W)


def interp_ref(A, B, fwd, times, bwd=None):
    """opt.interp_frames' twin: A, B u8[H,W,3]; fwd f32[H,W,2]; bwd the same or None; times K floats in (0, 1) ->
    (out u8[K,H,W,3], src u8[K,H,W])"""
    A, B = np.asarray(A, np.uint8), np.asarray(B, np.uint8)
    fwd = np.asarray(fwd, F)
    bwd = None if bwd is None else np.asarray(bwd, F)
    times = np.asarray(times, F).reshape(-1)
    H, W = A.shape[:2]
    N, K = W * H, times.size
    assert 1 <= K <= MAX_TIMES and np.all(np.isfinite(times) & (times > 0) & (times < 1))
    ii, jj = grid(W, H)
    keys = splat_keys(A, B, fwd, times, bwd)
    out, src = np.zeros((K, H, W, 3), np.uint8), np.zeros((K, H, W), np.uint8)
    Af, Bf = A.reshape(N, 3).astype(np.int64), B.reshape(N, 3).astype(np.int64)
    for k, t in enumerate(times):
        s = F(1.0) - t
        tq = int(t * F(256) + F(0.5))
        key, filled = fill(keys[k])
        key, filled = key.reshape(N), filled.reshape(N)

        col = (((256 - tq) * Af + tq * Bf + 128) >> 8)               # the hole formula, everywhere
        sk = np.full(N, 255, np.int64)
        at = np.nonzero(key != NONE)[0]
        from_ = (key[at] & np.uint64(0x7FFFFFFF)).astype(np.int64)
        sideB = ((key[at] >> np.uint64(31)) & np.uint64(1)).astype(bool)
        u = fwd.reshape(N, 2)[from_].copy()
        if bwd is not None:
            u[sideB] = -bwd.reshape(N, 2)[from_[sideB]]
        x, y = ii[at].astype(F), jj[at].astype(F)
        with np.errstate(all="ignore"):
            a0 = np.stack([tr.fma(-t, u[:, 0], x), tr.fma(-t, u[:, 1], y)], -1)
            b1 = np.stack([tr.fma(s, u[:, 0], x), tr.fma(s, u[:, 1], y)], -1)
        okA, okB = tr.in_frame(a0, W, H), tr.in_frame(b1, W, H)
        with np.errstate(all="ignore"):
            m = np.nonzero(okA)[0]
            f0 = tr.sample(fwd, a0[m])
            okA[m] = agree(f0 - u[m], f0, u[m])
            if bwd is not None:
                m = np.nonzero(okB)[0]
                g1 = tr.sample(bwd, b1[m])
                okB[m] = agree(u[m] + g1, u[m], g1)
        sk[at] = np.where(okA, np.where(okB, 0, 1), np.where(okB, 2, 3)) + 4 * filled[at]
        both, onlyA, onlyB = okA & okB, okA & ~okB, okB & ~okA
        ca, cb = colour(A, a0[okA]), colour(B, b1[okB])
        CA, CB = np.zeros((at.size, 3), np.int64), np.zeros((at.size, 3), np.int64)
        CA[okA], CB[okB] = ca, cb
        col[at[both]] = ((256 - tq) * CA[both] + tq * CB[both] + (1 << 23)) >> 24
        col[at[onlyA]] = (CA[onlyA] + 32768) >> 16
        col[at[onlyB]] = (CB[onlyB] + 32768) >> 16
        assert col.min() >= 0 and col.max() <= 255
        out[k], src[k] = col.reshape(H, W, 3), sk.reshape(H, W)
    return out, src
