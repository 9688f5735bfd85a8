"""Vectorised numpy twin of DESIGN.md "Random textures" (arap_flow_amd/csrc/arap_tex.h), written from that text: uint32
and float32 arithmetic only, the same operations in the same order.  An fmaf is the float64 product (exact: two float32
factors) plus the float64 addend, rounded to float32; where that float64 sum lands exactly between two float32 values --
the only place a second rounding could differ from the single one -- the element is redone in exact rational arithmetic.

A layer description is the tuple (kind, seed, m[6], p0, p1, c0, c1, c2) of pipeline.TexLayer, the kind a number or a name
of KINDS."""
from fractions import Fraction

import numpy as np

F = np.float32
U = np.uint32
KINDS = ("checker", "brick", "voronoi", "noise", "wave")
CHECKER, BRICK, VORONOI, NOISE, WAVE = range(5)
LIM = F(1048576.0)                     # 2^20


def fma(a, b, c):
    a, b, c = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F), np.asarray(c, F))
    s = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
    out = s.astype(F)
    tie = (s.view(np.uint64) & np.uint64(0x1fffffff)) == np.uint64(0x10000000)
    if tie.any():                      # exactly rounded, one element at a time
        out = out.copy()
        for idx in zip(*np.nonzero(tie)):
            exact = Fraction(float(a[idx])) * Fraction(float(b[idx])) + Fraction(float(c[idx]))
            lo, hi = sorted((float(np.nextafter(out[idx], F(-np.inf))), float(np.nextafter(out[idx], F(np.inf)))))
            cands = [F(lo), out[idx], F(hi)]
            # nearest, ties to the even mantissa
            out[idx] = min(cands, key=lambda q: (abs(Fraction(float(q)) - exact), int(np.asarray(q, F).view(U)) & 1))
    return out


def mix(x):
    x = np.asarray(x, U)
    with np.errstate(over="ignore"):           # (numpy warns when a 0-d product wraps; wrapping is the definition)
        x = x ^ (x >> U(16))
        x = x * U(0x7feb352d)
        x = x ^ (x >> U(15))
        x = x * U(0x846ca68b)
        return x ^ (x >> U(16))


def hash3(seed, i, j, k):
    """h(i, j, k) for int32 lattice coordinates (arrays) and the stream k"""
    s = mix(np.asarray((int(seed) + int(k)) & 0xffffffff, U))
    return mix(mix(s ^ np.asarray(i, np.int32).view(U)) ^ np.asarray(j, np.int32).view(U))


def r01(h):
    return (h >> U(8)).astype(F) * F(2.0 ** -24)


def clamp(a):
    a = np.asarray(a, F)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(a), F(0), np.minimum(np.maximum(a, -LIM), LIM)).astype(F)


def cell(a):
    """(lattice cell int32, fraction float32) of a coordinate, clamped here"""
    a = clamp(a)
    f = np.floor(a)
    return f.astype(np.int32), (a - f).astype(F)


def blend(ca, cb, t):
    """mix(ca, cb, t) per channel -> u8 [..., 3]"""
    t = np.minimum(np.maximum(np.asarray(t, F), F(0)), F(1))[..., None]
    a, b = np.asarray(ca, np.uint8).astype(F), np.asarray(cb, np.uint8).astype(F)
    return (fma(t, b - a, a) + F(0.5)).astype(np.uint8)


def flat(pick, c_false, c_true):
    return np.where(np.asarray(pick, bool)[..., None], np.asarray(c_true, np.uint8), np.asarray(c_false, np.uint8))


def vnoise(seed, u, v, k):
    i, tx = cell(u)
    j, ty = cell(v)
    sx = (tx * tx) * (F(3) - F(2) * tx)
    sy = (ty * ty) * (F(3) - F(2) * ty)
    one = np.int32(1)
    a00, a10 = r01(hash3(seed, i, j, k)), r01(hash3(seed, i + one, j, k))
    a01, a11 = r01(hash3(seed, i, j + one, k)), r01(hash3(seed, i + one, j + one, k))
    top, bot = fma(sx, a10 - a00, a00), fma(sx, a11 - a01, a01)
    return fma(sy, bot - top, top)


def texture_points(layer, W, H):
    """(u, v) float32 [H, W]: the layer's clamped texture point at every pixel"""
    m = np.asarray(layer[2], F)
    ys, xs = np.mgrid[0:H, 0:W]
    xs, ys = xs.astype(F), ys.astype(F)
    return clamp(fma(m[0], xs, fma(m[1], ys, m[2]))), clamp(fma(m[3], xs, fma(m[4], ys, m[5])))


def colour(layer, W, H):
    """the layer's texture at every pixel of a W x H frame -> u8 [H, W, 3]"""
    kind, seed, _, p0, p1, c0, c1, c2 = layer
    kind = KINDS.index(kind) if isinstance(kind, str) else int(kind)
    p0, p1 = F(p0), F(p1)
    u, v = texture_points(layer, W, H)
    (i, fu), (j, fv) = cell(u), cell(v)
    if kind == CHECKER:
        return flat((i + j) & 1, c0, c1)
    if kind == BRICK:
        col, fs = cell(np.where((j & 1) != 0, u + p1, u))
        brick = flat(hash3(seed, col, j, 0) & U(1), c0, c1)
        return np.where(((fs < p0) | (fv < p0))[..., None], np.asarray(c2, np.uint8), brick)
    if kind == VORONOI:
        best = wi = wj = None
        for dj in (-1, 0, 1):
            for di in (-1, 0, 1):
                ci, cj = i + np.int32(di), j + np.int32(dj)
                dx = (F(di) + r01(hash3(seed, ci, cj, 0))) - fu
                dy = (F(dj) + r01(hash3(seed, ci, cj, 1))) - fv
                d = dx * dx + dy * dy
                if best is None:
                    best, wi, wj = d, ci, cj
                else:
                    closer = d < best
                    best, wi, wj = np.where(closer, d, best), np.where(closer, ci, wi), np.where(closer, cj, wj)
        return blend(c0, c1, r01(hash3(seed, wi, wj, 2)))
    if kind == NOISE:
        total, scale, weight = np.zeros_like(u), F(1), F(0.5)
        for o in range(4):
            total = total + weight * vnoise(seed, u * scale, v * scale, o)
            scale, weight = scale * F(2), weight * F(0.5)
        low = blend(c0, c1, F(2) * total)
        high = blend(c1, c2, F(2) * (total - F(0.5)))
        return np.where((total < F(0.5))[..., None], low, high)
    if kind == WAVE:
        n = vnoise(seed, u, v, 0)
        _, t = cell(u + p0 * (F(2) * n - F(1)))
        if p1 >= F(0.5):
            t = F(1) - np.abs(F(2) * t - F(1))
        return blend(c0, c1, t)
    raise ValueError("unknown kind %r" % (kind,))


def owner(masks):
    """per pixel the highest layer whose mask is 0 there, -1 where none: the stacking order of the layered warp"""
    obj = np.asarray(masks) == 0
    n = obj.shape[0]
    top = (n - 1) - np.argmax(obj[::-1], axis=0)
    return np.where(obj.any(0), top, -1)


def texture(rgb, masks, layers):
    """ArapFlow_Texture: rgb u8[H,W,3], masks u8[n,H,W] or None (every pixel is layer 0's), layers -> u8[H,W,3]"""
    rgb = np.asarray(rgb, np.uint8)
    H, W = rgb.shape[:2]
    own = np.zeros((H, W), np.int64) if masks is None else owner(masks)
    out = rgb.copy()
    for l, layer in enumerate(layers):
        sel = own == l
        if sel.any():
            out[sel] = colour(layer, W, H)[sel]
    return out
