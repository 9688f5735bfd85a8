"""Numpy twin of DESIGN.md "Relit frames" (arap_flow_amd/csrc/arap_light.h, ArapFlow_LightTables), written from that text:
integer and float32 arithmetic only, every float32 operator one operation in the order of the definition's parentheses.
The hash, r01, the value noise and the fused multiply-add of the field point are tex_ref's.  relight() is vectorised and
takes the shadow's window counts from an integral image; relight_brute() is the same statement pixel by pixel, with
explicit loops over the window and scalar arithmetic, and shares with it only tex_ref's value noise.

A frame description is the tuple (seed, m[6], amp, vig, gain[3], gamma, sh_dx, sh_dy, sh_r, sh_g, sigma0, sigma1) of
pipeline.LightFrame; its floats are rounded to float32 here, as opt.light_frame rounds them."""
import math

import numpy as np

import tex_ref

F = np.float32
SQRT3 = F(1.7320508)


def tables(frame, W, H):
    """ArapFlow_LightTables: (lut u8[3,256], geom f32[3])"""
    gain, gamma = [float(F(g)) for g in frame[4]], float(F(frame[5]))
    lut = np.zeros((3, 256), np.uint8)
    for c in range(3):
        for i in range(256):
            lut[c, i] = int(math.floor(255.0 * min(max(gain[c] * math.pow(i / 255.0, gamma), 0.0), 1.0) + 0.5))
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    r2 = cx * cx + cy * cy
    return lut, np.array([cx, cy, 1.0 / r2 if r2 > 0 else 0.0], np.float64).astype(F)


def objects(cover, cover_is_mask):
    cover = np.asarray(cover)
    return cover == 0 if cover_is_mask else cover != 0


def window_counts(obj, dx, dy, r):
    """a[y, x] = #{(i, j): |i| <= r, |j| <= r, obj(x - dx + i, y - dy + j)}, obj false outside the frame: from the
    integral image of obj"""
    H, W = obj.shape
    S = np.zeros((H + 1, W + 1), np.int64)
    S[1:, 1:] = np.cumsum(np.cumsum(obj.astype(np.int64), 0), 1)
    ys, xs = np.mgrid[0:H, 0:W]
    x0, x1 = np.clip(xs - dx - r, 0, W), np.clip(xs - dx + r + 1, 0, W)
    y0, y1 = np.clip(ys - dy - r, 0, H), np.clip(ys - dy + r + 1, 0, H)
    return S[y1, x1] - S[y0, x1] - S[y1, x0] + S[y0, x0]


def relight(rgb, cover, frame, cover_is_mask=False):
    """ArapFlow_Relight: rgb u8[H,W,3], cover u8[H,W] or None (sh_g = 0 only) -> u8[H,W,3]"""
    seed, m, amp, vig, _, _, dx, dy, r, g, s0, s1 = frame
    rgb = np.asarray(rgb, np.uint8)
    H, W = rgb.shape[:2]
    lut, (cx, cy, inv_r2) = tables(frame, W, H)
    v = rgb.astype(np.int64)
    if g > 0:
        obj = objects(cover, cover_is_mask)
        A = (2 * r + 1) ** 2
        a = window_counts(obj, dx, dy, r)
        shaded = (v * (256 * A - g * a)[..., None] + 128 * A) // (256 * A)
        v = np.where(obj[..., None], v, shaded)
    u, w = tex_ref.texture_points((None, None, m), W, H)
    vn = tex_ref.vnoise(seed, u, w, 0)
    amp, vig, s0, s1 = F(amp), F(vig), F(s0), F(s1)
    L = F(1) + amp * (F(2) * vn - F(1))
    ys, xs = np.mgrid[0:H, 0:W]
    fx, fy = xs.astype(F), ys.astype(F)
    V = F(1) - vig * np.minimum(((fx - cx) * (fx - cx) + (fy - cy) * (fy - cy)) * inv_r2, F(1))
    shade = L * V
    out = np.empty_like(rgb)
    xi, yi = xs.astype(np.int32), ys.astype(np.int32)
    for c in range(3):
        v3 = lut[c][v[..., c]].astype(F) * shade
        r0, r1, r2, r3 = (tex_ref.r01(tex_ref.hash3(seed, xi, yi, 1 + 4 * c + j)) for j in range(4))
        n = (((r0 + r1) + (r2 + r3)) - F(2)) * SQRT3
        v4 = v3 + (s0 + s1 * v3) * n
        out[..., c] = (np.fmin(np.fmax(v4, F(0)), F(255)) + F(0.5)).astype(np.uint8)
    return out


def _mix(x):
    x ^= x >> 16
    x = x * 0x7feb352d & 0xffffffff
    x ^= x >> 15
    x = x * 0x846ca68b & 0xffffffff
    return x ^ x >> 16


def _r01(seed, i, j, k):
    h = _mix(_mix(_mix((seed + k) & 0xffffffff) ^ (i & 0xffffffff)) ^ (j & 0xffffffff))
    return F(h >> 8) * F(2.0 ** -24)


def relight_brute(rgb, cover, frame, cover_is_mask=False):
    """the definition pixel by pixel: explicit loops over the shadow's window, scalar arithmetic"""
    seed, m, amp, vig, _, _, dx, dy, r, g, s0, s1 = frame
    rgb = np.asarray(rgb, np.uint8)
    H, W = rgb.shape[:2]
    lut, (cx, cy, inv_r2) = tables(frame, W, H)
    m = [F(q) for q in m]
    amp, vig, s0, s1 = F(amp), F(vig), F(s0), F(s1)

    def obj(px, py):
        if not (0 <= px < W and 0 <= py < H):
            return False
        return cover[py][px] == 0 if cover_is_mask else cover[py][px] != 0
    out = np.zeros_like(rgb)
    for y in range(H):
        for x in range(W):
            v = [int(q) for q in rgb[y, x]]
            if g > 0 and not obj(x, y):
                a = 0
                for j in range(-r, r + 1):
                    for i in range(-r, r + 1):
                        a += obj(x - dx + i, y - dy + j)
                A = (2 * r + 1) * (2 * r + 1)
                v = [(q * (256 * A - g * a) + 128 * A) // (256 * A) for q in v]
            fx, fy = F(x), F(y)
            one = lambda q: np.asarray([q], F)              # (tex_ref works on arrays)
            u = tex_ref.fma(one(m[0]), one(fx), tex_ref.fma(one(m[1]), one(fy), one(m[2])))
            w = tex_ref.fma(one(m[3]), one(fx), tex_ref.fma(one(m[4]), one(fy), one(m[5])))
            vn = tex_ref.vnoise(seed, u, w, 0)[0]
            L = F(1) + amp * (F(2) * vn - F(1))
            V = F(1) - vig * min(((fx - cx) * (fx - cx) + (fy - cy) * (fy - cy)) * inv_r2, F(1))
            shade = L * V
            for c in range(3):
                v3 = F(lut[c][v[c]]) * shade
                r0, r1, r2, r3 = (_r01(seed, x, y, 1 + 4 * c + j) for j in range(4))
                n = (((r0 + r1) + (r2 + r3)) - F(2)) * SQRT3
                v4 = v3 + (s0 + s1 * v3) * n
                out[y, x, c] = int(min(max(v4, F(0)), F(255)) + F(0.5))
    return out
