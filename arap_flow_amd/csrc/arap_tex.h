// arap_tex.h -- procedural textures on the objects of a frame: the random-texture twin of a pair (gfx950).
//
// Definitions: DESIGN.md "Random textures"; the numpy twin is tests/tex_ref.py.  One kernel of the warp and background
// family (dim3(64, 4) blocks over (ceil(W/64), ceil(H/4)), one thread per pixel, no atomics, no scratch, no LDS): a pixel
// finds its layer -- the highest index whose mask is 0 there, the stacking order of the layered warp -- and gets that
// layer's texture colour, a pure function of (x, y), the layer's seed and its few parameters; a pixel of no layer keeps
// the input's bytes.  The library is built with -ffp-contract=off: every operator below is one IEEE f32 operation, and an
// fmaf is written only where the definition has one.  No transcendental, no sqrt, no division.
//
// The layer table lies in device memory (52 bytes a layer, the state's buffer): the layer index differs per lane, so a
// table passed by value would be indexed through scratch.  A wave's 64 neighbours of one row mostly share a layer, so
// its table reads hit one or two cache lines.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "arap_bg.h"

namespace arap {

// ArapFlow_TexLayer of include/arap_opt.h, field for field (static_assert in abi_warp.h)
struct TexLayer {
    uint32_t kind, seed;
    BgMap m;                               // pixel -> texture point, bg_apply's expression
    float p0, p1;
    uint8_t c0[3], c1[3], c2[3], reserved[3];
};

enum : uint32_t { TEX_CHECKER = 0, TEX_BRICK = 1, TEX_VORONOI = 2, TEX_NOISE = 3, TEX_WAVE = 4, TEX_KINDS = 5 };

__device__ __forceinline__ uint32_t tex_mix(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// h(i, j, k) of lattice point (i, j), stream k
__device__ __forceinline__ uint32_t tex_hash(uint32_t seed, int i, int j, uint32_t k)
{
    return tex_mix(tex_mix(tex_mix(seed + k) ^ (uint32_t)i) ^ (uint32_t)j);
}

// r01: the top 24 bits as a float in [0, 1), exact
__device__ __forceinline__ float tex_r01(uint32_t h) { return (float)(h >> 8) * 5.9604644775390625e-08f; }

// a coordinate, clamped to [-2^20, 2^20] (NaN -> 0): the conversion to int below is defined
__device__ __forceinline__ float tex_clamp(float a) { return a == a ? fminf(fmaxf(a, -1048576.0f), 1048576.0f) : 0.0f; }

// the lattice cell of a coordinate (clamped here) and its fraction a - floor(a), in [0, 1] (1 for a tiny negative a)
__device__ __forceinline__ int tex_cell(float a, float& frac)
{
    a = tex_clamp(a);
    const float f = floorf(a);
    frac = a - f;
    return (int)f;
}

// mix(ca, cb, t), t clamped to [0, 1], round half up
__device__ __forceinline__ void tex_blend(const uint8_t ca[3], const uint8_t cb[3], float t, uint8_t out[3])
{
    t = fminf(fmaxf(t, 0.0f), 1.0f);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float a = (float)ca[c], b = (float)cb[c];
        out[c] = (uint8_t)(fmaf(t, b - a, a) + 0.5f);
    }
}

__device__ __forceinline__ void tex_copy(const uint8_t c[3], uint8_t out[3]) { out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; }

// vn(u, v, k): value noise on the integer lattice, in [0, 1]
__device__ __forceinline__ float tex_vnoise(uint32_t seed, float u, float v, uint32_t k)
{
    float tx, ty;
    const int i = tex_cell(u, tx), j = tex_cell(v, ty);
    const float sx = (tx * tx) * (3.0f - 2.0f * tx), sy = (ty * ty) * (3.0f - 2.0f * ty);
    const float a00 = tex_r01(tex_hash(seed, i, j, k)), a10 = tex_r01(tex_hash(seed, i + 1, j, k));
    const float a01 = tex_r01(tex_hash(seed, i, j + 1, k)), a11 = tex_r01(tex_hash(seed, i + 1, j + 1, k));
    const float top = fmaf(sx, a10 - a00, a00), bot = fmaf(sx, a11 - a01, a01);
    return fmaf(sy, bot - top, top);
}

// the colour of layer L at pixel (x, y)
__device__ __forceinline__ void tex_colour(const TexLayer& L, int x, int y, uint8_t out[3])
{
    const float2 p = bg_apply(L.m, x, y);
    const uint32_t seed = L.seed;
    float fu, fv;
    const float u = tex_clamp(p.x), v = tex_clamp(p.y);
    const int i = tex_cell(u, fu), j = tex_cell(v, fv);
    switch (L.kind) {
    case TEX_CHECKER:
        tex_copy(((i + j) & 1) ? L.c1 : L.c0, out);
        return;
    case TEX_BRICK: {
        float fs;
        const int col = tex_cell((j & 1) ? u + L.p1 : u, fs);
        if (fs < L.p0 || fv < L.p0) tex_copy(L.c2, out);
        else tex_copy((tex_hash(seed, col, j, 0) & 1) ? L.c1 : L.c0, out);
        return;
    }
    case TEX_VORONOI: {
        float best = 0.0f;
        int wi = 0, wj = 0;
        for (int dj = -1; dj <= 1; ++dj)
            for (int di = -1; di <= 1; ++di) {
                const int ci = i + di, cj = j + dj;
                const float dx = ((float)di + tex_r01(tex_hash(seed, ci, cj, 0))) - fu;
                const float dy = ((float)dj + tex_r01(tex_hash(seed, ci, cj, 1))) - fv;
                const float d = dx * dx + dy * dy;
                if ((dj == -1 && di == -1) || d < best) { best = d; wi = ci; wj = cj; }
            }
        tex_blend(L.c0, L.c1, tex_r01(tex_hash(seed, wi, wj, 2)), out);
        return;
    }
    case TEX_NOISE: {
        float sum = 0.0f, scale = 1.0f, weight = 0.5f;
#pragma unroll
        for (uint32_t o = 0; o < 4; ++o) {
            sum = sum + weight * tex_vnoise(seed, u * scale, v * scale, o);
            scale = scale * 2.0f;
            weight = weight * 0.5f;
        }
        if (sum < 0.5f) tex_blend(L.c0, L.c1, 2.0f * sum, out);
        else tex_blend(L.c1, L.c2, 2.0f * (sum - 0.5f), out);
        return;
    }
    default: {                                                           // TEX_WAVE (the entry point refuses other kinds)
        const float n = tex_vnoise(seed, u, v, 0);
        float t;
        (void)tex_cell(u + L.p0 * (2.0f * n - 1.0f), t);
        if (L.p1 >= 0.5f) t = 1.0f - fabsf(2.0f * t - 1.0f);
        tex_blend(L.c0, L.c1, t, out);
        return;
    }
    }
}

// grid = (ceil(W/64), ceil(H/4)), block = (64,4).  masks: [n][H][W], 0 = object, or NULL: every pixel is layer 0's
__global__ __launch_bounds__(256) void k_tex_fill(const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ masks,
                                                  const TexLayer* __restrict__ layers, int n, uint8_t* __restrict__ out_rgb,
                                                  int W, int H)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t N = (size_t)W * H, i = (size_t)y * W + x;
    int owner = masks ? -1 : 0;
    if (masks)
        for (int l = n - 1; l >= 0; --l)
            if (masks[(size_t)l * N + i] == 0) { owner = l; break; }
    uint8_t v[3];
    if (owner < 0) { v[0] = rgb[3 * i]; v[1] = rgb[3 * i + 1]; v[2] = rgb[3 * i + 2]; }
    else tex_colour(layers[owner], x, y, v);
    out_rgb[3 * i] = v[0]; out_rgb[3 * i + 1] = v[1]; out_rgb[3 * i + 2] = v[2];
}

}  // namespace arap
