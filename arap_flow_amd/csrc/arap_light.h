// arap_light.h -- relit frames: one soft shadow of the objects on the background, a tone curve, a smooth illumination
// field, a vignette and sensor noise on a finished frame (gfx950).
//
// Definitions: DESIGN.md "Relit frames"; the numpy twin is tests/light_ref.py.  One kernel of the warp and background
// family (dim3(64, 4) blocks over (ceil(W/64), ceil(H/4)), one thread per pixel, no atomics, no scratch).  The library is
// built with -ffp-contract=off: every operator below is one IEEE f32 operation, in the order the parentheses give.  No
// transcendental, no sqrt, no float division: the tone curve is a 3 x 256 byte table made on the host.
//
// Everything but the shadow is pointwise.  The shadow needs, per background pixel, the number of object pixels in a
// (2r+1)^2 window displaced by (-sh_dx, -sh_dy).  A block stages the cover BITS of the union of its pixels' windows,
// (64 + 2r) x (4 + 2r) <= 96 x 36 bytes, in LDS once (every byte of the cover is read from memory once per block that
// needs it, zeros for pixels outside the frame), and forms the counts separably: the 4 + 2r rows of a column are summed
// first, sliding down the block's four rows (one thread per column: 2r + 1 reads, then two per further row), which
// leaves 4 x (64 + 2r) column sums <= 33 in bytes; then every thread adds the 2r + 1 column sums of its row.  The
// columns go first because the tile is four rows tall: that pass shrinks 36 rows to 4, the other order would shrink 96
// columns only to 64.  LDS: 96 * 36 + 96 * 4 = 3840 bytes a block, rows 96 bytes apart: a wave's 64 neighbours read
// 64 consecutive bytes, each group of 32 lanes eight or nine consecutive dwords (as many banks, the lanes of a dword
// served by a broadcast), no conflict.
//
// SHADOW is a template flag (sh_g = 0 is uniform per launch): without it no LDS is declared, nothing is staged and the
// kernel has no barrier.  With it every thread of the block, the ones outside the frame included, reaches both barriers:
// the only return lies behind them.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "arap_tex.h"

namespace arap {

constexpr int LIGHT_MAX_R = 16, LIGHT_MAX_SHIFT = 64;          // ARAPFLOW_LIGHT_MAX_R, ARAPFLOW_LIGHT_MAX_SHIFT
constexpr int LIGHT_TILE_W = 64 + 2 * LIGHT_MAX_R, LIGHT_TILE_H = 4 + 2 * LIGHT_MAX_R;

// what the kernel needs of an ArapFlow_LightFrame, by value (uniform: scalar loads)
struct LightParams {
    uint32_t seed;
    BgMap m;                               // pixel -> field point, bg_apply's expression
    float amp, vig;
    float cx, cy, inv_r2;                  // ArapFlow_LightTables' geom
    int sh_dx, sh_dy, sh_r, sh_g;
    float sigma0, sigma1;
};

// the number of object pixels in the window of pixel (threadIdx.x, threadIdx.y) of the block.  Every thread of the
// block calls it (two barriers).
template <bool COVER_IS_MASK>
__device__ __forceinline__ int light_window_count(const uint8_t* __restrict__ cover, const LightParams& q, int W, int H)
{
    __shared__ uint8_t bits[LIGHT_TILE_H * LIGHT_TILE_W];
    __shared__ uint8_t cols[4 * LIGHT_TILE_W];
    const int tx = threadIdx.x, ty = threadIdx.y, r = q.sh_r;
    const int tw = 64 + 2 * r, th = 4 + 2 * r;
    const int gx0 = (int)blockIdx.x * 64 - q.sh_dx - r, gy0 = (int)blockIdx.y * 4 - q.sh_dy - r;
    for (int row = ty; row < th; row += 4) {
        const int gy = gy0 + row;
        for (int col = tx; col < tw; col += 64) {
            const int gx = gx0 + col;
            bool obj = false;
            if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                const uint8_t c = cover[(size_t)gy * W + gx];
                obj = COVER_IS_MASK ? c == 0 : c != 0;
            }
            bits[row * LIGHT_TILE_W + col] = obj ? 1 : 0;
        }
    }
    __syncthreads();
    const int col = ty * 64 + tx;
    if (col < tw) {
        int sum = 0;
        for (int j = 0; j <= 2 * r; ++j) sum += bits[j * LIGHT_TILE_W + col];
        cols[col] = (uint8_t)sum;
#pragma unroll
        for (int oy = 1; oy < 4; ++oy) {
            sum += (int)bits[(2 * r + oy) * LIGHT_TILE_W + col] - (int)bits[(oy - 1) * LIGHT_TILE_W + col];
            cols[oy * LIGHT_TILE_W + col] = (uint8_t)sum;
        }
    }
    __syncthreads();
    int a = 0;
    for (int i = 0; i <= 2 * r; ++i) a += cols[ty * LIGHT_TILE_W + tx + i];
    return a;
}

// grid = (ceil(W/64), ceil(H/4)), block = (64,4).  lut: [3][256] device bytes.  cover: [H][W], read only with SHADOW
// (then for every pixel of the block's window) and may be NULL without it.
template <bool SHADOW, bool COVER_IS_MASK>
__global__ __launch_bounds__(256) void k_relight(const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ cover,
                                                 const uint8_t* __restrict__ lut, LightParams q,
                                                 uint8_t* __restrict__ out_rgb, int W, int H)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    int a = 0;
    if (SHADOW) a = light_window_count<COVER_IS_MASK>(cover, q, W, H);
    if (x >= W || y >= H) return;
    const size_t i = (size_t)y * W + x;
    uint32_t v[3] = {rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]};
    if (SHADOW) {
        const uint8_t c = cover[i];
        if (!(COVER_IS_MASK ? c == 0 : c != 0)) {
            const uint32_t side = 2u * (uint32_t)q.sh_r + 1u, A = side * side;
            const uint32_t keep = 256u * A - (uint32_t)q.sh_g * (uint32_t)a, half = 128u * A, den = 256u * A;
#pragma unroll
            for (int c3 = 0; c3 < 3; ++c3) v[c3] = (v[c3] * keep + half) / den;
        }
    }
    const float2 p = bg_apply(q.m, x, y);
    const float vn = tex_vnoise(q.seed, p.x, p.y, 0);
    const float L = 1.0f + q.amp * (2.0f * vn - 1.0f);
    const float fx = (float)x, fy = (float)y;
    const float V = 1.0f - q.vig * fminf(((fx - q.cx) * (fx - q.cx) + (fy - q.cy) * (fy - q.cy)) * q.inv_r2, 1.0f);
    const float shade = L * V;
#pragma unroll
    for (uint32_t c = 0; c < 3; ++c) {
        const float v3 = (float)lut[256 * c + v[c]] * shade;
        const float r0 = tex_r01(tex_hash(q.seed, x, y, 1 + 4 * c)), r1 = tex_r01(tex_hash(q.seed, x, y, 2 + 4 * c));
        const float r2 = tex_r01(tex_hash(q.seed, x, y, 3 + 4 * c)), r3 = tex_r01(tex_hash(q.seed, x, y, 4 + 4 * c));
        const float n = (((r0 + r1) + (r2 + r3)) - 2.0f) * 1.7320508f;
        const float v4 = v3 + (q.sigma0 + q.sigma1 * v3) * n;
        out_rgb[3 * i + c] = (uint8_t)(fminf(fmaxf(v4, 0.0f), 255.0f) + 0.5f);
    }
}

}  // namespace arap
