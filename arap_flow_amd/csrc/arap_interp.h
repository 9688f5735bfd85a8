// arap_interp.h -- frames from flows: the in-between frames of a pair at K times from an estimated flow, by flow splatting
// (Baker et al., IJCV 2011, section 3.3.2), the baseline a flow estimator is scored by on the in-between frames (gfx950).
//
// Definition: DESIGN.md "Frames from flows" and include/arap_opt.h; the numpy twin is tests/interp_ref.py.  Two kernels
// behind one clear of the K key images, each launched once for all K times:
//   k_interp_splat   one lane per source pixel and side (A with fwd, B with bwd).  The flow and the cost -- the photometric
//                    difference at where the flow lands -- are loaded and computed once, then K 64-bit atomicMin follow,
//                    one per time, on the key image of that time.  The key is cost << 32 | side << 31 | source index:
//                    the minimum is the lowest cost, side A on equal cost, the lowest source index within a side,
//                    whatever the order the lanes arrive in.  No other atomic, no float atomic.
//   k_interp_gather  a block owns a run of INTERP_RUN pixels of one row at one time.  Every lane loads the key of its own
//                    pixel; a ballot per wave gives the "has a key" bits of the run, one more ballot of the first wave
//                    those of the INTERP_FILL pixels left and right of it; six 64-bit words in LDS hold the run +- 16.
//                    A lane without a key cuts the 33 bits around it out of those words and finds the nearest keyed pixel
//                    of its row by two bit scans (__clzll to the left, __ffsll to the right), then reads that one foreign
//                    key: no loop of dependent loads.  Then the pixel's own work: the winner's flow, at most two bilinear
//                    flow samples (the forward-backward tests), two integer bilinear colour samples, the blend.
// Every test for "inside the frame" is made before any floorf, so every gather is inside its plane.
#pragma once
#include "../../include/arap_opt.h"
#include "arap_chain.h"

namespace arap {

constexpr int INTERP_MAX_TIMES = ARAPFLOW_INTERP_MAX_TIMES;
constexpr int INTERP_FILL = ARAPFLOW_INTERP_FILL;
constexpr int INTERP_RUN = 256;                          // pixels of a row a gather block owns: four waves
constexpr unsigned long long INTERP_NONE = ~0ull;        // a key image's clear value: no source landed here
static_assert(INTERP_FILL == 16 && INTERP_RUN % 64 == 0, "the fill window is cut out of two 64-bit words");

struct InterpJob {
    const uint8_t *A, *B;                 // [H][W][3]
    const float2 *fwd, *bwd;              // [H][W]; bwd or NULL
    unsigned long long* key;              // [K][H][W]
    uint8_t* out;                         // [K][H][W][3]
    uint8_t* src;                         // [K][H][W] or NULL
    int W, H;
    unsigned K, runs;                     // runs: gather blocks per row
    float t[INTERP_MAX_TIMES];
};

// both components finite and below 1e9 (the .flo "unknown" mark) in magnitude; false on NaN
__device__ __forceinline__ bool interp_valid(float2 u) { return fabsf(u.x) < 1e9f && fabsf(u.y) < 1e9f; }

// the nearest pixel of a coordinate inside [0, hi] (the clamp acts only where hi + .5f rounds up, beyond 2^23)
__device__ __forceinline__ int interp_round(float v, int hi) { return min((int)floorf(v + 0.5f), hi); }

// grid = (ceil(N / 256), bwd ? 2 : 1), block = 256; blockIdx.y is the side
__global__ __launch_bounds__(256) void k_interp_splat(InterpJob j)
{
    const size_t N = (size_t)j.W * j.H;
    const size_t at = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (at >= N) return;
    const unsigned side = blockIdx.y;
    const float2 u = (side ? j.bwd : j.fwd)[at];
    if (!interp_valid(u)) return;
    const int x = (int)(at % (unsigned)j.W), y = (int)(at / (unsigned)j.W);
    const float2 e = make_float2((float)x + u.x, (float)y + u.y);
    unsigned cost = 766;
    if (in_frame(e, j.W, j.H)) {
        const size_t q = (size_t)interp_round(e.y, j.H - 1) * j.W + interp_round(e.x, j.W - 1);
        const uint8_t* const a = (side ? j.B : j.A) + at * 3;
        const uint8_t* const b = (side ? j.A : j.B) + q * 3;
        cost = (unsigned)(abs((int)a[0] - (int)b[0]) + abs((int)a[1] - (int)b[1]) + abs((int)a[2] - (int)b[2]));
    }
    const unsigned long long kv = (unsigned long long)cost << 32 | (unsigned long long)side << 31 | (unsigned long long)at;
    for (unsigned k = 0; k < j.K; ++k) {
        const float tt = side ? 1.0f - j.t[k] : j.t[k];
        const float2 p = make_float2(fmaf(tt, u.x, (float)x), fmaf(tt, u.y, (float)y));
        if (!in_frame(p, j.W, j.H)) continue;
        const size_t r = (size_t)interp_round(p.y, j.H - 1) * j.W + interp_round(p.x, j.W - 1);
        atomicMin(j.key + k * N + r, kv);
    }
}

// C(I, a), a inside the frame: the integer bilinear colour sample, 8-bit weights, at most 255 * 65536 a channel
__device__ __forceinline__ void interp_colour(const uint8_t* I, float2 a, int W, int H, unsigned c[3])
{
    const int x0 = (int)floorf(a.x), y0 = (int)floorf(a.y);
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    const unsigned wx = (unsigned)(int)((a.x - (float)x0) * 256.f + 0.5f), wy = (unsigned)(int)((a.y - (float)y0) * 256.f + 0.5f);
    const uint8_t* const r0 = I + (size_t)y0 * W * 3;
    const uint8_t* const r1 = I + (size_t)y1 * W * 3;
    const unsigned w00 = (256u - wx) * (256u - wy), w01 = wx * (256u - wy), w10 = (256u - wx) * wy, w11 = wx * wy;
    for (int ch = 0; ch < 3; ++ch)
        c[ch] = w00 * r0[3 * x0 + ch] + w01 * r0[3 * x1 + ch] + w10 * r1[3 * x0 + ch] + w11 * r1[3 * x1 + ch];
}

// the forward-backward test of a flow f sampled where u points from, against u (d = f - u) or, with the sign of a
// backward flow, against -u (d = u + f); false on NaN
__device__ __forceinline__ bool interp_agree(float2 d, float2 first, float2 second)
{
    const float d2 = (d.x * d.x) + (d.y * d.y);
    const float m2 = ((first.x * first.x) + (first.y * first.y)) + ((second.x * second.x) + (second.y * second.y));
    return d2 <= fmaf(0.01f, m2, 0.5f);
}

// grid = (runs * H, K), block = INTERP_RUN; block b of a time is run b % runs of row b / runs
__global__ __launch_bounds__(INTERP_RUN) void k_interp_gather(InterpJob j)
{
    // bit 64 + l of the 384 is "pixel x0 + l has a key": word 0 carries the 16 pixels left of the run in its top bits,
    // words 1..4 the run, word 5 the 16 pixels right of it in its low bits
    __shared__ unsigned long long has[2 + INTERP_RUN / 64];
    const int W = j.W, H = j.H;
    const int y = (int)(blockIdx.x / j.runs), x0 = (int)(blockIdx.x % j.runs) * INTERP_RUN, x = x0 + (int)threadIdx.x;
    const unsigned k = blockIdx.y;
    const size_t N = (size_t)W * H;
    const unsigned long long* const key = j.key + k * N + (size_t)y * W;
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;

    unsigned long long own = x < W ? key[x] : INTERP_NONE;
    const unsigned long long mine = __ballot(own != INTERP_NONE);
    if (lane == 0) has[1 + wave] = mine;
    if (wave == 0) {
        const int hx = lane < (unsigned)INTERP_FILL ? x0 - INTERP_FILL + (int)lane : x0 + INTERP_RUN + (int)lane - INTERP_FILL;
        const bool on = lane < 2u * INTERP_FILL && hx >= 0 && hx < W && key[hx] != INTERP_NONE;
        const unsigned long long halo = __ballot(on);
        if (lane == 0) {
            has[0] = (halo & 0xffffull) << 48;
            has[1 + INTERP_RUN / 64] = (halo >> 16) & 0xffffull;
        }
    }
    __syncthreads();
    if (x >= W) return;

    unsigned filled = 0;
    if (own == INTERP_NONE) {
        // the 33 bits x - 16 .. x + 16, bit 16 the pixel's own
        const unsigned start = 64u - INTERP_FILL + threadIdx.x, w = start >> 6, sh = start & 63u;
        unsigned long long win = has[w] >> sh;
        if (sh) win |= has[w + 1] << (64u - sh);
        const unsigned long long left = win & 0xffffull, right = (win >> 17) & 0xffffull;
        const int dl = left ? __clzll((long long)left) - 47 : 2 * INTERP_FILL, dr = right ? __ffsll((long long)right) : 2 * INTERP_FILL;
        if (min(dl, dr) <= INTERP_FILL) {
            own = key[dl <= dr ? x - dl : x + dr];
            filled = 4;
        }
    }

    const size_t at = (size_t)y * W + x;
    const float t = j.t[k];
    const unsigned tq = (unsigned)(int)(t * 256.f + 0.5f);
    unsigned c[3], s = 255;
    bool blend = true;
    if (own != INTERP_NONE) {
        const size_t from = (size_t)(own & 0x7fffffffull);
        float2 u;
        if (own >> 31 & 1ull) {
            const float2 g = j.bwd[from];
            u = make_float2(-g.x, -g.y);
        } else {
            u = j.fwd[from];
        }
        const float sT = 1.0f - t;
        const float2 a0 = make_float2(fmaf(-t, u.x, (float)x), fmaf(-t, u.y, (float)y));
        const float2 b1 = make_float2(fmaf(sT, u.x, (float)x), fmaf(sT, u.y, (float)y));
        bool okA = false, okB = false;
        if (in_frame(a0, W, H)) {
            const float2 f0 = chain_sample(j.fwd, a0, W, H);
            okA = interp_agree(make_float2(f0.x - u.x, f0.y - u.y), f0, u);
        }
        if (in_frame(b1, W, H)) {
            okB = true;
            if (j.bwd) {
                const float2 g1 = chain_sample(j.bwd, b1, W, H);
                okB = interp_agree(make_float2(u.x + g1.x, u.y + g1.y), u, g1);
            }
        }
        s = filled + (okA ? (okB ? 0u : 1u) : (okB ? 2u : 3u));
        if (okA && okB) {
            unsigned ca[3], cb[3];
            interp_colour(j.A, a0, W, H, ca);
            interp_colour(j.B, b1, W, H, cb);
            for (int ch = 0; ch < 3; ++ch) c[ch] = ((256u - tq) * ca[ch] + tq * cb[ch] + (1u << 23)) >> 24;
            blend = false;
        } else if (okA || okB) {
            interp_colour(okA ? j.A : j.B, okA ? a0 : b1, W, H, c);
            for (int ch = 0; ch < 3; ++ch) c[ch] = (c[ch] + 32768u) >> 16;
            blend = false;
        }
    }
    if (blend) {
        const uint8_t* const a = j.A + at * 3;
        const uint8_t* const b = j.B + at * 3;
        for (int ch = 0; ch < 3; ++ch) c[ch] = ((256u - tq) * a[ch] + tq * b[ch] + 128u) >> 8;
    }
    uint8_t* const o = j.out + (k * N + at) * 3;
    o[0] = (uint8_t)c[0]; o[1] = (uint8_t)c[1]; o[2] = (uint8_t)c[2];
    if (j.src) j.src[k * N + at] = (uint8_t)s;
}

}  // namespace arap
