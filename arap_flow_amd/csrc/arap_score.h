// arap_score.h -- flow scoring: the Sintel / KITTI error table of an estimated flow against a generated pair (gfx950).
//
// Definitions: DESIGN.md "Flow scoring"; the numpy twin is tests/score_ref.py.  The library is built with
// -ffp-contract=off: every float operator below is one IEEE f32 operation, and sqrtf is correctly rounded (arap_device.h,
// ginv).  A pure streaming reduction: 16 bytes of flow and up to 4 bytes of planes read per pixel, nothing written but
// the table and the optional error map.  Integer accumulators only, combined by integer adds and maxima: the table is a
// function of the inputs alone, whatever order lanes, waves and blocks arrive in.
//
// One launch per call: grid = (blocks of a pair, pairs), block = 256.  The pixels of pair p start p * W * H pixels into
// every plane, so with W * H no multiple of 4 a pair's planes are misaligned for wide loads.  A pair is cut into a head
// of 0..3 pixels up to the first whose index in the whole buffer is a multiple of 4, groups of 4 pixels, and a tail of
// 0..3: a group is read with two 16-byte loads per flow, one 4-byte load of occ and of skip, one 8-byte load of dist and
// written with one 16-byte store of err, all aligned whenever the buffers themselves are (16 bytes for the flows and err,
// 8 for dist, 4 for occ and skip); head and tail go one pixel per lane.  Buffers that are not take the one-pixel path for
// every pixel (ScoreJob::vec = 0).
//
// What a lane keeps: for each of the rows 1..8 four 32-bit registers -- count, n1, n3, n5 as the four bytes
// of one, fl and nonfinite as the halves of another, the sum of q, the maximum of q -- and one for the two counts of row
// 9.  Row 0 is not kept: a counted pixel is in exactly one of the rows 6, 7, 8, so row 0 is their sum (maximum).  A lane
// sees at most SCORE_LANE_PIXELS = 129 pixels of a pair (the launch shape guarantees it), so a byte count stays <= 255
// and a sum <= 129 * 2^24 < 2^32.  Across the wave and the block every count travels as a 16-bit half (256 lanes * 255 <
// 2^16) and the sum as its low and high 16 bits in a word each (256 * 65535 < 2^32); the 64-bit values exist from the
// final step on.
#pragma once
#include "../../include/arap_opt.h"
#include "arap_device.h"

namespace arap {

enum {
    SCORE_ROWS = 10, SCORE_FIELDS = 8,
    SCORE_CLASSES = 8,                    // rows 1..8, the ones a lane accumulates: class c is row c + 1
    SCORE_FIRST_SPEED = 5,                // classes 5, 6, 7: s0-10, s10-40, s40+
    SCORE_WORDS = 6,                      // per class across lanes: count|n3, n1|n5, fl|nonfinite, sum low, sum high, max
    SCORE_RED = SCORE_CLASSES * SCORE_WORDS + 1,      // ... and the word of row 9
    SCORE_GROUP_ITERS = 32,               // at most this many groups of 4 pixels per lane and pair,
    SCORE_PIXEL_ITERS = 128,              // or this many single pixels where the buffers are not aligned
    SCORE_LANE_PIXELS = 4 * SCORE_GROUP_ITERS + 1
};
static_assert(SCORE_ROWS == ARAPFLOW_SCORE_ROWS && SCORE_FIELDS == ARAPFLOW_SCORE_FIELDS, "the table of arap_opt.h");
static_assert(SCORE_LANE_PIXELS <= 255 && SCORE_PIXEL_ITERS <= 255, "a lane's counts are bytes");

struct ScoreJob {
    const float2 *gt, *est;
    const uint8_t* occ;
    const uint16_t* dist;
    const uint8_t* skip;
    unsigned long long* table;
    float* err;
    unsigned N, n;                        // pixels of a pair, pairs
    int vec;                              // every buffer aligned for the group loads
};

struct ScoreAcc {
    unsigned cnt[SCORE_CLASSES];          // count | n1 << 8 | n3 << 16 | n5 << 24
    unsigned out[SCORE_CLASSES];          // fl | nonfinite << 16
    unsigned sum[SCORE_CLASSES], mx[SCORE_CLASSES];
    unsigned left;                        // skipped | gt_nonfinite << 16
};

// One pixel into the lane's accumulators; returns its value in the error map.  Classes below C0 are not kept (a launch
// without planes has none of the rows 1..5).
template <int C0>
__device__ __forceinline__ float score_pixel(ScoreAcc& a, float2 g, float2 s, unsigned occ, unsigned dist, unsigned skip,
                                             bool has_occ, bool has_dist)
{
    const float inf = __uint_as_float(0x7f800000u);
    const float du = s.x - g.x, dv = s.y - g.y;
    const float e2 = (du * du) + (dv * dv);
    const float e = sqrtf(e2);
    const float g2 = (g.x * g.x) + (g.y * g.y);
    const float ec = (e <= 4096.f) ? e : 4096.f;
    const unsigned q = (unsigned)((ec * 4096.f) + 0.5f);
    const bool gt_ok = g2 < inf;
    const bool counted = skip == 0 && gt_ok;
    a.left += skip != 0 ? 1u : (gt_ok ? 0u : 0x10000u);
    const bool o3 = !(e2 <= 9.f);
    const unsigned c = 1u | (!(e2 <= 1.f) ? 0x100u : 0u) | (o3 ? 0x10000u : 0u) | (!(e2 <= 25.f) ? 0x1000000u : 0u);
    const unsigned o = ((o3 && !(e2 <= (0.0025f * g2))) ? 1u : 0u) | (!(e2 < inf) ? 0x10000u : 0u);
    const bool in[SCORE_CLASSES] = {
        has_occ && occ == 0, has_occ && occ != 0,
        has_dist && dist < 100u, has_dist && dist >= 100u && dist < 3600u, has_dist && dist >= 3600u && dist < 19600u,
        g2 < 100.f, g2 >= 100.f && g2 < 1600.f, g2 >= 1600.f};
#pragma unroll
    for (int k = C0; k < SCORE_CLASSES; ++k) {
        const unsigned m = (counted && in[k]) ? 0xffffffffu : 0u;
        a.cnt[k] += c & m;
        a.out[k] += o & m;
        a.sum[k] += q & m;
        a.mx[k] = max(a.mx[k], q & m);
    }
    return counted ? e : -1.f;
}

// field f of class c from the block's totals
__device__ __forceinline__ unsigned long long score_field(const unsigned* tot, int c, int f)
{
    const unsigned* w = tot + c * SCORE_WORDS;
    switch (f) {
        case 0: return w[0] & 0xffffu;                                    // count
        case 1: return ((unsigned long long)w[4] << 16) + w[3];          // sum
        case 2: return w[1] & 0xffffu;                                    // n1
        case 3: return w[0] >> 16;                                        // n3
        case 4: return w[1] >> 16;                                        // n5
        case 5: return w[2] & 0xffffu;                                    // fl
        case 6: return w[2] >> 16;                                        // nonfinite
        default: return w[5];                                             // max
    }
}

// PLANES = false: a launch with occ, dist and skip all NULL, which has neither their loads nor the rows 1..5.  With PLANES
// a plane that is NULL is skipped by a branch that is uniform over the launch.  err likewise.
// grid = (gx, min(n, 65535)), block = 256; gx * 256 * SCORE_GROUP_ITERS >= the groups of a pair (ArapFlow_FlowScore)
template <bool PLANES>
__global__ __launch_bounds__(256) void k_flow_score(ScoreJob j)
{
    constexpr int C0 = PLANES ? 0 : SCORE_FIRST_SPEED;
    __shared__ unsigned red[4][SCORE_RED];
    __shared__ unsigned tot[SCORE_RED];
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const unsigned t0 = blockIdx.x * 256u + tid, stride = gridDim.x * 256u;
    const bool has_occ = PLANES && j.occ, has_dist = PLANES && j.dist, has_skip = PLANES && j.skip;

    for (unsigned p = blockIdx.y; p < j.n; p += gridDim.y) {
        const size_t base = (size_t)p * j.N;
        const unsigned head = j.vec ? min((unsigned)((0 - base) & 3u), j.N) : j.N;
        const unsigned groups = (j.N - head) >> 2, tail0 = head + 4u * groups, singles = head + (j.N - tail0);
        const float2* const gt = j.gt + base;
        const float2* const est = j.est + base;
        const uint8_t* const occ = has_occ ? j.occ + base : nullptr;
        const uint16_t* const dist = has_dist ? j.dist + base : nullptr;
        const uint8_t* const skip = has_skip ? j.skip + base : nullptr;
        float* const err = j.err ? j.err + base : nullptr;

        ScoreAcc a = {};
        for (unsigned g = t0; g < groups; g += stride) {
            const unsigned i = head + 4u * g;
            const float4 g01 = *(const float4*)(gt + i), g23 = *(const float4*)(gt + i + 2);
            const float4 s01 = *(const float4*)(est + i), s23 = *(const float4*)(est + i + 2);
            unsigned oc = 0u, sk = 0u;
            uint2 di = make_uint2(0u, 0u);
            if (has_occ) oc = *(const unsigned*)(occ + i);
            if (has_dist) di = *(const uint2*)(dist + i);
            if (has_skip) sk = *(const unsigned*)(skip + i);
            float4 e;
            e.x = score_pixel<C0>(a, make_float2(g01.x, g01.y), make_float2(s01.x, s01.y), oc & 0xffu, di.x & 0xffffu, sk & 0xffu, has_occ, has_dist);
            e.y = score_pixel<C0>(a, make_float2(g01.z, g01.w), make_float2(s01.z, s01.w), (oc >> 8) & 0xffu, di.x >> 16, (sk >> 8) & 0xffu, has_occ, has_dist);
            e.z = score_pixel<C0>(a, make_float2(g23.x, g23.y), make_float2(s23.x, s23.y), (oc >> 16) & 0xffu, di.y & 0xffffu, (sk >> 16) & 0xffu, has_occ, has_dist);
            e.w = score_pixel<C0>(a, make_float2(g23.z, g23.w), make_float2(s23.z, s23.w), oc >> 24, di.y >> 16, sk >> 24, has_occ, has_dist);
            if (err) *(float4*)(err + i) = e;
        }
        for (unsigned s = t0; s < singles; s += stride) {
            const unsigned i = s < head ? s : tail0 + (s - head);
            const float e = score_pixel<C0>(a, gt[i], est[i], has_occ ? occ[i] : 0u, has_dist ? dist[i] : 0u,
                                            has_skip ? skip[i] : 0u, has_occ, has_dist);
            if (err) err[i] = e;
        }

        // lanes -> wave (lane 63) -> LDS; a class whose plane is absent is zero in every lane and stays so
#pragma unroll
        for (int c = C0; c < SCORE_CLASSES; ++c) {
            unsigned w[SCORE_WORDS] = {0u, 0u, 0u, 0u, 0u, 0u};
            if (c >= SCORE_FIRST_SPEED || (c < 2 ? has_occ : has_dist)) {
                w[0] = wave_reduce_u32_l63<false>(a.cnt[c] & 0x00ff00ffu);
                w[1] = wave_reduce_u32_l63<false>((a.cnt[c] >> 8) & 0x00ff00ffu);
                w[2] = wave_reduce_u32_l63<false>(a.out[c]);
                w[3] = wave_reduce_u32_l63<false>(a.sum[c] & 0xffffu);
                w[4] = wave_reduce_u32_l63<false>(a.sum[c] >> 16);
                w[5] = wave_reduce_u32_l63<true>(a.mx[c]);
            }
            if (lane == 63u)
#pragma unroll
                for (int k = 0; k < SCORE_WORDS; ++k) red[wave][c * SCORE_WORDS + k] = w[k];
        }
        {
            const unsigned left = wave_reduce_u32_l63<false>(a.left);
            if (lane == 63u) red[wave][SCORE_RED - 1] = left;
        }
        __syncthreads();
        // waves -> block
        if (tid < SCORE_RED) {
            const bool live = tid >= C0 * SCORE_WORDS;
            const unsigned r0 = live ? red[0][tid] : 0u, r1 = live ? red[1][tid] : 0u, r2 = live ? red[2][tid] : 0u,
                           r3 = live ? red[3][tid] : 0u;
            const bool is_max = tid < SCORE_RED - 1 && tid % SCORE_WORDS == SCORE_WORDS - 1;
            tot[tid] = is_max ? max(max(r0, r1), max(r2, r3)) : (r0 + r1) + (r2 + r3);
        }
        __syncthreads();
        // block -> table: one thread per entry, and only entries that are not the identity are touched
        if (tid < SCORE_ROWS * SCORE_FIELDS) {
            const int row = (int)tid / SCORE_FIELDS, f = (int)tid % SCORE_FIELDS;
            unsigned long long v = 0ull;
            if (row == 0) {
                const unsigned long long x = score_field(tot, SCORE_FIRST_SPEED, f), y = score_field(tot, SCORE_FIRST_SPEED + 1, f),
                                         z = score_field(tot, SCORE_FIRST_SPEED + 2, f);
                v = f == SCORE_FIELDS - 1 ? max(x, max(y, z)) : x + y + z;
            } else if (row <= SCORE_CLASSES) {
                v = score_field(tot, row - 1, f);
            } else if (f < 2) {
                v = f == 0 ? (tot[SCORE_RED - 1] & 0xffffu) : (tot[SCORE_RED - 1] >> 16);
            }
            unsigned long long* const entry = j.table + ((size_t)p * SCORE_ROWS + row) * SCORE_FIELDS + f;
            if (v) {
                if (row != SCORE_ROWS - 1 && f == SCORE_FIELDS - 1) atomicMax(entry, v);
                else atomicAdd(entry, v);
            }
        }
        __syncthreads();                  // red and tot are written again for the block's next pair
    }
}

}  // namespace arap
