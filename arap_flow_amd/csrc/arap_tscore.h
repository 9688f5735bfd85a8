// arap_tscore.h -- track scoring: the TAP-Vid table of estimated point tracks against a generated track file (gfx950).
//
// Definitions: DESIGN.md "Track scoring"; the numpy twin is tests/tscore_ref.py.  The library is built with
// -ffp-contract=off: every float operator below is one IEEE f32 operation, and sqrtf is correctly rounded (arap_device.h,
// ginv).  A pure streaming reduction: 18 bytes read per point and frame, nothing written but the table.  Integer
// accumulators only, combined by integer adds and maxima: the table is a function of the inputs alone, whatever order
// lanes, waves and blocks arrive in.
//
// One launch per call, one lane per point of a chunk of THREADS points, block b takes the j.K <= 32 chunks b * K ..
// b * K + K - 1.  THREADS = 256 while that gives at most TSCORE_BLOCKS blocks of one chunk; beyond, 1024 (sixteen waves,
// four 256-point pieces at a time): what the table's atomics cost grows with the number of blocks, not of waves
// (profiles/track_score).  A lane walks the frames 1 .. F-1 and, within a frame, its point of every chunk, so at a fixed
// frame and chunk a wave reads 512 contiguous bytes of each pos and 64 of each occ; the loads of the next (frame, chunk)
// are issued before the current one is counted.  Per chunk the lane keeps two bits, in two registers for all chunks:
// "valid" and "the ground truth was hidden in an earlier frame".
//
// All but two fields are one-bit facts per lane and frame: the wave takes nine ballots per frame and chunk (valid, gv,
// ev, hidden before, in_1 .. in_16), a class is a scalar AND of them and a field's count the popcount of a scalar AND,
// added up over the chunks in scalar registers -- no lane sum, no packing.  A lane beyond P loads the last point and is
// masked out of `valid`, which every class contains, so it is in no count; every lane stays active, which is what the
// DPP sums ask for.  Only the counts that are independent are taken (TSCORE_* below): of a class with gv, count = gt_vis
// and est_vis = agree; a point-frame with gv is in exactly one of the classes 1 and 2, so every field of class 0 that
// implies gv is the sum (max: the maximum) of theirs; class 0's count is the number of valid points in every frame.
// sum and max of q are kept per lane over the chunks (<= 32 * 2^24) and reduced across the wave once per frame
// (wave_reduce_u32_l63 of arap_device.h; the sum as its low 16 bits and the rest, so that 64 lanes fit a word).
//
// Once per frame a wave adds what it has into the block's LDS copy of the table (64-bit cells: a block's sum can pass
// 2^32) with LDS integer atomics, lane 0 the counts and lane 63 the reductions; the block ends by deriving the
// dependent fields and one 64-bit integer atomic per non-zero cell of the table.
#pragma once
#include "../../include/arap_opt.h"
#include "arap_device.h"

namespace arap {

enum {
    TSCORE_MAX_FRAMES = ARAPFLOW_TSCORE_MAX_FRAMES, TSCORE_CLASSES = ARAPFLOW_TSCORE_CLASSES,
    TSCORE_FIELDS = ARAPFLOW_TSCORE_FIELDS,
    TSCORE_CELLS = TSCORE_CLASSES * TSCORE_FIELDS,        // of one frame
    TSCORE_COUNT = 0, TSCORE_GT_VIS = 1, TSCORE_EST_VIS = 2, TSCORE_AGREE = 3, TSCORE_WITHIN = 4, TSCORE_TP = 9,
    TSCORE_SUM = 14, TSCORE_MAX = 15,
    TSCORE_THREADS_SMALL = 256, TSCORE_THREADS = 1024,    // a block, and the points of a chunk: the two instantiations
    TSCORE_MAX_CHUNKS = 32,                               // chunks a block takes: one bit each in a lane's two registers
    TSCORE_BLOCKS = 256                                   // a block takes one chunk up to this many blocks, more beyond
};
static_assert(TSCORE_CLASSES == 3 && TSCORE_FIELDS == 16, "the fields written below");

struct TScoreJob {
    const float2 *gt_pos, *est_pos;       // [F][P]
    const uint8_t *gt_occ, *est_occ;      // [F][P]
    unsigned long long* table;            // [F][3][16]
    unsigned F, P, K;                     // K: chunks a block takes, 1 .. TSCORE_MAX_CHUNKS
    float sx, sy;
};

__device__ __forceinline__ void tscore_add(unsigned long long* cell, unsigned long long v)
{
    if (v) atomicAdd(cell, v);
}

// the independent counts of a class with gv over the chunks of one frame, in scalar registers
struct TScoreCounts {
    unsigned n, est, within[5], tp[5];
    __device__ __forceinline__ void add(unsigned long long m, unsigned long long ev, const unsigned long long* in)
    {
        n += __popcll(m);
        est += __popcll(m & ev);
#pragma unroll
        for (int x = 0; x < 5; ++x) {
            within[x] += __popcll(m & in[x]);
            tp[x] += __popcll(m & in[x] & ev);
        }
    }
    __device__ __forceinline__ void flush(unsigned long long* cell) const          // called by one lane
    {
        tscore_add(cell + TSCORE_COUNT, n);
        tscore_add(cell + TSCORE_EST_VIS, est);
#pragma unroll
        for (int x = 0; x < 5; ++x) {
            tscore_add(cell + TSCORE_WITHIN + x, within[x]);
            tscore_add(cell + TSCORE_TP + x, tp[x]);
        }
    }
};

// the wave's sum of a lane's sum (<= 2^29) in lane 63, as 64 bits
__device__ __forceinline__ unsigned long long tscore_wave_sum(unsigned s)
{
    const unsigned lo = wave_reduce_u32_l63<false>(s & 0xffffu), hi = wave_reduce_u32_l63<false>(s >> 16);
    return ((unsigned long long)hi << 16) + lo;
}

struct TScoreLoad { float2 g, s; unsigned go, eo; };

__device__ __forceinline__ TScoreLoad tscore_load(const TScoreJob& j, unsigned f, unsigned k)
{
    const size_t at = (size_t)f * j.P + k;
    TScoreLoad r;
    r.g = j.gt_pos[at]; r.s = j.est_pos[at];
    r.go = j.gt_occ[at]; r.eo = j.est_occ[at];
    return r;
}

// value of cell c of frame f >= 1 from the block's LDS table, which holds the independent fields only
__device__ __forceinline__ unsigned long long tscore_cell(const unsigned long long* tab, unsigned f, unsigned c)
{
    const unsigned long long* const row = tab + (size_t)f * TSCORE_CELLS;
    const unsigned cls = c / TSCORE_FIELDS, k = c % TSCORE_FIELDS;
    const unsigned long long* const c1 = row + TSCORE_FIELDS;
    const unsigned long long* const c2 = row + 2 * TSCORE_FIELDS;
    if (cls != 0) {
        const unsigned long long* const own = cls == 1 ? c1 : c2;
        return own[k == TSCORE_GT_VIS ? TSCORE_COUNT : k == TSCORE_AGREE ? TSCORE_EST_VIS : k];
    }
    if (k == TSCORE_COUNT) return tab[0];                                   // every valid point, in every frame
    if (k == TSCORE_GT_VIS) return c1[TSCORE_COUNT] + c2[TSCORE_COUNT];
    if (k == TSCORE_EST_VIS || k == TSCORE_AGREE) return row[k];
    if (k == TSCORE_MAX) return max(c1[k], c2[k]);
    return c1[k] + c2[k];
}

// grid = (ceil(ceil(P / THREADS) / K)), block = THREADS
template <unsigned THREADS>
__global__ __launch_bounds__(THREADS) void k_track_score(TScoreJob j)
{
    __shared__ unsigned long long tab[TSCORE_MAX_FRAMES * TSCORE_CELLS];
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    const unsigned cells = j.F * TSCORE_CELLS;
    for (unsigned c = tid; c < cells; c += THREADS) tab[c] = 0ull;
    __syncthreads();

    const unsigned chunks = (j.P + THREADS - 1u) / THREADS, first = blockIdx.x * j.K;
    const unsigned nc = min(j.K, chunks - first);                            // >= 1 by the grid
    const unsigned k0 = first * THREADS + tid;                                // the lane's point of chunk c is k0 + THREADS c
    auto point = [&](unsigned c) { return min(k0 + THREADS * c, j.P - 1u); };

    // frame 0: the valid and the invalid points; a lane's valid bits
    unsigned valid_bits = 0u, n_valid = 0u, n_invalid = 0u;
    for (unsigned c = 0; c < nc; ++c) {
        const bool live = k0 + THREADS * c < j.P;
        const bool valid = live && j.gt_occ[point(c)] == 0;
        valid_bits |= (valid ? 1u : 0u) << c;
        const unsigned long long b_live = __builtin_amdgcn_ballot_w64(live), b_valid = __builtin_amdgcn_ballot_w64(valid);
        n_valid += __popcll(b_valid);
        n_invalid += __popcll(b_live & ~b_valid);
    }
    if (lane == 0u) {
        tscore_add(tab + 0, n_valid);
        tscore_add(tab + 1, n_invalid);
    }

    unsigned hidden_bits = 0u;                                               // bit c: hidden in one of the frames 1 .. f-1
    TScoreLoad next = tscore_load(j, 1u, point(0));                         // (F >= 2)
    for (unsigned f = 1; f < j.F; ++f) {
        unsigned est0 = 0u, agree0 = 0u;                                    // class 0's own counts
        TScoreCounts c1 = {}, c2 = {};
        unsigned s1 = 0u, x1 = 0u, s2 = 0u, x2 = 0u;                        // per lane: sum and max of q in the classes 1 and 2
        for (unsigned c = 0; c < nc; ++c) {
            const TScoreLoad cur = next;
            if (c + 1 < nc) next = tscore_load(j, f, point(c + 1));
            else if (f + 1 < j.F) next = tscore_load(j, f + 1, point(0));
            const bool valid = (valid_bits >> c) & 1u, hb = (hidden_bits >> c) & 1u;
            const bool gv = cur.go == 0, ev = cur.eo == 0;
            const float dx = (cur.s.x - cur.g.x) * j.sx, dy = (cur.s.y - cur.g.y) * j.sy;
            const float e2 = (dx * dx) + (dy * dy);
            const float e = sqrtf(e2);
            const float ec = (e <= 4096.f) ? e : 4096.f;
            const unsigned q = (unsigned)((ec * 4096.f) + 0.5f);

            const unsigned long long b_valid = __builtin_amdgcn_ballot_w64(valid), b_gv = __builtin_amdgcn_ballot_w64(gv);
            const unsigned long long b_ev = __builtin_amdgcn_ballot_w64(ev), b_hb = __builtin_amdgcn_ballot_w64(hb);
            const unsigned long long in[5] = {
                __builtin_amdgcn_ballot_w64(gv && e2 < 1.f), __builtin_amdgcn_ballot_w64(gv && e2 < 4.f),
                __builtin_amdgcn_ballot_w64(gv && e2 < 16.f), __builtin_amdgcn_ballot_w64(gv && e2 < 64.f),
                __builtin_amdgcn_ballot_w64(gv && e2 < 256.f)};
            const unsigned long long m1 = b_valid & b_gv & ~b_hb, m2 = b_valid & b_gv & b_hb;
            est0 += __popcll(b_valid & b_ev);
            agree0 += __popcll(b_valid & ~(b_gv ^ b_ev));
            c1.add(m1, b_ev, in);
            if (m2) c2.add(m2, b_ev, in);                                   // (wave-uniform)
            const unsigned q1 = (valid && gv && !hb) ? q : 0u, q2 = (valid && gv && hb) ? q : 0u;
            s1 += q1; x1 = max(x1, q1);
            s2 += q2; x2 = max(x2, q2);
            hidden_bits |= (gv ? 0u : 1u) << c;
        }
        // the wave's frame into the block's table
        unsigned long long* const row = tab + (size_t)f * TSCORE_CELLS;
        const unsigned long long sum1 = tscore_wave_sum(s1);
        const unsigned max1 = wave_reduce_u32_l63<true>(x1);
        unsigned long long sum2 = 0ull;
        unsigned max2 = 0u;
        if (c2.n) {                                                         // (wave-uniform)
            sum2 = tscore_wave_sum(s2);
            max2 = wave_reduce_u32_l63<true>(x2);
        }
        if (lane == 0u) {
            tscore_add(row + TSCORE_EST_VIS, est0);
            tscore_add(row + TSCORE_AGREE, agree0);
            c1.flush(row + TSCORE_FIELDS);
            if (c2.n) c2.flush(row + 2 * TSCORE_FIELDS);
        }
        if (lane == 63u) {
            tscore_add(row + TSCORE_FIELDS + TSCORE_SUM, sum1);
            if (max1) atomicMax(row + TSCORE_FIELDS + TSCORE_MAX, (unsigned long long)max1);
            tscore_add(row + 2 * TSCORE_FIELDS + TSCORE_SUM, sum2);
            if (max2) atomicMax(row + 2 * TSCORE_FIELDS + TSCORE_MAX, (unsigned long long)max2);
        }
    }
    __syncthreads();
    // block -> table: the dependent fields derived, and only cells that are not the identity touched
    for (unsigned c = tid; c < cells; c += THREADS) {
        const unsigned long long v = c < TSCORE_CELLS ? tab[c] : tscore_cell(tab, c / TSCORE_CELLS, c % TSCORE_CELLS);
        if (!v) continue;
        if (c % TSCORE_FIELDS == TSCORE_MAX) atomicMax(j.table + c, v);         // (frame 0 has none)
        else atomicAdd(j.table + c, v);
    }
}

}  // namespace arap
