// arap_mscore.h -- map scoring: the DAVIS J / F table of estimated label maps and the precision / recall histogram of
// estimated occlusion and motion-boundary maps, with the tolerant boundary match both share (gfx950).
//
// Definitions: DESIGN.md "Map scoring"; the numpy twin is tests/mscore_ref.py.  Integers only: no float anywhere in this
// file.  Counts are combined by integer adds alone, so every output is a function of the inputs whatever order lanes,
// waves and blocks arrive in.
//
// Order on the stream:   k_mscore_count                                              (one launch for all n maps)
//   then per boundary match (a label of a map, or a threshold of a map), one map at a time through the call's scratch:
//                          k_mscore_sets -> k_seg_cols -> k_seg_rows -> k_seg_cols -> k_seg_rows -> k_mscore_hits
// k_seg_cols / k_seg_rows are arap_seg.h's exact distance passes, used as they are.
//
// k_mscore_count.  The pixels of map p start p * W * H bytes into every plane, so with W * H no multiple of 16 a map is
// misaligned for wide loads.  As in k_flow_score a map is cut into a head of 0..15 pixels up to the first whose index in
// the whole buffer is a multiple of 16, groups of 16 pixels and a tail of 0..15: a group is one 16-byte load per plane
// and lane, aligned whenever the buffers themselves are; head and tail go one pixel per lane, and so does every pixel of
// buffers that are not aligned (MScoreJob::vec = 0).
//
// What binds it is contention, not bandwidth: an occlusion map has two values and a label map a handful, so an atomic per
// pixel would serialise a wave on one address.  A wave therefore aggregates before any atomic: for each of the 16 pixel
// slots of a group it loops over the DISTINCT keys its lanes hold (readlane, ballot of the lanes with that key,
// popcount) and one lane adds the count to the block's LDS table, one LDS add per distinct key and wave.  The counts of
// row 0 are kept per lane (fewer than 2^31 pixels) and summed over the wave once per map, by arap_device.h's integer DPP tree.
// The LDS table holds full 32-bit words (a block sees fewer than 2^31 pixels of a map: n * W * H < 2^31), and only its
// non-zero entries reach the 64-bit table, by integer vector atomics.  Every loop that holds a ballot or a barrier has
// a trip count that is uniform over the wave (block).
#pragma once
#include "../../include/arap_opt.h"
#include "arap_device.h"
#include "arap_seg.h"

namespace arap {

enum {
    LSCORE_FIELDS = 8,
    MSCORE_MAX_THR = 8,
    MSCORE_LABEL_WORDS = 3 * 256,         // gt, est, inter of the rows 0..255 (row 0's three are not used)
    MSCORE_FRAME_WORDS = 5,               // row 0 of a label table
    MSCORE_HIST_WORDS = 512,
    MSCORE_BLOCKS = 1024                  // about four blocks of 256 per CU: the grid's blocks in all
};
static_assert(LSCORE_FIELDS == ARAPFLOW_LSCORE_FIELDS && MSCORE_MAX_THR == ARAPFLOW_MSCORE_MAX_THR, "arap_opt.h");

struct MScoreJob {
    const uint8_t *gt, *est, *skip;       // skip may be NULL
    unsigned long long* out;              // table uint64[n][L+1][8], or hist uint64[n][2][256]
    unsigned N, n, L;                     // pixels of a map, maps, labels scored
    int vec;                              // every plane aligned for the group loads
};

// word q (0..3) of a 16-byte group: selects, no indexed register array
__device__ __forceinline__ unsigned mscore_word(const uint4& v, int q)
{
    return q == 0 ? v.x : q == 1 ? v.y : q == 2 ? v.z : v.w;
}

// One pixel slot of the wave: `live` lanes hold a pixel of the map (g, e, s = gt, est, skip).  Called by all lanes of the
// wave together.  LABELS: tab[3 k + f] for the label rows, fr[] the lane's five counts of row 0.  Otherwise
// tab[256 c + v].  PLAIN (experiments, ARAPOPT_MSCORE_PLAIN=1; the histogram only): one LDS atomic per counted pixel,
// what the aggregation is measured against (profiles/map_score/README.md).
template <bool LABELS, bool PLAIN>
__device__ __forceinline__ void mscore_slot(unsigned* tab, unsigned (&fr)[MSCORE_FRAME_WORDS], unsigned L, bool live, unsigned g,
                                            unsigned e, unsigned s, unsigned lane)
{
    const bool counted = live && s == 0;
    const unsigned key = LABELS ? (g | (e << 8)) : (((g != 0) ? 256u : 0u) | e);
    if (LABELS) {
        fr[0] += counted ? 1u : 0u;
        fr[1] += live && s != 0 ? 1u : 0u;
        fr[2] += counted && g == e ? 1u : 0u;
        fr[3] += counted && g > L ? 1u : 0u;
        fr[4] += counted && e > L ? 1u : 0u;
    }
    if (PLAIN) {
        if (counted) atomicAdd(&tab[key], 1u);
        return;
    }
    unsigned long long todo = __ballot(counted);
    while (todo) {                                           // uniform: todo is the wave's
        const unsigned first = (unsigned)__ffsll((long long)todo) - 1u;
        const unsigned k = (unsigned)__builtin_amdgcn_readlane((int)key, (int)first);
        const unsigned long long same = __ballot(counted && key == k);
        const unsigned c = (unsigned)__popcll(same);
        if (lane == first) {
            if (LABELS) {
                const unsigned kg = k & 0xffu, ke = k >> 8;
                if (kg >= 1u && kg <= L) atomicAdd(&tab[3u * kg], c);
                if (ke >= 1u && ke <= L) atomicAdd(&tab[3u * ke + 1u], c);
                if (kg == ke && kg >= 1u && kg <= L) atomicAdd(&tab[3u * kg + 2u], c);
            } else {
                atomicAdd(&tab[k], c);
            }
        }
        todo &= ~same;
    }
}

// LABELS: the rows' region counts and row 0 of ArapFlow_LabelScore's table; else ArapFlow_MapScore's histogram.
// grid = (gx, min(n, 65535)), block = 256; a block loops over the groups of its maps
template <bool LABELS, bool PLAIN = false>
__global__ __launch_bounds__(256) void k_mscore_count(MScoreJob j)
{
    constexpr unsigned WORDS = LABELS ? MSCORE_LABEL_WORDS + MSCORE_FRAME_WORDS : MSCORE_HIST_WORDS;
    __shared__ unsigned tab[WORDS];
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    const unsigned b0 = blockIdx.x * 256u, stride = gridDim.x * 256u;
    const unsigned used = LABELS ? 3u * (j.L + 1u) : (unsigned)MSCORE_HIST_WORDS;      // the words of tab a map can touch

    for (unsigned p = blockIdx.y; p < j.n; p += gridDim.y) {
        for (unsigned t = tid; t < WORDS; t += 256u) tab[t] = 0u;
        __syncthreads();
        const size_t base = (size_t)p * j.N;
        const unsigned head = j.vec ? min((unsigned)((0 - base) & 15u), j.N) : j.N;
        const unsigned groups = (j.N - head) >> 4, tail0 = head + 16u * groups, singles = head + (j.N - tail0);
        const uint8_t* const gt = j.gt + base;
        const uint8_t* const est = j.est + base;
        const uint8_t* const skip = j.skip ? j.skip + base : nullptr;
        unsigned fr[MSCORE_FRAME_WORDS] = {0u, 0u, 0u, 0u, 0u};

        for (unsigned g0 = b0; g0 < groups; g0 += stride) {
            const unsigned g = g0 + tid;
            const bool live = g < groups;
            uint4 vg = make_uint4(0u, 0u, 0u, 0u), ve = vg, vs = vg;
            if (live) {
                const unsigned i = head + 16u * g;
                vg = *(const uint4*)(gt + i);
                ve = *(const uint4*)(est + i);
                if (skip) vs = *(const uint4*)(skip + i);
            }
            // a word of four slots at a time, and with labels a slot at a time: unrolled further the compiler forms the
            // slots' lane masks up front and runs out of scalar registers (131 spilled with all 16 unrolled)
            constexpr int UNROLL = LABELS ? 1 : 4;
#pragma unroll 1
            for (int q = 0; q < 4; ++q) {
                const unsigned wg = mscore_word(vg, q), we = mscore_word(ve, q), ws = mscore_word(vs, q);
#pragma unroll UNROLL
                for (int k = 0; k < 32; k += 8)
                    mscore_slot<LABELS, PLAIN>(tab, fr, j.L, live, (wg >> k) & 0xffu, (we >> k) & 0xffu, (ws >> k) & 0xffu, lane);
            }
        }
        for (unsigned s0 = b0; s0 < singles; s0 += stride) {
            const unsigned s = s0 + tid;
            const bool live = s < singles;
            unsigned g = 0u, e = 0u, sk = 0u;
            if (live) {
                const unsigned i = s < head ? s : tail0 + (s - head);
                g = gt[i];
                e = est[i];
                if (skip) sk = skip[i];
            }
            mscore_slot<LABELS, PLAIN>(tab, fr, j.L, live, g, e, sk, lane);
        }
        if (LABELS)
#pragma unroll
            for (int f = 0; f < MSCORE_FRAME_WORDS; ++f) {
                const unsigned w = wave_reduce_u32_l63<false>(fr[f]);             // all 64 lanes are here
                if (lane == 63u && w) atomicAdd(&tab[MSCORE_LABEL_WORDS + f], w);
            }
        __syncthreads();
        // block -> table: only entries that are not zero are touched
        if (LABELS) {
            unsigned long long* const out = j.out + (size_t)p * (j.L + 1u) * LSCORE_FIELDS;
            for (unsigned t = 3u + tid; t < used; t += 256u) {
                const unsigned v = tab[t];
                if (v) atomicAdd(out + (size_t)(t / 3u) * LSCORE_FIELDS + t % 3u, (unsigned long long)v);
            }
            if (tid < MSCORE_FRAME_WORDS) {
                const unsigned v = tab[MSCORE_LABEL_WORDS + tid];
                if (v) atomicAdd(out + tid, (unsigned long long)v);
            }
        } else {
            unsigned long long* const out = j.out + (size_t)p * MSCORE_HIST_WORDS;
            for (unsigned t = tid; t < used; t += 256u) {
                const unsigned v = tab[t];
                if (v) atomicAdd(out + t, (unsigned long long)v);
            }
        }
        __syncthreads();                  // tab is cleared again for the block's next map
    }
}

// The two byte maps (1 / 0) of one boundary match of one map, skipped pixels removed.
// LABELS: A = bmap(gt == key), B = bmap(est == key), the DAVIS toolkit's seg2bmap at equal size: a pixel differs from its
// right, lower or lower-right neighbour; the last row looks right only, the last column down only, the last pixel is 0.
// Otherwise: A = gt != 0, B = est >= key.
// grid = (ceil(W/64), ceil(H/4)), block = (64,4)
template <bool LABELS>
__global__ __launch_bounds__(256) void k_mscore_sets(const uint8_t* __restrict__ gt, const uint8_t* __restrict__ est,
                                                     const uint8_t* __restrict__ skip, unsigned key, uint8_t* __restrict__ A,
                                                     uint8_t* __restrict__ B, int W, int H)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t i = (size_t)y * W + x;
    bool a, b;
    if (LABELS) {
        const bool right = x + 1 < W, down = y + 1 < H;
        const bool mg = gt[i] == key, me = est[i] == key;
        a = b = false;
        if (right) {
            a = a || (gt[i + 1] == key) != mg;
            b = b || (est[i + 1] == key) != me;
        }
        if (down) {
            a = a || (gt[i + W] == key) != mg;
            b = b || (est[i + W] == key) != me;
        }
        if (right && down) {
            a = a || (gt[i + W + 1] == key) != mg;
            b = b || (est[i + W + 1] == key) != me;
        }
    } else {
        a = gt[i] != 0;
        b = est[i] >= key;
    }
    const bool keep = !skip || skip[i] == 0;
    A[i] = a && keep ? 1 : 0;
    B[i] = b && keep ? 1 : 0;
}

// The four numbers of a boundary match into out[0..3]: a = |A|, b = |B|, a_hit = the pixels of A within the radius of B
// (dB, the distance to B, is not SEG_FAR), b_hit likewise.  Wave ballots and popcounts added up in wave-uniform registers,
// one LDS word per wave and number, one 64-bit atomic per block and non-zero number.  The loop's trip count is uniform
// over the block and the only return lies behind the barrier.
// grid = min(ceil(N / 256), MSCORE_BLOCKS), block = 256
__global__ __launch_bounds__(256) void k_mscore_hits(const uint8_t* __restrict__ A, const uint8_t* __restrict__ B,
                                                     const uint16_t* __restrict__ dA, const uint16_t* __restrict__ dB,
                                                     unsigned long long* __restrict__ out, unsigned N)
{
    __shared__ unsigned red[4][4];
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    unsigned c[4] = {0u, 0u, 0u, 0u};
    for (unsigned i0 = blockIdx.x * 256u; i0 < N; i0 += gridDim.x * 256u) {
        const unsigned i = i0 + tid;
        const bool live = i < N;
        const bool a = live && A[i] != 0, b = live && B[i] != 0;
        const bool ah = a && dB[i] != SEG_FAR, bh = b && dA[i] != SEG_FAR;
        c[0] += (unsigned)__popcll(__ballot(a));
        c[1] += (unsigned)__popcll(__ballot(b));
        c[2] += (unsigned)__popcll(__ballot(ah));
        c[3] += (unsigned)__popcll(__ballot(bh));
    }
    if (lane == 0u)
#pragma unroll
        for (int k = 0; k < 4; ++k) red[wave][k] = c[k];
    __syncthreads();
    if (tid >= 4u) return;
    const unsigned v = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
    if (v) atomicAdd(out + tid, (unsigned long long)v);
}

}  // namespace arap
