// arap_fscore.h -- frame scoring: the PSNR / integer-SSIM table of estimated frames against generated ones (gfx950).
//
// Definitions: DESIGN.md "Frame scoring"; the numpy twin is tests/fscore_ref.py.  The library is built with
// -ffp-contract=off and correctly rounded division: every float operator of the SSIM quotient is one IEEE f32 operation.
// Everything before it is integer arithmetic, and so is every accumulator: the table is a function of the inputs alone,
// whatever order lanes, waves and blocks arrive in.
//
// One launch per call: grid = (blocks of a pair, pairs), block = 256.  A block takes every gridDim.x-th tile of its pair,
// adds their totals up in LDS and goes to the table once a pair.  A tile is a chain of dependent steps, so a call is
// fastest with a block per tile (measured: 256, 512 and 1024 blocks in all were each slower wherever they made a block
// loop, profiles/frame_score); ArapFlow_FrameScore caps a launch at FSCORE_BLOCKS blocks only to bound it.
//
// For a tile a block owns FSCORE_TW x FSCORE_TH = 64 x 32 pixels: it counts those pixels, and the windows whose ANCHOR
// (top-left + 3) is one of them, so a pixel's planes are read once and serve both.  Such a window reaches 3 pixels left
// of and above the tile and 4 right of and below it, so the block stages 71 x 39 pixels (clipped to the frame):
//   1. raw: every staged row of both frames into LDS, 16 bytes a load.  A pair starts p * W * H * 3 bytes into the
//      buffer and a row wherever it does, so a row is fetched as the 16-byte chunks of the BUFFER that cover it (at most
//      15), each landing at its own offset in the row's LDS line; a chunk that would run past the buffer's last byte,
//      and every chunk of a buffer that is not 16-byte aligned itself (FScoreJob::vec = 0), goes byte by byte.
//   2. luma: each staged pixel's Y of both frames once, packed a | b << 8, into LDS; the thread that forms an owned
//      pixel's luma also takes its channel differences and its planes, counts it, and leaves its class mask in LDS.
//   3. windows: a wave takes 8 of the tile's 32 anchor rows, a lane one anchor column.  Per row the lane sums its 8
//      pixels horizontally (s1 | s2 << 16, ss, s12), and the four window sums run down the rows: the entering row
//      added, the leaving one (kept in registers, the loop is unrolled) subtracted.  Integers, so exact.
// Why 64 x 32: the halo is 2769 / 2048 - 1 = 35 % more pixels staged than owned (26 % of what is read); 64 x 64 would
// bring that to 23 % but leave 112 blocks for a 854 x 480 pair on 256 compute units where this gives 210, and a wave's
// 15 row sums for 8 windows would become 23 for 16 with twice the registers kept.  LDS: 18.7 KB raw + 5.5 KB luma + 4 KB
// masks, seven blocks a compute unit.
//
// Tried and dropped (profiles/frame_score): issuing all of a thread's chunk and plane loads of a tile before the first
// wait, from unrolled loops, gained up to 12 % without planes and lost up to 25 % with them, through the registers the
// loads in flight take (157 to 210 VGPRs against 128).
//
// What a lane keeps per class (rows 0..7): sse, sad, count | windows << 16, max, the sum of q, the largest 2^21 - q; and
// pixels | windows << 16 of row 8.  A lane sees at most 11 pixels and 8 windows of a tile: sse <= 11 * 195075, the sum
// of q <= 8 * 2^21.  A wave's sums stay below 2^32 (64 * 8 * 2^21 = 2^30); across the waves and the tiles they are added
// in 64 bits (one tile of identical frames has a sum of q of 2^32 exactly), the two counts of a packed word in 32 each.
#pragma once
#include "../../include/arap_opt.h"
#include "arap_device.h"

namespace arap {

enum {
    FSCORE_ROWS = 9, FSCORE_FIELDS = 7,
    FSCORE_CLASSES = 8,                   // rows 0..7, the ones a lane accumulates
    FSCORE_TW = 64, FSCORE_TH = 32,       // the pixels (and anchors) a block owns
    FSCORE_LW = FSCORE_TW + 7, FSCORE_LH = FSCORE_TH + 7,       // the pixels it stages
    FSCORE_CHUNKS = 15,                   // 16-byte chunks covering 71 * 3 bytes wherever they start: (15 + 213 + 15) / 16
    FSCORE_LINE = 16 * FSCORE_CHUNKS,
    FSCORE_WORDS = 6,                     // per class across lanes: sse, sad, count | windows << 16, max, sum of q, worst
    FSCORE_RED = FSCORE_CLASSES * FSCORE_WORDS + 1,             // ... and the word of row 8
    FSCORE_SKIPPED = 0x100,               // a class mask's "left out" bit
    FSCORE_BLOCKS = 1 << 16               // blocks of a launch, at most (while every pair has one)
};
static_assert(FSCORE_ROWS == ARAPFLOW_FSCORE_ROWS && FSCORE_FIELDS == ARAPFLOW_FSCORE_FIELDS, "the table of arap_opt.h");
static_assert(15 + 3 * FSCORE_LW <= FSCORE_LINE, "a staged row fits its LDS line at any offset");

struct FScoreJob {
    const uint8_t *ref, *est;
    const uint8_t* occ;
    const uint16_t* dist;
    const uint8_t *skip, *obj;
    unsigned long long* table;
    float* ssim;
    unsigned W, H, n;
    unsigned tx, tiles;                   // tiles a row of tiles, tiles a pair
    int vec;                              // ref and est 16-byte aligned
};

template <int NC>
struct FScoreAcc {
    unsigned sse[NC], sad[NC], cw[NC], mx[NC], qs[NC], worst[NC];
    unsigned left;                        // pixels | windows << 16 of row 8
};

// the integer SSIM of one window from its four sums: s and q of DESIGN.md
__device__ __forceinline__ float fscore_ssim(unsigned sab, unsigned ss, unsigned s12, unsigned& q)
{
    const int s1 = (int)(sab & 0xffffu), s2 = (int)(sab >> 16);
    const int vars = 64 * (int)ss - s1 * s1 - s2 * s2, covar = 64 * (int)s12 - s1 * s2;
    const int A = 2 * s1 * s2 + 416, B = 2 * covar + 235963, C = s1 * s1 + s2 * s2 + 416, D = vars + 235963;
    const float s = ((float)A * (float)B) / ((float)C * (float)D);
    const float t = fmaxf(s + 1.0f, 0.0f);
    q = (unsigned)((t * 1048576.f) + 0.5f);
    return s;
}

// PLANES = false: a launch with occ, dist, skip and obj all NULL, which has neither their loads nor the rows 1..8.  With
// PLANES a plane that is NULL is skipped by a branch that is uniform over the launch.  ssim likewise.
// grid = (gx <= tiles, gy <= n), block = 256; both are looped over where a call has more
template <bool PLANES>
__global__ __launch_bounds__(256) void k_frame_score(FScoreJob j)
{
    constexpr int NC = PLANES ? FSCORE_CLASSES : 1;
    __shared__ __attribute__((aligned(16))) uint8_t raw[2][FSCORE_LH][FSCORE_LINE];
    __shared__ unsigned short luma[FSCORE_LH][FSCORE_LW];
    __shared__ unsigned short cls[FSCORE_TH][FSCORE_TW];
    __shared__ unsigned red[4][FSCORE_RED];
    __shared__ unsigned long long tot[FSCORE_RED];
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const int W = (int)j.W, H = (int)j.H;
    const size_t N = (size_t)j.W * j.H, bytes = (size_t)j.n * N * 3;
    const bool has_occ = PLANES && j.occ, has_dist = PLANES && j.dist, has_skip = PLANES && j.skip, has_obj = PLANES && j.obj;
    const bool any_window = W >= 8 && H >= 8;

    for (unsigned p = blockIdx.y; p < j.n; p += gridDim.y) {
        if (tid < FSCORE_RED) tot[tid] = 0ull;            // (first added to after the barriers of a tile)
        for (unsigned tile = blockIdx.x; tile < j.tiles; tile += gridDim.x) {
            const size_t base = (size_t)p * N;
            const int X0 = (int)(tile % j.tx) * FSCORE_TW, Y0 = (int)(tile / j.tx) * FSCORE_TH;
            const int xl = max(X0 - 3, 0), xr = min(X0 + FSCORE_TW + 3, W - 1);
            const int yt = max(Y0 - 3, 0), yb = min(Y0 + FSCORE_TH + 3, H - 1);
            const int cols = xr - xl + 1, rows = yb - yt + 1;

            // 1. raw rows of both frames
            for (unsigned i = tid; i < 2u * FSCORE_LH * FSCORE_CHUNKS; i += 256u) {
                const unsigned f = i / (FSCORE_LH * FSCORE_CHUNKS), rem = i - f * (FSCORE_LH * FSCORE_CHUNKS);
                const unsigned r = rem / FSCORE_CHUNKS, ch = rem - r * FSCORE_CHUNKS;
                if ((int)r >= rows) continue;
                const size_t b0 = (base + (size_t)(yt + (int)r) * j.W + (size_t)xl) * 3, b1 = b0 + (size_t)cols * 3;
                const size_t c0 = (b0 & ~(size_t)15) + 16u * ch;
                if (c0 >= b1) continue;
                const uint8_t* const src = f ? j.est : j.ref;
                if (j.vec && c0 + 16 <= bytes) {
                    *(uint4*)&raw[f][r][16u * ch] = *(const uint4*)(src + c0);
                } else {
                    for (unsigned k = 0; k < 16u; ++k)
                        if (c0 + k >= b0 && c0 + k < b1) raw[f][r][16u * ch + k] = src[c0 + k];
                }
            }
            __syncthreads();

            // 2. luma of every staged pixel; the owned ones are counted
            FScoreAcc<NC> a = {};
            for (unsigned i = tid; i < (unsigned)(FSCORE_LH * FSCORE_LW); i += 256u) {
                const int r = (int)(i / FSCORE_LW), c = (int)(i - (unsigned)r * FSCORE_LW);
                if (r >= rows || c >= cols) continue;
                const int x = xl + c, y = yt + r;
                const size_t g = base + (size_t)y * j.W + (size_t)x;
                const unsigned o = (unsigned)(((g - (size_t)c) * 3) & 15) + 3u * (unsigned)c;
                const int r0 = raw[0][r][o], r1 = raw[0][r][o + 1], r2 = raw[0][r][o + 2];
                const int e0 = raw[1][r][o], e1 = raw[1][r][o + 1], e2 = raw[1][r][o + 2];
                const unsigned ya = (unsigned)(77 * r0 + 150 * r1 + 29 * r2 + 128) >> 8;
                const unsigned ye = (unsigned)(77 * e0 + 150 * e1 + 29 * e2 + 128) >> 8;
                luma[r][c] = (unsigned short)(ya | (ye << 8));
                if (x < X0 || x >= X0 + FSCORE_TW || y < Y0 || y >= Y0 + FSCORE_TH) continue;
                const unsigned d0 = (unsigned)abs(r0 - e0), d1 = (unsigned)abs(r1 - e1), d2 = (unsigned)abs(r2 - e2);
                const unsigned sse = d0 * d0 + d1 * d1 + d2 * d2, sad = d0 + d1 + d2, mx = max(d0, max(d1, d2));
                unsigned m = 1u;
                if (PLANES) {
                    if (has_occ) m |= j.occ[g] == 0 ? 2u : 4u;
                    if (has_dist) {
                        const unsigned d = j.dist[g];
                        m |= d < 100u ? 8u : d < 3600u ? 16u : d < 19600u ? 32u : 0u;
                    }
                    if (has_obj) m |= j.obj[g] == 0 ? 64u : 128u;
                    if (has_skip && j.skip[g] != 0) m = FSCORE_SKIPPED;
                    cls[y - Y0][x - X0] = (unsigned short)m;
                }
                a.left += m >> 8;
#pragma unroll
                for (int k = 0; k < NC; ++k) {
                    const unsigned on = ((m >> k) & 1u) ? 0xffffffffu : 0u;
                    a.sse[k] += sse & on;
                    a.sad[k] += sad & on;
                    a.cw[k] += 1u & on;
                    a.mx[k] = max(a.mx[k], mx & on);
                }
                const bool anchor = any_window && x >= 3 && x <= W - 5 && y >= 3 && y <= H - 5;
                if (j.ssim && !(anchor && m != FSCORE_SKIPPED)) j.ssim[g] = -2.f;
            }
            __syncthreads();

            // 3. the windows anchored on the tile: this wave's 8 anchor rows, this lane's column
            const int y_lo = max(Y0 + 8 * (int)wave, 3), y_hi = min(Y0 + 8 * (int)wave + 7, H - 5);
            if (any_window && y_lo <= y_hi) {
                const int ax = X0 + (int)lane;
                const bool okx = ax >= 3 && ax <= W - 5;
                const int cb = okx ? ax - 3 - xl : 0, rb = y_lo - 3 - yt, kmax = y_hi - y_lo + 7;
                unsigned hab[7], hss[7], h12[7];
                unsigned Sab = 0u, Sss = 0u, S12 = 0u;
#pragma unroll
                for (int k = 0; k < 15; ++k) {
                    if (k > kmax) continue;
                    unsigned ab = 0u, ss = 0u, s12 = 0u;
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const unsigned v = luma[rb + k][cb + i], ya = v & 0xffu, ye = v >> 8;
                        ab += ya | (ye << 16);
                        ss += ya * ya + ye * ye;
                        s12 += ya * ye;
                    }
                    Sab += ab; Sss += ss; S12 += s12;
                    if (k < 7) {
                        hab[k] = ab; hss[k] = ss; h12[k] = s12;
                    } else {
                        if (okx) {
                            const int ay = y_lo + (k - 7);
                            unsigned q;
                            const float s = fscore_ssim(Sab, Sss, S12, q);
                            const unsigned m = PLANES ? cls[ay - Y0][lane] : 1u;
                            a.left += (m >> 8) << 16;
#pragma unroll
                            for (int c = 0; c < NC; ++c) {
                                const unsigned on = ((m >> c) & 1u) ? 0xffffffffu : 0u;
                                a.cw[c] += 0x10000u & on;
                                a.qs[c] += q & on;
                                a.worst[c] = max(a.worst[c], ((1u << 21) - q) & on);
                            }
                            if (j.ssim && m != FSCORE_SKIPPED) j.ssim[base + (size_t)ay * j.W + (size_t)ax] = s;
                        }
                        if (k < 14) {
                            Sab -= hab[k - 7]; Sss -= hss[k - 7]; S12 -= h12[k - 7];
                        }
                    }
                }
            }

            // lanes -> wave (lane 63) -> LDS; a class whose plane is absent is zero in every lane and stays so
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                unsigned w[FSCORE_WORDS] = {0u, 0u, 0u, 0u, 0u, 0u};
                if (c == 0 || (c < 3 ? has_occ : c < 6 ? has_dist : has_obj)) {
                    w[0] = wave_reduce_u32_l63<false>(a.sse[c]);
                    w[1] = wave_reduce_u32_l63<false>(a.sad[c]);
                    w[2] = wave_reduce_u32_l63<false>(a.cw[c]);
                    w[3] = wave_reduce_u32_l63<true>(a.mx[c]);
                    w[4] = wave_reduce_u32_l63<false>(a.qs[c]);
                    w[5] = wave_reduce_u32_l63<true>(a.worst[c]);
                }
                if (lane == 63u)
#pragma unroll
                    for (int k = 0; k < FSCORE_WORDS; ++k) red[wave][c * FSCORE_WORDS + k] = w[k];
            }
            {
                const unsigned left = wave_reduce_u32_l63<false>(a.left);
                if (lane == 63u) red[wave][FSCORE_RED - 1] = left;
            }
            __syncthreads();
            // waves -> the block's totals of this pair, in 64 bits; a packed pair of counts opens into its two halves
            if (tid < FSCORE_RED) {
                const bool live = tid < NC * FSCORE_WORDS || tid == FSCORE_RED - 1;
                const unsigned k = tid % FSCORE_WORDS;
                const bool is_max = tid < FSCORE_RED - 1 && (k == 3 || k == 5), packed = tid == FSCORE_RED - 1 || k == 2;
                unsigned long long v = tot[tid];
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const unsigned r = live ? red[w][tid] : 0u;
                    const unsigned long long r64 = packed ? ((unsigned long long)(r >> 16) << 32) | (r & 0xffffu) : r;
                    v = is_max ? max(v, r64) : v + r64;
                }
                tot[tid] = v;
            }
            __syncthreads();              // every other LDS array is written again for the block's next tile
        }
        // block -> table, once a pair: one thread per entry, and only entries that are not the identity are touched
        if (tid < FSCORE_ROWS * FSCORE_FIELDS) {
            const int row = (int)tid / FSCORE_FIELDS, f = (int)tid % FSCORE_FIELDS;
            unsigned long long v = 0ull;
            if (row < FSCORE_CLASSES) {
                const unsigned long long* const w = tot + row * FSCORE_WORDS;
                v = f == 0 ? (w[2] & 0xffffffffull) : f == 1 ? w[0] : f == 2 ? w[1] : f == 3 ? w[3] : f == 4 ? (w[2] >> 32)
                    : f == 5 ? w[4] : w[5];
            } else if (f < 2) {
                v = f == 0 ? (tot[FSCORE_RED - 1] & 0xffffffffull) : (tot[FSCORE_RED - 1] >> 32);
            }
            unsigned long long* const entry = j.table + ((size_t)p * FSCORE_ROWS + row) * FSCORE_FIELDS + f;
            if (v) {
                if (row < FSCORE_CLASSES && (f == 3 || f == 6)) atomicMax(entry, v);
                else atomicAdd(entry, v);
            }
        }
        __syncthreads();                  // tot is cleared for the block's next pair
    }
}

}  // namespace arap
