// arap_seg.h -- segment maps of a pair: object index maps of both frames, motion boundaries of the forward and the
// backward flow, and the squared distance to the nearest boundary (gfx950).
//
// Definitions: DESIGN.md "Segment maps"; the numpy twin is tests/seg_ref.py.  The frame-2 side reads the layered
// rasteriser's key image (k_layers_raster, arap_layers.h) and k_layers_keys' backward flow; nothing of the family is
// restated here: the owner is layer_owner, the winner key_winner, the background's flow bg_apply's expression.  The
// library is built with -ffp-contract=off: every float operator below is one IEEE f32 operation.  No atomics of its own,
// no float reduction; every output is a function of the inputs alone.
//
// Order on the stream, per frame:   k_seg_index1 | k_layers_raster -> k_layers_keys -> k_seg_index2
//                                   -> k_seg_jump -> [k_seg_cols -> k_seg_rows]
// The full flow of a frame (F1, then B2: the frames run one after the other and share the buffer), the boundary map when
// it is no output, and the column distances live in the call's scratch.
//
// The distance is exact by construction: the squared Euclidean distance to the nearest boundary pixel is
// min over columns x' of (x - x')^2 + g(x', y)^2 with g the distance to the nearest boundary pixel INSIDE column x', and
// a candidate can only be <= radius^2 when |x - x'| <= radius and g <= radius.  k_seg_cols forms g capped at radius + 1
// (one byte: radius <= 254), k_seg_rows the minimum; all of it in integers.
#pragma once
#include "arap_bg.h"
#include "arap_layers.h"

namespace arap {

constexpr int SEG_MAX_RADIUS = 254;                     // ARAPFLOW_SEG_MAX_RADIUS: radius + 1 fits the byte of g
constexpr unsigned SEG_FAR = 65535u;                    // the sentinel of dist, and "no boundary within reach" in LDS
constexpr int SEG_WIN = 64 + 2 * SEG_MAX_RADIUS;        // the widest row window of a block

// the flow of the moving background at (x, y): ArapFlow_Background's expression for flow_full / bwd_full
__device__ __forceinline__ float2 seg_bg_flow(const BgMap& G, int x, int y)
{
    const float2 p = bg_apply(G, x, y);
    return make_float2(p.x - (float)x, p.y - (float)y);
}

// frame 1, per pixel p: idx1 = owner + 1 (0: no layer owns p); F1 = the owner's flow, or the background's (MOVING), or 0.
// Each output only if its pointer is set.  grid = (ceil(W/64), ceil(H/4)), block = (64,4)
template <bool MOVING>
__global__ __launch_bounds__(256) void k_seg_index1(LayerSet s, BgMap G, uint8_t* __restrict__ idx, float2* __restrict__ F,
                                                    int W, int H)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= W || y >= H) return;
    const int N = W * H, i = x + W * y;
    const unsigned l = layer_owner(s, N, i);
    if (idx) idx[i] = l == LAYER_NONE ? 0 : (uint8_t)(l + 1u);
    if (!F) return;
    float2 f = make_float2(0.f, 0.f);
    if (l != LAYER_NONE) f = s.flows[(size_t)l * N + i];
    else if (MOVING) f = seg_bg_flow(G, x, y);
    F[i] = f;
}

// frame 2, per pixel q, between k_layers_keys (which has written B2 of the covered pixels and 0 elsewhere into F) and the
// clearing of the keys: idx2 = the winner's layer + 1 (0: nothing drawn); MOVING: F of an uncovered pixel = the
// background's backward flow.  Same launch shape.
template <bool MOVING>
__global__ __launch_bounds__(256) void k_seg_index2(const unsigned long long* __restrict__ key, BgMap Ginv,
                                                    uint8_t* __restrict__ idx, float2* __restrict__ F, int W, int H)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= W || y >= H) return;
    const int i = x + W * y;
    const KeyWinner w = key_winner(key[i]);
    if (idx) idx[i] = w.covered ? (uint8_t)(w.layer + 1u) : 0;
    if (MOVING && F && !w.covered) F[i] = seg_bg_flow(Ginv, x, y);
}

// does the flow jump between two neighbours?  !(d2 <= tau2): a non-finite difference is a jump
__device__ __forceinline__ bool seg_jump(float2 a, float2 b, float tau2)
{
    const float dx = a.x - b.x, dy = a.y - b.y;
    const float d2 = dx * dx + dy * dy;
    return !(d2 <= tau2);
}

// mb = 255 where the flow jumps against a 4-neighbour inside the frame.  The neighbours are read through the cache: a
// wave's 64 pixels of one row share their left / right values and the block's four rows their up / down ones, so a
// staged tile would save no memory traffic, only L1 hits (profiles/seg/README.md).  Same launch shape.
__global__ __launch_bounds__(256) void k_seg_jump(const float2* __restrict__ F, float tau2, uint8_t* __restrict__ mb, int W, int H)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= W || y >= H) return;
    const int i = x + W * y;
    const float2 f = F[i];
    bool b = false;
    if (x > 0) b = b || seg_jump(f, F[i - 1], tau2);
    if (x + 1 < W) b = b || seg_jump(f, F[i + 1], tau2);
    if (y > 0) b = b || seg_jump(f, F[i - W], tau2);
    if (y + 1 < H) b = b || seg_jump(f, F[i + W], tau2);
    mb[i] = b ? 255 : 0;
}

// pass 1 of the distance: g(x, y) = min(|y - y'| over boundary pixels (x, y'), radius + 1).  A column is a chain -- a
// counter swept down and back up -- and one thread per column leaves a frame of 854 x 480 with 854 threads of 960
// dependent steps each (measured: 115 .. 135 us a frame, four times the whole layered warp; profiles/seg/README.md).  So a
// column is cut into SEG_RUNS runs of S = ceil(H / SEG_RUNS) rows, one thread each: it finds the first and last boundary
// row of its run, the block exchanges them in LDS, a thread looks up the nearest boundary above and below its run (at
// most SEG_RUNS - 1 LDS reads each way) and then sweeps its own S rows down and back up from those.  The same integers as
// the one long sweep.  A wave is 16 neighbouring columns of 4 runs: 4 segments of 16 consecutive bytes per load.  Every
// thread of the block, the ones outside the frame or past its last row included, reaches the barrier.
// grid = ceil(W / SEG_COLS), block = (SEG_COLS, SEG_RUNS)
constexpr int SEG_COLS = 16, SEG_RUNS = 64;

__global__ __launch_bounds__(SEG_COLS * SEG_RUNS) void k_seg_cols(const uint8_t* __restrict__ mb, uint8_t* __restrict__ g,
                                                                  int radius, int W, int H)
{
    __shared__ int first[SEG_RUNS][SEG_COLS], last[SEG_RUNS][SEG_COLS];      // rows, -1: no boundary in the run
    const int tx = threadIdx.x, t = threadIdx.y;
    const int x = blockIdx.x * SEG_COLS + tx;
    const int S = (H + SEG_RUNS - 1) / SEG_RUNS;
    const int y0 = min(t * S, H), y1 = min(y0 + S, H);
    int f = -1, l = -1;
    if (x < W)
        for (int y = y0; y < y1; ++y)
            if (mb[(size_t)y * W + x]) {
                if (f < 0) f = y;
                l = y;
            }
    first[t][tx] = f;
    last[t][tx] = l;
    __syncthreads();
    if (x >= W || y0 >= y1) return;
    int above = -1, below = -1;
    for (int k = t - 1; k >= 0 && above < 0; --k) above = last[k][tx];
    for (int k = t + 1; k < SEG_RUNS && below < 0; ++k) below = first[k][tx];
    const int cap = radius + 1;
    int c = above < 0 ? cap : min(y0 - 1 - above, cap);                      // the counter at row y0 - 1
    for (int y = y0; y < y1; ++y) {
        const size_t i = (size_t)y * W + x;
        c = mb[i] ? 0 : min(c + 1, cap);
        g[i] = (uint8_t)c;
    }
    c = below < 0 ? cap : min(below - y1, cap);                              // the counter at row y1, coming up
    for (int y = y1 - 1; y >= y0; --y) {
        const size_t i = (size_t)y * W + x;
        const int down = g[i];
        c = down == 0 ? 0 : min(c + 1, cap);
        if (c < down) g[i] = (uint8_t)c;
    }
}

// pass 2 of the distance, the hot one: dist(x, y) = min over |dx| <= radius of dx^2 + g(x + dx, y)^2 over the entries
// with g <= radius; above radius^2 (or no such entry): SEG_FAR.  A block stages the squares of its (64 + 2 radius) x 4
// window once, 16 bits each (254^2 < 65535), SEG_FAR for g > radius and for columns outside the frame; rows are
// SEG_WIN * 2 bytes apart and a wave's 64 neighbours read 64 consecutive halfwords: 32 dwords, no bank conflict.  A
// thread walks outwards from its own column and stops once dx^2 reaches its best, which no further candidate can beat.
// Every thread of the block, the ones outside the frame included, reaches the barrier: the only return lies behind it.
// grid = (ceil(W/64), ceil(H/4)), block = (64,4)
__global__ __launch_bounds__(256) void k_seg_rows(const uint8_t* __restrict__ g, uint16_t* __restrict__ dist, int radius, int W,
                                                  int H)
{
    __shared__ uint16_t sq[4 * SEG_WIN];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int tw = 64 + 2 * radius;
    const int gx0 = (int)blockIdx.x * 64 - radius, gy = (int)blockIdx.y * 4 + ty;
    for (int col = tx; col < tw; col += 64) {
        const int gx = gx0 + col;
        unsigned v = SEG_FAR;
        if (gx >= 0 && gx < W && gy < H) {
            const unsigned d = g[(size_t)gy * W + gx];
            if (d <= (unsigned)radius) v = d * d;
        }
        sq[ty * SEG_WIN + col] = (uint16_t)v;
    }
    __syncthreads();
    const int x = gx0 + radius + tx;
    if (x >= W || gy >= H) return;
    const uint16_t* row = sq + ty * SEG_WIN + radius + tx;
    unsigned best = row[0];
    for (int d = 1; d <= radius; ++d) {
        const unsigned dd = (unsigned)(d * d);
        if (dd >= best) break;
        best = min(best, dd + min((unsigned)row[d], (unsigned)row[-d]));
    }
    dist[(size_t)gy * W + x] = (uint16_t)(best <= (unsigned)(radius * radius) ? best : SEG_FAR);
}

}  // namespace arap
