// arap_occ.h -- backward flow and occlusion maps from the warp rasteriser (gfx950).
//
// Definitions: DESIGN.md "Backward flow and occlusion".  All kernels take the same WarpJob array as k_warp_raster /
// k_warp_resolve (arap_warp.h) and only run when a caller asked for the outputs; with the outputs off none of them is
// launched.  Integer atomics only (a count per cell); every output is a function of the inputs alone.
//
// Order on the stream:  k_warp_raster -> k_warp_keys -> [k_occ_count -> k_occ_scan -> k_occ_scatter -> k_occ_tri]
//                       -> k_warp_resolve (which clears the keys k_warp_keys reads).
// Limits: N < 2^31 (a binned vertex carries its index in a full int); the layered query (arap_layers.h) packs
// v | l << 24 into the same field and so has N <= 2^24.  Both packings and both "does this triangle test this point"
// rules are stated once here, in bin_payload / bin_index / bin_tested.
#pragma once
#include "arap_warp.h"

namespace arap {

// m(v): the largest index of a rasterised triangle with vertex (x, y) as a corner, or -1.  The vertex is p00 of quad
// (x,y) (triangle 2u only), p01 of quad (x-1,y) and p10 of quad (x,y-1) (both triangles), p11 of quad (x-1,y-1)
// (triangle 2u+1 only): in decreasing order of the largest index
__device__ __forceinline__ int own_max_tri(const uint8_t* mask, int W, int H, int x, int y)
{
    const int u = x + W * y;
    if (quad_on(mask, W, H, x, y)) return 2 * u;
    if (quad_on(mask, W, H, x - 1, y)) return 2 * (u - 1) + 1;
    if (quad_on(mask, W, H, x, y - 1)) return 2 * (u - W) + 1;
    if (quad_on(mask, W, H, x - 1, y - 1)) return 2 * (u - W - 1) + 1;
    return -1;
}

__device__ __forceinline__ bool in_frame(float2 P, int W, int H)
{
    return P.x >= 0.f && P.x <= (float)(W - 1) && P.y >= 0.f && P.y <= (float)(H - 1);     // false on NaN
}

// tri_bary of the triangle with corners c, placed by the job's (first) field, at the point (sx, sy)
__device__ __forceinline__ bool tri_bary_at(const WarpJob& j, const TriCorners& c, float sx, float sy, float& b0, float& b1,
                                            float& b2)
{
    const float2 p0 = warp_pos(j, c.x[0], c.y[0], c.i[0]), p1 = warp_pos(j, c.x[1], c.y[1], c.i[1]);
    const float2 p2 = warp_pos(j, c.x[2], c.y[2], c.i[2]);
    return tri_bary(p0, p1, p2, sx, sy, b0, b1, b2);
}

// B(q) of a covered pixel q = (qx, qy) whose winner is triangle t of job j: s - q with s the source point interpolated
// at q with the rasteriser's barycentrics.  The one copy: k_warp_keys and the layered key pass (arap_layers.h) call it.
__device__ __forceinline__ float2 tri_backward(const WarpJob& j, int W, unsigned t, int qx, int qy)
{
    const TriCorners c = tri_corners(t, W);
    const float sx = (float)qx, sy = (float)qy;
    float b0, b1, b2;
    if (!tri_bary_at(j, c, sx, sy, b0, b1, b2)) return make_float2(0.f, 0.f);       // (never: the raster passed this test at q)
    const float srcx = bary_mix((float)c.x[0], (float)c.x[1], (float)c.x[2], b0, b1, b2);
    const float srcy = bary_mix((float)c.y[0], (float)c.y[1], (float)c.y[2], b0, b1, b2);
    return make_float2(srcx - sx, srcy - sy);
}

// Backward pass, before k_warp_resolve.  Per frame-2 pixel q: the winner T(q) = key's triangle; B(q) = s - q with s
// the source point interpolated at q with the rasteriser's barycentrics; OccBwd(q) = uncovered object pixel; and the
// forward occlusion of a background pixel = covered.  Each output only if its pointer is set.
// grid = (ceil(N/256), 1, njobs), block = 256
__global__ __launch_bounds__(256) void k_warp_keys(const WarpJob* jobs, int W, int N)
{
    const WarpJob j = jobs[blockIdx.z];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const unsigned long long k = j.key[i];
    const int qy = i / W, qx = i - qy * W;
    if (j.occ && j.mask[i] != 0) j.occ[i] = k ? 255 : 0;
    if (j.occ_bwd) j.occ_bwd[i] = (!k && j.mask[i] == 0) ? 255 : 0;
    if (!j.bwd) return;
    j.bwd[i] = k ? tri_backward(j, W, key_winner(k).tri, qx, qy) : make_float2(0.f, 0.f);
}

// the cell of an in-frame point
__device__ __forceinline__ int occ_cell(float2 P, int W) { return (int)floorf(P.x) + W * (int)floorf(P.y); }

// The count tail of every query, for point i at P: out of frame -> Occ = 255; else Occ = 0 and one count in the cell
// of P.  The returned old count is the point's rank in the cell, so the scatter needs no atomics.  (Under a smooth warp
// a cell holds about one point: the counts hardly collide, and the compiler's per-wave aggregation of same-address
// atomics has nothing to merge.)
__device__ __forceinline__ void occ_count_point(const WarpJob& j, int i, float2 P, int W, int H)
{
    const bool in = in_frame(P, W, H);
    j.occ[i] = in ? 0 : 255;
    if (!in) return;
    j.rank[i] = atomicAdd(j.cell + occ_cell(P, W), 1u);
}

// The scatter tail, after the scan: a counted point to its slot, bin[start(cell) + rank] = {P.x, P.y, payload, m}
__device__ __forceinline__ void occ_bin_point(const WarpJob& j, int i, float2 P, int W, int H, int payload, int m)
{
    if (!in_frame(P, W, H)) return;
    j.bin[j.cell[occ_cell(P, W)] + j.rank[i]] = make_int4(__float_as_int(P.x), __float_as_int(P.y), payload, m);
}

// The payload of a binned point: its index i, full width (N < 2^31) -- or, LAYERED, i | l << 24 with l its layer
// (N <= 2^24).  bin_index reads the index back; bin_tested is the rule by which triangle `tri` of layer `layer` tests
// the point v = {P.x, P.y, payload, m}:  tri > m  (not one of the point's own triangles, nor an earlier one) -- or,
// LAYERED,  layer > l || (layer == l && tri > m).
template <bool LAYERED>
__device__ __forceinline__ int bin_payload(int i, unsigned l)
{
    return LAYERED ? (int)((unsigned)i | (l << 24)) : i;
}

template <bool LAYERED>
__device__ __forceinline__ int bin_index(int4 v)
{
    return LAYERED ? v.z & 0xffffff : v.z;
}

template <bool LAYERED>
__device__ __forceinline__ bool bin_tested(int4 v, unsigned layer, int tri)
{
    if (!LAYERED) return tri > v.w;
    const unsigned l = (unsigned)v.z >> 24;
    return layer > l || (layer == l && tri > v.w);
}

// Forward occlusion, pass 1: every object vertex v at P(v) through the count tail
// grid = (ceil(N/256), 1, njobs), block = 256
__global__ __launch_bounds__(256) void k_occ_count(const WarpJob* jobs, int W, int H, int N)
{
    const WarpJob j = jobs[blockIdx.z];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N || j.mask[i] != 0) return;
    const int y = i / W, x = i - y * W;
    occ_count_point(j, i, warp_pos(j, x, y, i), W, H);
}

// pass 2: exclusive scan of the N cell counts in place (cell[N] = total).  One workgroup per frame walks the frame in
// chunks of 4096 counts: 4 per lane (one 16-byte load), wave scan by shuffles, wave totals through LDS.
// grid = (1, 1, njobs), block = 1024
__global__ __launch_bounds__(1024) void k_occ_scan(const WarpJob* jobs, int N)
{
    const WarpJob j = jobs[blockIdx.z];
    unsigned* cnt = j.cell;
    __shared__ unsigned wsum[2][16];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    unsigned carry = 0;
    int par = 0;
    for (int base = 0; base < N; base += 4096, par ^= 1) {
        const int i0 = base + 4 * (int)threadIdx.x;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (i0 + 3 < N) v = *(const uint4*)(cnt + i0);      // (cell is 256-byte aligned, i0 % 4 == 0)
        else {
            if (i0 < N) v.x = cnt[i0];
            if (i0 + 1 < N) v.y = cnt[i0 + 1];
            if (i0 + 2 < N) v.z = cnt[i0 + 2];
        }
        const unsigned s = (v.x + v.y) + (v.z + v.w);
        unsigned inc = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        if (lane == 63) wsum[par][wid] = inc;
        __syncthreads();                        // (double-buffered wsum: one barrier per chunk)
        unsigned pre = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const unsigned t = wsum[par][w];
            pre += w < wid ? t : 0u;
            tot += t;
        }
        unsigned e = carry + pre + (inc - s);
        uint4 o4;
        o4.x = e; e += v.x;
        o4.y = e; e += v.y;
        o4.z = e; e += v.z;
        o4.w = e;
        if (i0 + 3 < N) *(uint4*)(cnt + i0) = o4;
        else {
            if (i0 < N) cnt[i0] = o4.x;
            if (i0 + 1 < N) cnt[i0 + 1] = o4.y;
            if (i0 + 2 < N) cnt[i0 + 2] = o4.z;
        }
        carry += tot;
    }
    if (threadIdx.x == 0) cnt[N] = carry;
}

// pass 3: every counted vertex to its slot: bin[start(cell) + rank] = {P.x, P.y, v, m(v)}
// grid = (ceil(N/256), 1, njobs), block = 256
__global__ __launch_bounds__(256) void k_occ_scatter(const WarpJob* jobs, int W, int H, int N)
{
    const WarpJob j = jobs[blockIdx.z];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N || j.mask[i] != 0) return;
    const int y = i / W, x = i - y * W;
    occ_bin_point(j, i, warp_pos(j, x, y, i), W, H, bin_payload<false>(i, 0u), own_max_tri(j.mask, W, H, x, y));
}

// The querying triangle walk: triangle `tri` of layer `layer` tests, by bin_tested, the points binned in the cells
// raster_tri visits for it, and flags those at which the rasteriser would show it
template <bool LAYERED>
__device__ __forceinline__ void occ_tri(const WarpJob& j, int W, int H, unsigned layer, int tri, float2 p0, float2 p1,
                                        float2 p2)
{
    int xa, ya;
    float maxx, maxy;
    if (!tri_cells(W, H, p0, p1, p2, xa, ya, maxx, maxy)) return;
    for (int x = xa; x < W && (float)x <= maxx; ++x)
        for (int y = ya; y < H && (float)y <= maxy; ++y) {
            const int c = x + W * y;
            const unsigned e = j.cell[c + 1];
            for (unsigned k = j.cell[c]; k < e; ++k) {
                const int4 v = j.bin[k];
                if (!bin_tested<LAYERED>(v, layer, tri)) continue;
                float b0, b1, b2;
                if (tri_bary(p0, p1, p2, __int_as_float(v.x), __int_as_float(v.y), b0, b1, b2))
                    j.occ[bin_index<LAYERED>(v)] = 255;
            }
        }
}

// warp_quad with occ_tri as the action, for the job seen as layer `layer`
template <bool LAYERED>
__device__ __forceinline__ void occ_quad(const WarpJob& j, int W, int H, int x, int y, unsigned layer)
{
    warp_quad<false>(j, W, H, x, y, [&](unsigned t, float2 p0, float2 p1, float2 p2, const float*, const float*,
                                        const float*) { occ_tri<LAYERED>(j, W, H, layer, (int)t, p0, p1, p2); });
}

// pass 4: every rasterised triangle t tests the vertices binned in the cells raster_tri visits for t: a later
// triangle that is not one of v's own and that the rasteriser would show at P(v) occludes v.  Only ever writes 255.
// grid = (ceil(W/64), ceil(H/4), njobs), block = (64,4)
__global__ __launch_bounds__(256) void k_occ_tri(const WarpJob* jobs, int W, int H)
{
    const WarpJob j = jobs[blockIdx.z];
    occ_quad<false>(j, W, H, blockIdx.x * 64 + threadIdx.x, blockIdx.y * 4 + threadIdx.y, 0u);
}

}  // namespace arap
