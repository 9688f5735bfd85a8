// arap_layers.h -- one layered rasteriser pass over all segments of a frame (gfx950).
//
// Definitions: DESIGN.md "Layered warp".  A frame has n layers (the --multseg segments in list order); layer l has its
// own mask and its own flow, all layers share the frame's RGB, and the higher index is on top.  All layers rasterise
// into ONE key image, 64-bit atomicMax on
//     (l + 1) << 56 | (t + 1) << 24 | r << 16 | g << 8 | b
// so the winner of a frame-2 pixel is the lexicographically largest (layer, triangle) that covers it: what
// pipeline.merge_segments / merge_backward make of n separate warps, without the n warps.  New against n separate
// warps is the forward occlusion ACROSS layers: the owned vertices of every layer are binned once into one joint cell
// array (one count, one scan, one scatter for the frame, however many layers) and every rasterised triangle of every
// layer tests the vertices in the cells it visits with the rule  l' > l || (l' == l && t > m(v)).
//
// The inside test, the cell loop, the colour, the backward source point, m(v) and the scan are the single-layer ones
// (tri_bary, tri_cells, tri_rgb, tri_backward, own_max_tri, k_occ_scan): a layer is looked at through a WarpJob whose
// mask / flow_in point at that layer.  Integer atomics only; every output is a function of the inputs alone.
//
// Order on the stream:  k_layers_raster -> k_layers_keys -> [k_layers_count -> k_occ_scan -> k_layers_scatter ->
//                       k_layers_tri] -> k_layers_resolve (which clears the keys).
// Limits: n <= 255 (8 bits of layer + 1), 2N < 2^32 (32 bits of triangle + 1), and N <= 2^24 when the forward occlusion
// is asked for (a binned vertex carries v | l << 24).
#pragma once
#include "arap_occ.h"

namespace arap {

struct LayerSet {                   // the per-layer inputs of one frame; everything shared sits in a WarpJob
    const uint8_t* masks;           // [n][N]  0 = object
    const float2* flows;            // [n][N]
    uint8_t* owner;                 // [N] scratch: owner(v), LAYER_NONE if none (written by k_layers_count)
    int n;
};

constexpr unsigned LAYER_NONE = 255u;

// the shared job seen as layer l
__device__ __forceinline__ WarpJob layer_view(const WarpJob& j, const LayerSet& s, int l, int N)
{
    WarpJob v = j;
    v.field = nullptr;
    v.mask = s.masks + (size_t)l * N;
    v.flow_in = s.flows + (size_t)l * N;
    return v;
}

// owner(v): the largest l with mask_l[v] == 0, or LAYER_NONE
__device__ __forceinline__ unsigned layer_owner(const LayerSet& s, int N, int i)
{
    for (int l = s.n - 1; l >= 0; --l)
        if (s.masks[(size_t)l * N + i] == 0) return (unsigned)l;
    return LAYER_NONE;
}

__device__ __forceinline__ void layer_raster_tri(const WarpJob& j, int W, int H, unsigned layer, unsigned tri, float2 p0,
                                                 float2 p1, float2 p2, const float c0[3], const float c1[3],
                                                 const float c2[3])
{
    int xa, ya;
    float maxx, maxy;
    if (!tri_cells(W, H, p0, p1, p2, xa, ya, maxx, maxy)) return;
    const unsigned long long hi = ((unsigned long long)(layer + 1u) << 56) | ((unsigned long long)(tri + 1u) << 24);
    for (int x = xa; x < W && (float)x <= maxx; ++x)
        for (int y = ya; y < H && (float)y <= maxy; ++y) {
            float b0, b1, b2;
            if (!tri_bary(p0, p1, p2, (float)x, (float)y, b0, b1, b2)) continue;
            const unsigned rgbv = j.rgb ? tri_rgb(c0, c1, c2, b0, b1, b2) : 0u;
            atomicMax(j.key + (x + (size_t)W * y), hi | rgbv);
        }
}

// pass 1: k_warp_raster of layer blockIdx.z into the shared key image
// grid = (ceil(W/64), ceil(H/4), n), block = (64,4)
__global__ __launch_bounds__(256) void k_layers_raster(const WarpJob* job, LayerSet s, int W, int H)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x + 1 >= W || y + 1 >= H) return;
    const WarpJob j = layer_view(*job, s, blockIdx.z, W * H);
    if (!quad_on(j.mask, W, H, x, y)) return;
    const int i = x + W * y, i01 = i + 1, i10 = i + W, i11 = i + W + 1;
    const float2 p00 = warp_pos(j, x, y, i), p01 = warp_pos(j, x + 1, y, i01);
    const float2 p10 = warp_pos(j, x, y + 1, i10), p11 = warp_pos(j, x + 1, y + 1, i11);
    float v00[3] = {0, 0, 0}, v01[3] = {0, 0, 0}, v10[3] = {0, 0, 0}, v11[3] = {0, 0, 0};
    if (j.rgb) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            v00[k] = (float)j.rgb[3 * (size_t)i + k];
            v01[k] = (float)j.rgb[3 * (size_t)i01 + k];
            v10[k] = (float)j.rgb[3 * (size_t)i10 + k];
            v11[k] = (float)j.rgb[3 * (size_t)i11 + k];
        }
    }
    layer_raster_tri(j, W, H, blockIdx.z, 2u * (unsigned)i, p00, p01, p10, v00, v01, v10);
    layer_raster_tri(j, W, H, blockIdx.z, 2u * (unsigned)i + 1u, p10, p01, p11, v10, v01, v11);
}

// pass 2, per frame-2 pixel q: the winner (layer, triangle) from the key; B(q) with the winner's layer; OccBwd(q) =
// uncovered and owned; forward occlusion of a pixel without owner = covered.  Each output only if its pointer is set.
// grid = (ceil(N/256)), block = 256
__global__ __launch_bounds__(256) void k_layers_keys(const WarpJob* job, LayerSet s, int W, int N)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const WarpJob j = *job;
    const unsigned long long k = j.key[i];
    if (j.occ || j.occ_bwd) {
        const bool owned = layer_owner(s, N, i) != LAYER_NONE;
        if (j.occ && !owned) j.occ[i] = k ? 255 : 0;
        if (j.occ_bwd) j.occ_bwd[i] = (!k && owned) ? 255 : 0;
    }
    if (!j.bwd) return;
    float2 b = make_float2(0.f, 0.f);
    if (k) {
        const int qy = i / W, qx = i - qy * W;
        b = tri_backward(layer_view(j, s, (int)(k >> 56) - 1, N), W, (unsigned)(k >> 24) - 1u, qx, qy);
    }
    j.bwd[i] = b;
}

// pass 3, per frame-1 pixel v: owner(v); an owned vertex with P_l(v) out of frame -> Occ = 255, else Occ = 0 and one
// count in the JOINT cell (floor P.x, floor P.y); the returned old count is v's rank in the cell (k_occ_count)
// grid = (ceil(N/256)), block = 256
__global__ __launch_bounds__(256) void k_layers_count(const WarpJob* job, LayerSet s, int W, int H, int N)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const unsigned l = layer_owner(s, N, i);
    s.owner[i] = (uint8_t)l;
    if (l == LAYER_NONE) return;
    const WarpJob j = layer_view(*job, s, (int)l, N);
    const int y = i / W, x = i - y * W;
    const float2 P = warp_pos(j, x, y, i);
    const bool in = in_frame(P, W, H);
    j.occ[i] = in ? 0 : 255;
    if (!in) return;
    const int c = (int)floorf(P.x) + W * (int)floorf(P.y);
    j.rank[i] = atomicAdd(j.cell + c, 1u);
}

// pass 4 (after k_occ_scan on the joint counts): bin[start(cell) + rank] = {P.x, P.y, v | l << 24, m(v) in layer l}
// grid = (ceil(N/256)), block = 256
__global__ __launch_bounds__(256) void k_layers_scatter(const WarpJob* job, LayerSet s, int W, int H, int N)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const unsigned l = s.owner[i];
    if (l == LAYER_NONE) return;
    const WarpJob j = layer_view(*job, s, (int)l, N);
    const int y = i / W, x = i - y * W;
    const float2 P = warp_pos(j, x, y, i);
    if (!in_frame(P, W, H)) return;
    const int c = (int)floorf(P.x) + W * (int)floorf(P.y);
    j.bin[j.cell[c] + j.rank[i]] = make_int4(__float_as_int(P.x), __float_as_int(P.y), (int)((unsigned)i | (l << 24)),
                                             own_max_tri(j.mask, W, H, x, y));
}

__device__ __forceinline__ void layer_occ_tri(const WarpJob& j, int W, int H, unsigned layer, int tri, float2 p0,
                                              float2 p1, float2 p2)
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
                const unsigned l = (unsigned)v.z >> 24;
                if (!(layer > l || (layer == l && tri > v.w))) continue;      // a lower layer, or v's own / an earlier triangle
                float b0, b1, b2;
                if (tri_bary(p0, p1, p2, __int_as_float(v.x), __int_as_float(v.y), b0, b1, b2))
                    j.occ[(unsigned)v.z & 0xffffffu] = 255;
            }
        }
}

// pass 5: every rasterised triangle of layer blockIdx.z tests the vertices of ALL layers binned in the cells
// raster_tri visits for it.  Only ever writes 255.
// grid = (ceil(W/64), ceil(H/4), n), block = (64,4)
__global__ __launch_bounds__(256) void k_layers_tri(const WarpJob* job, LayerSet s, int W, int H)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x + 1 >= W || y + 1 >= H) return;
    const WarpJob j = layer_view(*job, s, blockIdx.z, W * H);
    if (!quad_on(j.mask, W, H, x, y)) return;
    const int i = x + W * y;
    const float2 p00 = warp_pos(j, x, y, i), p01 = warp_pos(j, x + 1, y, i + 1);
    const float2 p10 = warp_pos(j, x, y + 1, i + W), p11 = warp_pos(j, x + 1, y + 1, i + W + 1);
    layer_occ_tri(j, W, H, blockIdx.z, 2 * i, p00, p01, p10);
    layer_occ_tri(j, W, H, blockIdx.z, 2 * i + 1, p10, p01, p11);
}

// pass 6: unpack the composite RGB and mask, clear the keys
// grid = (ceil(N/256)), block = 256
__global__ __launch_bounds__(256) void k_layers_resolve(const WarpJob* job, int N)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const WarpJob j = *job;
    const unsigned long long k = j.key[i];
    j.key[i] = 0ull;
    if (j.out_rgb) {
        j.out_rgb[3 * (size_t)i + 0] = (uint8_t)((k >> 16) & 0xffu);
        j.out_rgb[3 * (size_t)i + 1] = (uint8_t)((k >> 8) & 0xffu);
        j.out_rgb[3 * (size_t)i + 2] = (uint8_t)(k & 0xffu);
    }
    if (j.out_mask) j.out_mask[i] = k ? 255 : 0;
}

}  // namespace arap
