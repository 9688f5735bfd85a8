// arap_layers.h -- one layered rasteriser pass over all segments of a frame (gfx950).
//
// Definitions: DESIGN.md "Layered warp".  A frame has n layers (the --multseg segments in list order); layer l has its
// own mask and its own flow, all layers share the frame's RGB, and the higher index is on top.  All layers rasterise
// into ONE key image, 64-bit atomicMax on the family's key (warp_key, arap_warp.h) with the layer in its top bits,
// so the winner of a frame-2 pixel is the lexicographically largest (layer, triangle) that covers it: what
// pipeline.merge_segments / merge_backward make of n separate warps, without the n warps.  New against n separate
// warps is the forward occlusion ACROSS layers: the owned vertices of every layer are binned once into one joint cell
// array (one count, one scan, one scatter for the frame, however many layers) and every rasterised triangle of every
// layer tests the vertices in the cells it visits with the rule  l' > l || (l' == l && t > m(v)).
//
// The quad body with both of its actions, the key, the backward source point, m(v), the count and scatter tails, the
// scan and the resolve are the single-layer ones (raster_quad, occ_quad, warp_key / key_winner, tri_backward,
// own_max_tri, occ_count_point, occ_bin_point, k_occ_scan, k_warp_resolve): a layer is looked at through a WarpJob
// whose mask / flow_in point at that layer, and no float expression is stated here.  Integer atomics only; every output
// is a function of the inputs alone.
//
// Order on the stream:  k_layers_raster -> k_layers_keys -> [k_layers_count -> k_occ_scan -> k_layers_scatter ->
//                       k_layers_tri] -> k_warp_resolve with the one shared job (which clears the keys).
// Limits: n <= 255 (8 bits of layer + 1), 2N < 2^32 (32 bits of triangle + 1), and N <= 2^24 when the forward occlusion
// is asked for (a binned vertex carries v | l << 24: bin_payload<true>).
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

// pass 1: k_warp_raster of layer blockIdx.z into the shared key image
// grid = (ceil(W/64), ceil(H/4), n), block = (64,4)
__global__ __launch_bounds__(256) void k_layers_raster(const WarpJob* job, LayerSet s, int W, int H)
{
    raster_quad(layer_view(*job, s, blockIdx.z, W * H), W, H, blockIdx.x * 64 + threadIdx.x, blockIdx.y * 4 + threadIdx.y,
                blockIdx.z);
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
    const KeyWinner w = key_winner(k);
    if (w.covered) {
        const int qy = i / W, qx = i - qy * W;
        b = tri_backward(layer_view(j, s, (int)w.layer, N), W, w.tri, qx, qy);
    }
    j.bwd[i] = b;
}

// pass 3, per frame-1 pixel v: owner(v); an owned vertex at P_l(v) through the count tail into the JOINT cells
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
    occ_count_point(j, i, warp_pos(j, x, y, i), W, H);
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
    occ_bin_point(j, i, warp_pos(j, x, y, i), W, H, bin_payload<true>(i, l), own_max_tri(j.mask, W, H, x, y));
}

// pass 5: every rasterised triangle of layer blockIdx.z tests the vertices of ALL layers binned in the cells
// raster_tri visits for it.  Only ever writes 255.
// grid = (ceil(W/64), ceil(H/4), n), block = (64,4)
__global__ __launch_bounds__(256) void k_layers_tri(const WarpJob* job, LayerSet s, int W, int H)
{
    occ_quad<true>(layer_view(*job, s, blockIdx.z, W * H), W, H, blockIdx.x * 64 + threadIdx.x,
                   blockIdx.y * 4 + threadIdx.y, blockIdx.z);
}

// pass 6 is k_warp_resolve (arap_warp.h) on the one shared job: unpack the composite RGB and mask, clear the keys

}  // namespace arap
