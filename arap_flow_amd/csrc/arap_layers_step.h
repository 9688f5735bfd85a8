// arap_layers_step.h -- layered in-between frames: the layered warp of a state a of all segments, the flow from that
// composite to a second state b, and the forward occlusion of that link in the composite's own pixel domain (gfx950).
//
// Definitions: DESIGN.md "Layered in-between frames".  Every layer l has two states, given as flows a_l and b_l.  The
// composite of state a is the layered warp's (k_layers_raster with the flows of a, k_warp_resolve).  New here:
//   step(q)     of a covered pixel: tri_transfer on the winner's layer, d(q) - q; (0, 0) where nothing is drawn;
//   OccStep(q)  is what q shows hidden in the next frame?  Every pixel q is one query point
//                   {d.x, d.y, q | l << 24, M(t)}       M(t) = max of own_max_tri over the corners of the winner t
//               -- an uncovered pixel asks from below every layer at d = q: {q, q | 0 << 24, -1} -- binned by the
//               cell of d into the joint cell array of the layered query.  Then k_layers_tri, unchanged, walks every
//               rasterised triangle of every layer PLACED BY b with its rule  l' > l || (l' == l && t' > M): the
//               layered query with pixels in the place of vertices.  A covered point that leaves the frame (or is
//               NaN) is flagged directly.
//
// The quad body, d(q), the subtraction, m(v), the corner numbering, the count and scatter tails, the scan and the key
// are the existing ones (raster_quad, occ_quad, tri_transfer_point, step_of, own_max_tri, tri_corners, occ_count_point,
// occ_bin_point, k_occ_scan, warp_key / key_winner, bin_payload): no float expression is stated here.  Integer atomics
// only (one count per query point); every output is a function of the inputs alone.
//
// Order on the stream:  k_layers_raster(a) -> [k_lstep_step -> [k_occ_scan -> k_lstep_scatter -> k_layers_tri(b)]]
//                       -> k_warp_resolve with the one shared job (which clears the keys).
// Scratch per pixel: 8 (key) and, for OccStep, 4 (cell) + 4 (rank) + 16 (query point) + 16 (bin) = 48 bytes.
// Limits: those of arap_layers.h (n <= 255, N < 2^31, N <= 2^24 with OccStep: a query point carries q | l << 24).
// Worst case: as the layered query's -- flows that collapse many points into few cells grow k_layers_tri's work up to
// quadratically.
#pragma once
#include "arap_layers.h"
#include "arap_mid.h"

namespace arap {

// layer l seen with both of its states: flow_in = a_l (the LayerSet's), flow_b = b_l
__device__ __forceinline__ WarpJob layer_view_ab(const WarpJob& j, const LayerSet& s, const float2* flows_b, int l,
                                                 int N)
{
    WarpJob v = layer_view(j, s, l, N);
    v.field_b = nullptr;
    v.flow_b = flows_b + (size_t)l * N;
    return v;
}

// M(t): the largest own_max_tri over the three corners of triangle t
__device__ __forceinline__ int tri_ring_max(const uint8_t* mask, int W, int H, unsigned t)
{
    const TriCorners c = tri_corners(t, W);
    const int m0 = own_max_tri(mask, W, H, c.x[0], c.y[0]), m1 = own_max_tri(mask, W, H, c.x[1], c.y[1]);
    return max(m0, max(m1, own_max_tri(mask, W, H, c.x[2], c.y[2])));
}

// pass 2, per pixel q of the composite of state a: the winner (l, t) from the key, step(q), and -- when OccStep is
// asked (j.occ) -- q's query point into `pts` and through the count tail into the joint cells.  Were the rasteriser's
// test to fail at a covered q (it cannot: the key says it passed there), tri_transfer_point leaves d = q, so step(q) is
// (0, 0) as tri_transfer's and the point asks at q as the winner (l, M(t))
// grid = (ceil(N/256)), block = 256
__global__ __launch_bounds__(256) void k_lstep_step(const WarpJob* job, LayerSet s, const float2* flows_b, int4* pts,
                                                    int W, int H, int N)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const WarpJob j = *job;
    const unsigned long long k = j.key[i];
    const int qy = i / W, qx = i - qy * W;
    float2 d = make_float2((float)qx, (float)qy);
    unsigned l = 0;
    int m = -1;                                  // (layer 0, M = -1: below every triangle of every layer)
    bool ok = false;
    const KeyWinner w = key_winner(k);
    if (w.covered) {
        l = w.layer;
        const WarpJob v = layer_view_ab(j, s, flows_b, (int)l, N);
        ok = tri_transfer_point(v, W, w.tri, qx, qy, d);
        if (j.occ) m = tri_ring_max(v.mask, W, H, w.tri);
    }
    if (j.step) j.step[i] = ok ? step_of(d, qx, qy) : make_float2(0.f, 0.f);
    if (!j.occ) return;
    pts[i] = make_int4(__float_as_int(d.x), __float_as_int(d.y), bin_payload<true>(i, l), m);
    occ_count_point(j, i, d, W, H);
}

// pass 4 (after k_occ_scan on the joint counts): bin[start(cell) + rank] = the query point
// grid = (ceil(N/256)), block = 256
__global__ __launch_bounds__(256) void k_lstep_scatter(const WarpJob* job, const int4* pts, int W, int H, int N)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const WarpJob j = *job;
    const int4 p = pts[i];
    occ_bin_point(j, i, make_float2(__int_as_float(p.x), __int_as_float(p.y)), W, H, p.z, p.w);
}

}  // namespace arap
