// arap_track.h -- point tracks through a sequence: where a caller-given sub-pixel point of frame 1 is in every state of
// every layer, and whether it can be seen there (gfx950).
//
// Definitions: DESIGN.md "Point tracks".  A frame has n layers (arap_layers.h) and T states; state s of layer l is the
// flow flows[s][l].  Every query point p of frame 1 has an owner (l, t): the lexicographically largest (layer,
// triangle) among the rasterised triangles of the four quads around p that pass the rasteriser's test at p with their
// corners on the grid -- for an integer p the winner of a zero-flow layered warp at that pixel.  In state s the point is
//     d = bary_mix of the owner's corners placed by state s, with the barycentrics found on the grid
// and it is one query point of the layered step query (arap_layers_step.h)
//     {d.x, d.y, k | l << 24, M(t)}       M(t) = tri_ring_max of the owner
// -- a point without owner stays at p and asks from below every layer: {p, k | 0 << 24, -1}; a point outside the frame
// (or NaN) is never located, stays at p and is flagged by the count tail -- binned by the cell of d into state s's own
// cell array.  Then every rasterised triangle of every layer placed by state s tests the points in the cells it visits
// with the layered rule  l' > l || (l' == l && t' > M).
//
// The inside test, the mix, the corner numbering, quad_on, M(t), in_frame, warp_pos, the count and scatter tails, the
// payload, the scan and the querying triangle walk are the existing ones (tri_bary, bary_mix, tri_corners,
// tri_ring_max, occ_count_point, occ_bin_point, bin_payload<true>, k_occ_scan, occ_quad<true>): no float expression is
// stated here.  Integer atomics only (one count per query point and state); every output is a function of the inputs
// alone.  No key image is touched.
//
// Order on the stream:  clear the T cell arrays -> k_track_locate -> k_track_state -> k_occ_scan (all states) ->
//                       k_track_scatter -> k_track_tri.
// Scratch: per state 4 (N + 1) (cell) and per point 4 (rank) + 16 (bin) + 16 (query point) + 1 (flag, used when the
// caller wants no occ); per point 32 (owner), once.
// Limits: n <= 255, N < 2^31, 1 <= P <= 2^24 (a query point carries k | l << 24), 1 <= T <= ARAPFLOW_MAX_SNAPSHOTS + 1.
// P may exceed N: rank, query points and bins are sized by P, the cells by N.
// Worst case: as the layered query's -- many points in few cells (a caller may put all P at one spot) grow k_track_tri's
// work up to P per visited cell.
#pragma once
#include "arap_layers_step.h"

namespace arap {

constexpr int TRACK_BACKGROUND = -1;

struct TrackOwner {                 // what k_track_locate knows of one query point
    float b0, b1, b2;               // the owner's barycentrics at p
    int layer;                      // TRACK_BACKGROUND: no owner (or p outside the frame)
    unsigned tri;
    int m;                          // M(t) on the owner's layer
    int pad[2];
};

struct TrackSet {                   // the inputs and outputs all states share; a state's scratch sits in its WarpJob
    const uint8_t* masks;           // [n][N]  0 = object
    const float2* flows;            // [T][n][N]
    const float2* points;           // [P]
    float2* pos;                    // [T][P] or NULL
    TrackOwner* own;                // [P] scratch
    int4* pts;                      // [T][P] scratch: the query points
    int n, P;
};

// the layers placed by state s
__device__ __forceinline__ LayerSet track_layers(const TrackSet& ts, int s, int N)
{
    LayerSet ls;
    ls.masks = ts.masks;
    ls.flows = ts.flows + (size_t)s * ts.n * N;
    ls.owner = nullptr;
    ls.n = ts.n;
    return ls;
}

// triangle t of a layer at p with its corners on the grid: the rasteriser's test and barycentrics
__device__ __forceinline__ bool track_tri_at(int W, unsigned t, float2 p, float& b0, float& b1, float& b2)
{
    const TriCorners c = tri_corners(t, W);
    return tri_bary(make_float2((float)c.x[0], (float)c.y[0]), make_float2((float)c.x[1], (float)c.y[1]),
                    make_float2((float)c.x[2], (float)c.y[2]), p.x, p.y, b0, b1, b2);
}

// pass 1, per point, once per call: the owner among the <= 8 n candidates, in decreasing (layer, triangle) order so
// that the first to pass is the largest; its barycentrics and M
// grid = (ceil(P/256)), block = 256
__global__ __launch_bounds__(256) void k_track_locate(TrackSet ts, int W, int H)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= ts.P) return;
    const float2 p = ts.points[k];
    TrackOwner o{0.f, 0.f, 0.f, TRACK_BACKGROUND, 0u, -1, {0, 0}};
    if (in_frame(p, W, H)) {                                    // (before any floorf or cast: p may be NaN or huge)
        const int N = W * H;
        const int ix = (int)floorf(p.x), iy = (int)floorf(p.y);
        for (int l = ts.n - 1; l >= 0 && o.layer == TRACK_BACKGROUND; --l) {
            const uint8_t* mask = ts.masks + (size_t)l * N;
            for (int q = 0; q < 4 && o.layer == TRACK_BACKGROUND; ++q) {        // quads in decreasing index order
                const int qx = ix - (q & 1), qy = iy - (q >> 1);
                if (!quad_on(mask, W, H, qx, qy)) continue;
                const unsigned u = (unsigned)(qx + W * qy);
                for (int odd = 1; odd >= 0; --odd) {
                    const unsigned t = 2u * u + (unsigned)odd;
                    if (!track_tri_at(W, t, p, o.b0, o.b1, o.b2)) continue;
                    o.layer = l;
                    o.tri = t;
                    o.m = tri_ring_max(mask, W, H, t);
                    break;
                }
            }
        }
    }
    ts.own[k] = o;
}

// pass 2, per point and state s = blockIdx.z: d, pos, the query point into `pts` and through the count tail into the
// state's cells (which writes occ to 0, or to 255 when d is outside the frame)
// grid = (ceil(P/256), 1, T), block = 256
__global__ __launch_bounds__(256) void k_track_state(const WarpJob* jobs, TrackSet ts, int W, int H)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= ts.P) return;
    const int s = blockIdx.z, N = W * H;
    const WarpJob j = jobs[s];
    const TrackOwner o = ts.own[k];
    float2 d = ts.points[k];
    unsigned l = 0;                              // (layer 0, M = -1: below every triangle of every layer)
    if (o.layer != TRACK_BACKGROUND) {
        l = (unsigned)o.layer;
        const WarpJob v = layer_view(j, track_layers(ts, s, N), o.layer, N);
        const TriCorners c = tri_corners(o.tri, W);
        const float2 d0 = warp_pos(v, c.x[0], c.y[0], c.i[0]), d1 = warp_pos(v, c.x[1], c.y[1], c.i[1]);
        const float2 d2 = warp_pos(v, c.x[2], c.y[2], c.i[2]);
        d.x = bary_mix(d0.x, d1.x, d2.x, o.b0, o.b1, o.b2);
        d.y = bary_mix(d0.y, d1.y, d2.y, o.b0, o.b1, o.b2);
    }
    const size_t at = (size_t)s * ts.P + k;
    if (ts.pos) ts.pos[at] = d;
    ts.pts[at] = make_int4(__float_as_int(d.x), __float_as_int(d.y), bin_payload<true>(k, l), o.m);
    occ_count_point(j, k, d, W, H);
}

// pass 4 (after k_occ_scan on every state's counts): bin[start(cell) + rank] = the query point
// grid = (ceil(P/256), 1, T), block = 256
__global__ __launch_bounds__(256) void k_track_scatter(const WarpJob* jobs, TrackSet ts, int W, int H)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= ts.P) return;
    const WarpJob j = jobs[blockIdx.z];
    const int4 p = ts.pts[(size_t)blockIdx.z * ts.P + k];
    occ_bin_point(j, k, make_float2(__int_as_float(p.x), __int_as_float(p.y)), W, H, p.z, p.w);
}

// pass 5: k_layers_tri with the state on the grid: blockIdx.z = s n + l, every rasterised triangle of layer l placed
// by state s tests the points binned in the cells raster_tri visits for it.  Only ever writes 255.
// grid = (ceil(W/64), ceil(H/4), T n), block = (64,4)
__global__ __launch_bounds__(256) void k_track_tri(const WarpJob* jobs, TrackSet ts, int W, int H)
{
    const int s = blockIdx.z / ts.n, l = blockIdx.z - s * ts.n, N = W * H;
    occ_quad<true>(layer_view(jobs[s], track_layers(ts, s, N), l, N), W, H, blockIdx.x * 64 + threadIdx.x,
                   blockIdx.y * 4 + threadIdx.y, (unsigned)l);
}

}  // namespace arap
