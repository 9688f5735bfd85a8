// arap_mid.h -- in-between frames from the constraint ramp: the flow between two deformation states, in the domain of
// the earlier one (gfx950).
//
// Definitions: DESIGN.md "In-between frames".  k_warp_step takes the same WarpJob array as k_warp_raster /
// k_warp_resolve (arap_warp.h) and runs only for jobs that carry a second field; without one it is not launched.
// No atomics; every output is a function of the inputs alone.
//
// Order on the stream:  k_warp_raster -> k_warp_step -> k_warp_resolve (which clears the keys k_warp_step reads).
#pragma once
#include "arap_warp.h"

namespace arap {

// position of vertex (x, y) in the job's second field (state b), by warp_pos's expression
__device__ __forceinline__ float2 warp_pos_b(const WarpJob& j, int x, int y, int i)
{
    if (j.field_b) return j.field_b[i];
    const float2 f = j.flow_b[i];
    return make_float2((float)x + f.x, (float)y + f.y);
}

// d(q) of a covered pixel q = (qx, qy) whose winner under the job's first field a is triangle t: the point of state b
// interpolated at q with the rasteriser's barycentrics of a(c0), a(c1), a(c2).  The one copy: tri_transfer and the
// layered step pass (arap_layers_step.h) call it.  False, and d untouched, where the rasteriser's test fails at q
// (never: it passed there)
__device__ __forceinline__ bool tri_transfer_point(const WarpJob& j, int W, unsigned t, int qx, int qy, float2& d)
{
    const TriCorners c = tri_corners(t, W);
    float b0, b1, b2;
    if (!tri_bary_at(j, c, (float)qx, (float)qy, b0, b1, b2)) return false;
    const float2 d0 = warp_pos_b(j, c.x[0], c.y[0], c.i[0]), d1 = warp_pos_b(j, c.x[1], c.y[1], c.i[1]);
    const float2 d2 = warp_pos_b(j, c.x[2], c.y[2], c.i[2]);
    d.x = bary_mix(d0.x, d1.x, d2.x, b0, b1, b2);
    d.y = bary_mix(d0.y, d1.y, d2.y, b0, b1, b2);
    return true;
}

// the step from pixel q to the point d: the one statement of the subtraction (tri_transfer, k_lstep_step)
__device__ __forceinline__ float2 step_of(float2 d, int qx, int qy)
{
    return make_float2(d.x - (float)qx, d.y - (float)qy);
}

// step(q) = d(q) - q.  With b = the pixel grid this is tri_backward's B(q) (arap_occ.h), expression for expression.
__device__ __forceinline__ float2 tri_transfer(const WarpJob& j, int W, unsigned t, int qx, int qy)
{
    float2 d;
    if (!tri_transfer_point(j, W, t, qx, qy, d)) return make_float2(0.f, 0.f);
    return step_of(d, qx, qy);
}

// Per pixel q of the in-between frame (the warp of field a): step(q) towards state b, (0, 0) where nothing is drawn
// (the background is static).  Before k_warp_resolve; jobs without a `step` pointer are passed over.
// grid = (ceil(N/256), 1, njobs), block = 256
__global__ __launch_bounds__(256) void k_warp_step(const WarpJob* jobs, int W, int N)
{
    const WarpJob j = jobs[blockIdx.z];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N || !j.step) return;
    const unsigned long long k = j.key[i];
    const int qy = i / W, qx = i - qy * W;
    j.step[i] = k ? tri_transfer(j, W, key_winner(k).tri, qx, qy) : make_float2(0.f, 0.f);
}

}  // namespace arap
