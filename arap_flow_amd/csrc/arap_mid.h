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
    const int u = (int)(t >> 1);
    const int uy = u / W, ux = u - uy * W;
    // corners of triangle t and their grid coordinates: 2u = (p00, p01, p10), 2u+1 = (p10, p01, p11)
    const int odd = (int)(t & 1u);
    const int ax = ux, ay = uy + odd, bx = ux + 1, by = uy, cx = ux + odd, cy = uy + 1;
    const int i0 = ax + W * ay, i1 = bx + W * by, i2 = cx + W * cy;
    const float2 p0 = warp_pos(j, ax, ay, i0), p1 = warp_pos(j, bx, by, i1), p2 = warp_pos(j, cx, cy, i2);
    float b0, b1, b2;
    if (!tri_bary(p0, p1, p2, (float)qx, (float)qy, b0, b1, b2)) return false;
    const float2 d0 = warp_pos_b(j, ax, ay, i0), d1 = warp_pos_b(j, bx, by, i1), d2 = warp_pos_b(j, cx, cy, i2);
    d.x = (d0.x * b0 + d1.x * b1) + d2.x * b2;
    d.y = (d0.y * b0 + d1.y * b1) + d2.y * b2;
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
    j.step[i] = k ? tri_transfer(j, W, (unsigned)(k >> 32) - 1u, qx, qy) : make_float2(0.f, 0.f);
}

}  // namespace arap
