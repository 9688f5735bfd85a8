// arap_warp.h -- forward triangle rasteriser + flow emission on the GPU (gfx950).
//
// Reference: ARAP/warping/src/main.cpp:69-104 (PointInTriangleLK), :110-142 (rasterizeTriangle),
// :145-225 (Warp); the same code lives in ARAP/deformation/src/CombinedSolver.h:61-97,248-342, and
// flow = Offset - grid is CombinedSolver.h:352-366.
//
// The reference rasterises quads sequentially (y outer, x inner; triangle (00,01,10) then
// (10,01,11)) and later writes overwrite earlier ones.  Here every mesh vertex owns the quad to its
// lower right and rasterises both triangles concurrently; the sequential order is restored with a
// 64-bit atomicMax per covered pixel on the key  (triangle_index + 1) << 32 | r << 16 | g << 8 | b :
// the largest triangle index wins, which is exactly the last writer of the sequential loop, and the
// colour rides along in the low bits.  A second kernel unpacks the keys (and clears them for the
// next frame).  Per-pixel arithmetic is the reference's float expression, operation for operation
// (-ffp-contract=off), so the output is bit exact against the CPU code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace arap {

struct WarpJob {                    // one frame
    const float2* field;            // warp field [N] (Offset), or NULL when `flow_in` is given
    const float2* flow_in;          // flow [N]: warp field = (x,y) + flow (main.cpp:159-166), or NULL
    const uint8_t* rgb;             // [N][3] or NULL
    const uint8_t* mask;            // [N]  0 = object
    float2* flow_out;               // [N] or NULL: Offset - (x,y)
    unsigned long long* key;        // [N] scratch, all zero on entry
    uint8_t* out_rgb;               // [N][3] or NULL
    uint8_t* out_mask;              // [N]
    // optional outputs of arap_occ.h (DESIGN.md "Backward flow and occlusion"): NULL = not wanted
    float2* bwd;                    // [N] backward flow, frame-2 domain
    uint8_t* occ_bwd;               // [N] 255 = revealed background in frame 2
    uint8_t* occ;                   // [N] 255 = frame-1 pixel occluded in frame 2
    unsigned* cell;                 // [N+1] scratch of the occlusion query: per-cell counts -> starts, zero on entry
    unsigned* rank;                 // [N]   scratch: a vertex's rank inside its cell
    int4* bin;                      // [N]   scratch: binned vertices {P.x, P.y, v, m(v)}
    // optional output of arap_mid.h (DESIGN.md "In-between frames"): all NULL = not wanted
    const float2* field_b;          // [N] second state as positions, or NULL when `flow_b` is given
    const float2* flow_b;           // [N] second state as a flow: position = (x,y) + flow, or NULL
    float2* step;                   // [N] flow from the warp of `field` to the second state, domain of the warped frame
};

__device__ __forceinline__ float2 warp_pos(const WarpJob& j, int x, int y, int i)
{
    if (j.field) return j.field[i];
    const float2 f = j.flow_in[i];
    return make_float2((float)x + f.x, (float)y + f.y);
}

// The rasteriser's inside test and barycentrics of triangle (p0, p1, p2) at the point (sx, sy) (main.cpp:69-104).  The
// one copy of this expression: raster_tri, the backward pass and the occlusion query (arap_occ.h) all call it, so their
// float results cannot drift apart.  Returns false where the rasteriser skips the point.
__device__ __forceinline__ bool tri_bary(float2 p0, float2 p1, float2 p2, float sx, float sy, float& b0, float& b1,
                                         float& b2)
{
    const float X0 = p0.x - sx * 1.0f, X1 = p1.x - sx * 1.0f, X2 = p2.x - sx * 1.0f;
    const float Y0 = p0.y - sy * 1.0f, Y1 = p1.y - sy * 1.0f, Y2 = p2.y - sy * 1.0f;
    float d01 = X0 * Y1 - Y0 * X1;
    float d12 = X1 * Y2 - Y1 * X2;
    float d20 = X2 * Y0 - Y2 * X0;
    if ((d01 < 0) & (d12 < 0) & (d20 < 0)) return false;
    const float OneOverD = 1.f / ((d01 + d12) + d20);
    d01 *= OneOverD;
    d12 *= OneOverD;
    d20 *= OneOverD;
    if (!(d01 >= 0 && d12 >= 0 && d20 >= 0)) return false;
    b0 = d12; b1 = d20; b2 = d01;
    return true;
}

// the cells raster_tri visits for a triangle: x = xa, xa+1, .. while x < W and x <= maxx (y likewise); false if none
// (a NaN corner)
__device__ __forceinline__ bool tri_cells(int W, int H, float2 p0, float2 p1, float2 p2, int& xa, int& ya, float& maxx,
                                          float& maxy)
{
    const float minx = floorf(fminf(p0.x, fminf(p1.x, p2.x)));
    const float miny = floorf(fminf(p0.y, fminf(p1.y, p2.y)));
    maxx = ceilf(fmaxf(p0.x, fmaxf(p1.x, p2.x)));
    maxy = ceilf(fmaxf(p0.y, fmaxf(p1.y, p2.y)));
    if (!(minx == minx && miny == miny && maxx == maxx && maxy == maxy)) return false;
    xa = minx < 0.f ? 0 : (minx > (float)W ? W : (int)minx);
    ya = miny < 0.f ? 0 : (miny > (float)H ? H : (int)miny);
    return true;
}

// the interpolated colour r << 16 | g << 8 | b of a covered pixel (main.cpp:131-137); the one copy, as tri_bary
__device__ __forceinline__ unsigned tri_rgb(const float c0[3], const float c1[3], const float c2[3], float b0, float b1,
                                            float b2)
{
    unsigned rgbv = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float v = (c0[k] * b0 + c1[k] * b1) + c2[k] * b2;
        rgbv = (rgbv << 8) | (unsigned)(unsigned char)v;
    }
    return rgbv;
}

__device__ __forceinline__ void raster_tri(const WarpJob& j, int W, int H, unsigned tri, float2 p0, float2 p1,
                                           float2 p2, const float c0[3], const float c1[3], const float c2[3])
{
    int xa, ya;
    float maxx, maxy;
    if (!tri_cells(W, H, p0, p1, p2, xa, ya, maxx, maxy)) return;
    for (int x = xa; x < W && (float)x <= maxx; ++x)
        for (int y = ya; y < H && (float)y <= maxy; ++y) {
            float b0, b1, b2;
            if (!tri_bary(p0, p1, p2, (float)x, (float)y, b0, b1, b2)) continue;
            const unsigned rgbv = j.rgb ? tri_rgb(c0, c1, c2, b0, b1, b2) : 0u;
            const unsigned long long key = ((unsigned long long)(tri + 1u) << 32) | rgbv;
            atomicMax(j.key + (x + (size_t)W * y), key);
        }
}

// grid = (ceil(W/64), ceil(H/4), njobs), block = (64,4)
__global__ __launch_bounds__(256) void k_warp_raster(const WarpJob* jobs, int W, int H)
{
    const WarpJob j = jobs[blockIdx.z];
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= W || y >= H) return;
    const int i = x + W * y;
    if (j.flow_out) {
        const float2 o = j.field[i];
        j.flow_out[i] = make_float2(o.x - (float)x, o.y - (float)y);
    }
    if (!(x + 1 < W && y + 1 < H)) return;
    const int i01 = i + 1, i10 = i + W, i11 = i + W + 1;
    if (!(j.mask[i] == 0 && j.mask[i10] == 0 && j.mask[i01] == 0 && j.mask[i11] == 0)) return;
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
    raster_tri(j, W, H, 2u * (unsigned)i, p00, p01, p10, v00, v01, v10);
    raster_tri(j, W, H, 2u * (unsigned)i + 1u, p10, p01, p11, v10, v01, v11);
}

// grid = (ceil(N/256), 1, njobs), block = 256
__global__ __launch_bounds__(256) void k_warp_resolve(const WarpJob* jobs, int N)
{
    const WarpJob j = jobs[blockIdx.z];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const unsigned long long k = j.key[i];
    j.key[i] = 0ull;
    if (j.out_rgb) {
        j.out_rgb[3 * (size_t)i + 0] = (uint8_t)((k >> 16) & 0xffu);
        j.out_rgb[3 * (size_t)i + 1] = (uint8_t)((k >> 8) & 0xffu);
        j.out_rgb[3 * (size_t)i + 2] = (uint8_t)(k & 0xffu);
    }
    j.out_mask[i] = k ? 255 : 0;
}

}  // namespace arap
