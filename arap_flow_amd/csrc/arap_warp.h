// arap_warp.h -- forward triangle rasteriser + flow emission on the GPU (gfx950).
//
// Reference: ARAP/warping/src/main.cpp:69-104 (PointInTriangleLK), :110-142 (rasterizeTriangle),
// :145-225 (Warp); the same code lives in ARAP/deformation/src/CombinedSolver.h:61-97,248-342, and
// flow = Offset - grid is CombinedSolver.h:352-366.
//
// The reference rasterises quads sequentially (y outer, x inner; triangle (00,01,10) then
// (10,01,11)) and later writes overwrite earlier ones.  Here every mesh vertex owns the quad to its
// lower right and rasterises both triangles concurrently; the sequential order is restored with a
// 64-bit atomicMax per covered pixel on a key (warp_key below) with the triangle index above the
// colour: the largest triangle index wins, which is exactly the last writer of the sequential loop,
// and the colour rides along in the low bits.  A second kernel unpacks the keys (and clears them for
// the next frame).  Per-pixel arithmetic is the reference's float expression, operation for operation
// (-ffp-contract=off), so the output is bit exact against the CPU code.
//
// This file holds what every member of the warp family shares (arap_occ.h, arap_mid.h, arap_layers.h,
// arap_layers_step.h): the job, the key, the inside test, the cell walk, the quad body, the corner
// numbering of a triangle and the barycentric mix, each stated once.
//
// Order on the stream:  k_warp_raster -> [passes of the other headers, which read the keys] -> k_warp_resolve.
// Limits: 2N < 2^32 (32 bits of triangle + 1 in the key).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct ArapFlow_MeshStats;          // include/arap_opt.h

namespace arap {

struct DiagAcc;                     // arap_diag.h

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
    // optional outputs of arap_diag.h (DESIGN.md "Fold diagnostics"): NULL = not wanted; `acc` and `stats` go together
    uint8_t* fold;                  // [N] 255 = object vertex with a folded or non-finite triangle at it
    DiagAcc* acc;                   // the job's accumulator, all zero on entry
    ArapFlow_MeshStats* stats;      // the statistics decoded from `acc`
};

// the position a flow value gives vertex (x, y) (main.cpp:159-166); the one copy
__device__ __forceinline__ float2 flow_pos(int x, int y, float2 f)
{
    return make_float2((float)x + f.x, (float)y + f.y);
}

__device__ __forceinline__ float2 warp_pos(const WarpJob& j, int x, int y, int i)
{
    if (j.field) return j.field[i];
    return flow_pos(x, y, j.flow_in[i]);
}

// where warp_quad takes a vertex's position from: by default the job's field or flow (warp_pos).  arap_blur.h places the
// vertices by a flow it mixes on the fly; every other caller leaves the default, and its code is what it was.
struct JobPos {
    __device__ __forceinline__ float2 operator()(const WarpJob& j, int x, int y, int i) const { return warp_pos(j, x, y, i); }
};

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

// the one barycentric mix of three corner values (main.cpp:131-137): colours, source points, points of a second state
__device__ __forceinline__ float bary_mix(float a, float b, float c, float b0, float b1, float b2)
{
    return (a * b0 + b * b1) + c * b2;
}

// the interpolated colour r << 16 | g << 8 | b of a covered pixel (main.cpp:131-137); the one copy, as tri_bary
__device__ __forceinline__ unsigned tri_rgb(const float c0[3], const float c1[3], const float c2[3], float b0, float b1,
                                            float b2)
{
    unsigned rgbv = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) rgbv = (rgbv << 8) | (unsigned)(unsigned char)bary_mix(c0[k], c1[k], c2[k], b0, b1, b2);
    return rgbv;
}

// The key of a covered pixel, one format for the whole family:
//     (l + 1) << 56 | (t + 1) << 24 | r << 16 | g << 8 | b        0 = not covered
// with t the triangle and l its layer (arap_layers.h; 0 on the single-layer paths).  atomicMax keeps the
// lexicographically largest (layer, triangle); 8 bits of l + 1 and 32 bits of t + 1 give the limits n <= 255, 2N < 2^32.
// warp_key states the bits above the colour, key_winner reads them back: no kernel shifts a key by hand.
__device__ __forceinline__ unsigned long long warp_key(unsigned layer, unsigned tri)
{
    return ((unsigned long long)(layer + 1u) << 56) | ((unsigned long long)(tri + 1u) << 24);
}

struct KeyWinner { bool covered; unsigned layer, tri; };        // layer and tri mean nothing where !covered

__device__ __forceinline__ KeyWinner key_winner(unsigned long long k)
{
    return KeyWinner{k != 0ull, (unsigned)(k >> 56) - 1u, (unsigned)(k >> 24) - 1u};
}

// rasterise triangle (p0, p1, p2) under the key bits `hi` = warp_key(layer, triangle)
__device__ __forceinline__ void raster_tri(const WarpJob& j, int W, int H, unsigned long long hi, float2 p0, float2 p1,
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
            atomicMax(j.key + (x + (size_t)W * y), hi | rgbv);
        }
}

// quad (qx, qy) is rasterised iff it lies in the grid and its four corners are object
__device__ __forceinline__ bool quad_on(const uint8_t* mask, int W, int H, int qx, int qy)
{
    if (qx < 0 || qy < 0 || qx + 1 >= W || qy + 1 >= H) return false;
    const size_t i = qx + (size_t)W * qy;
    return mask[i] == 0 && mask[i + 1] == 0 && mask[i + W] == 0 && mask[i + W + 1] == 0;
}

// The work of vertex (x, y) on the quad to its lower right, the one copy: if the quad is rasterised, its four corner
// positions, their colours when COLOUR (zeros without an image) and  act(t, p0, p1, p2, c0, c1, c2)  for its two
// triangles in the reference's order, 2i = (00,01,10) then 2i+1 = (10,01,11).  `act` rasterises or queries; `pos`
// places the corners (JobPos above).
template <bool COLOUR, class Act, class Pos = JobPos>
__device__ __forceinline__ void warp_quad(const WarpJob& j, int W, int H, int x, int y, Act act, Pos pos = Pos())
{
    if (!quad_on(j.mask, W, H, x, y)) return;
    const int i = x + W * y, i01 = i + 1, i10 = i + W, i11 = i + W + 1;
    const float2 p00 = pos(j, x, y, i), p01 = pos(j, x + 1, y, i01);
    const float2 p10 = pos(j, x, y + 1, i10), p11 = pos(j, x + 1, y + 1, i11);
    float v00[3] = {0, 0, 0}, v01[3] = {0, 0, 0}, v10[3] = {0, 0, 0}, v11[3] = {0, 0, 0};
    if (COLOUR && j.rgb) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            v00[k] = (float)j.rgb[3 * (size_t)i + k];
            v01[k] = (float)j.rgb[3 * (size_t)i01 + k];
            v10[k] = (float)j.rgb[3 * (size_t)i10 + k];
            v11[k] = (float)j.rgb[3 * (size_t)i11 + k];
        }
    }
    act(2u * (unsigned)i, p00, p01, p10, v00, v01, v10);
    act(2u * (unsigned)i + 1u, p10, p01, p11, v10, v01, v11);
}

// warp_quad with raster_tri as the action, for the job seen as layer `layer`
template <class Pos = JobPos>
__device__ __forceinline__ void raster_quad(const WarpJob& j, int W, int H, int x, int y, unsigned layer, Pos pos = Pos())
{
    warp_quad<true>(j, W, H, x, y, [&](unsigned t, float2 p0, float2 p1, float2 p2, const float* c0, const float* c1,
                                       const float* c2) { raster_tri(j, W, H, warp_key(layer, t), p0, p1, p2, c0, c1, c2); },
                    pos);
}

// warp_quad's numbering read back: the grid coordinates and indices of the three corners of triangle t,
// 2u = (p00, p01, p10), 2u+1 = (p10, p01, p11) of the quad of vertex u
struct TriCorners { int x[3], y[3], i[3]; };

__device__ __forceinline__ TriCorners tri_corners(unsigned t, int W)
{
    const int u = (int)(t >> 1);
    const int uy = u / W, ux = u - uy * W;
    const int odd = (int)(t & 1u);
    TriCorners c = {{ux, ux + 1, ux + odd}, {uy + odd, uy, uy + 1}, {0, 0, 0}};
#pragma unroll
    for (int k = 0; k < 3; ++k) c.i[k] = c.x[k] + W * c.y[k];
    return c;
}

// grid = (ceil(W/64), ceil(H/4), njobs), block = (64,4)
__global__ __launch_bounds__(256) void k_warp_raster(const WarpJob* jobs, int W, int H)
{
    const WarpJob j = jobs[blockIdx.z];
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= W || y >= H) return;
    if (j.flow_out) {
        const int i = x + W * y;
        const float2 o = j.field[i];
        j.flow_out[i] = make_float2(o.x - (float)x, o.y - (float)y);
    }
    raster_quad(j, W, H, x, y, 0u);
}

// unpack RGB and mask, each if its pointer is set, and clear the keys
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
    if (j.out_mask) j.out_mask[i] = k ? 255 : 0;
}

}  // namespace arap
