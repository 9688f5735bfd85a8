// arap_diag.h -- fold diagnostics of a warp field: per-job mesh statistics and the per-vertex fold map (gfx950).
//
// Definitions: DESIGN.md "Fold diagnostics".  Both kernels take the same WarpJob array as k_warp_raster (arap_warp.h)
// and only run when a caller asked for the outputs; with them off nothing is launched.  The kernels read the field and
// the mask only, not the raster keys, so they may sit anywhere between the solve and the end of the warp chain.
// Every output is an integer count, a flag or an extremum in the total order of the IEEE bit patterns: integer atomics
// only, and the result is a function of the inputs alone, whatever order the blocks arrive in.
//
// Order on the stream:  hipMemsetAsync(accumulators, 0) -> k_warp_diag -> k_diag_finish.
#pragma once
#include "../../include/arap_opt.h"
#include "arap_occ.h"

namespace arap {

// The per-job accumulator, all zero = the identity of every word, so one memset re-arms it.  The three extrema travel
// as order-preserving keys (diag_key) under atomicMax: det_max and disp2_max as the key itself, det_min as its
// complement.  The key of every finite value and of +-inf, and its complement, is > 0; 0 means "none seen".
struct DiagAcc { unsigned vertices, outside, triangles, folded, nonfinite, ndet_min, det_max, disp2_max; };
enum { DIAG_WORDS = 8, DIAG_SUMS = 5 };           // the first DIAG_SUMS words are sums, the rest maxima
static_assert(sizeof(DiagAcc) == 4 * DIAG_WORDS, "one word per statistic");

// float -> unsigned, monotone in the total order of the bit patterns (-0 < +0), and back
__device__ __forceinline__ unsigned diag_key(float f)
{
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float diag_unkey(unsigned k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// det(t) of DESIGN.md: e1 = p1 - p0, e2 = p2 - p0, e1.x e2.y - e1.y e2.x, every operator one float32 operation
__device__ __forceinline__ float tri_det(float2 p0, float2 p1, float2 p2)
{
    const float e1x = p1.x - p0.x, e1y = p1.y - p0.y, e2x = p2.x - p0.x, e2y = p2.y - p0.y;
    return (e1x * e2y) - (e1y * e2x);
}

__device__ __forceinline__ bool diag_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }     // false on NaN

// The two dets of quad (qx, qy) through warp_quad (its numbering, quad_on and warp_pos): false if it is not rasterised
__device__ __forceinline__ bool diag_quad(const WarpJob& j, int W, int H, int qx, int qy, float det[2])
{
    bool on = false;
    warp_quad<false>(j, W, H, qx, qy, [&](unsigned t, float2 p0, float2 p1, float2 p2, const float*, const float*,
                                          const float*) { on = true; det[t & 1u] = tri_det(p0, p1, p2); });
    return on;
}

// a rasterised triangle with this det is folded (finite, <= 0) or non-finite: its corners go into the fold map
__device__ __forceinline__ bool diag_tri_bad(float det) { return !(diag_finite(det) && det > 0.f); }

// the flag bits of quad (qx, qy) in the fold gather: bit k set = triangle 2u + k is rasterised and bad
__device__ __forceinline__ unsigned diag_quad_bits(bool on, const float det[2])
{
    return on ? ((diag_tri_bad(det[0]) ? 1u : 0u) | (diag_tri_bad(det[1]) ? 2u : 0u)) : 0u;
}

// Every vertex: its own counts and the two dets of the quad to its lower right; wave sums by ballot, wave maxima by
// shuffles, the four waves through LDS, then one atomic per statistic that is not the identity.  The fold map is a
// gather over the block's quad flags in LDS, staged with a one-quad halo to the left and above; halo quads are
// flagged only, never counted.
// grid = (ceil(W/64), ceil(H/4), njobs), block = (64,4)
__global__ __launch_bounds__(256) void k_warp_diag(const WarpJob* jobs, int W, int H)
{
    const WarpJob j = jobs[blockIdx.z];
    __shared__ uint8_t qbad[5][66];               // flags of quad (x0 - 1 + c, y0 - 1 + r)
    __shared__ unsigned red[4][DIAG_WORDS];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int x0 = blockIdx.x * 64, y0 = blockIdx.y * 4;
    const int x = x0 + tx, y = y0 + ty;
    const bool in_grid = x < W && y < H;
    const int i = in_grid ? x + W * y : 0;
    const bool object = in_grid && j.mask[i] == 0;

    float det[2] = {1.f, 1.f};
    const bool on = diag_quad(j, W, H, x, y, det);
    const bool fin0 = on && diag_finite(det[0]), fin1 = on && diag_finite(det[1]);

    if (j.fold) {
        qbad[ty + 1][tx + 1] = (uint8_t)diag_quad_bits(on, det);
        const int h = tx + 64 * ty;               // the 65 quads above the block, then the 4 to its left
        if (h < 69) {
            const int c = h < 65 ? h : 0, r = h < 65 ? 0 : h - 64;
            float hd[2] = {1.f, 1.f};
            const bool hon = diag_quad(j, W, H, x0 - 1 + c, y0 - 1 + r, hd);
            qbad[r][c] = (uint8_t)diag_quad_bits(hon, hd);
        }
    }

    if (j.acc) {
        bool outside = false;
        unsigned kdisp = 0u;
        if (object) {
            const float2 P = warp_pos(j, x, y, i);
            outside = !in_frame(P, W, H);
            if (diag_finite(P.x) && diag_finite(P.y)) {
                const float dx = P.x - (float)x, dy = P.y - (float)y;
                kdisp = diag_key((dx * dx) + (dy * dy));
            }
        }
        unsigned nmin = 0u, kmax = 0u;
        if (fin0) { const unsigned k = diag_key(det[0]); nmin = ~k; kmax = k; }
        if (fin1) { const unsigned k = diag_key(det[1]); nmin = max(nmin, ~k); kmax = max(kmax, k); }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            nmin = max(nmin, (unsigned)__shfl_xor((int)nmin, o, 64));
            kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, o, 64));
            kdisp = max(kdisp, (unsigned)__shfl_xor((int)kdisp, o, 64));
        }
        const unsigned nvert = (unsigned)__popcll(__ballot(object));
        const unsigned nout = (unsigned)__popcll(__ballot(outside));
        const unsigned ntri = 2u * (unsigned)__popcll(__ballot(on));
        const unsigned nnon = (unsigned)(__popcll(__ballot(on && !fin0)) + __popcll(__ballot(on && !fin1)));
        const unsigned nfold = (unsigned)(__popcll(__ballot(fin0 && det[0] <= 0.f)) + __popcll(__ballot(fin1 && det[1] <= 0.f)));
        if (tx == 0) {
            unsigned* r = red[ty];
            r[0] = nvert; r[1] = nout; r[2] = ntri; r[3] = nfold; r[4] = nnon; r[5] = nmin; r[6] = kmax; r[7] = kdisp;
        }
    }
    __syncthreads();

    if (j.acc && ty == 0 && tx < DIAG_WORDS) {
        const unsigned a = red[0][tx], b = red[1][tx], c = red[2][tx], d = red[3][tx];
        unsigned* acc = (unsigned*)j.acc + tx;
        if (tx < DIAG_SUMS) {
            const unsigned v = (a + b) + (c + d);
            if (v) atomicAdd(acc, v);
        } else {
            const unsigned v = max(max(a, b), max(c, d));
            if (v) atomicMax(acc, v);
        }
    }
    if (j.fold && in_grid) {
        // the vertex is p00 of quad (x, y) (triangle 2u), p01 of (x-1, y) and p10 of (x, y-1) (both triangles),
        // p11 of (x-1, y-1) (triangle 2u+1): own_max_tri's list (arap_occ.h)
        const unsigned any = (qbad[ty + 1][tx + 1] & 1u) | qbad[ty + 1][tx] | qbad[ty][tx + 1] | (qbad[ty][tx] & 2u);
        j.fold[i] = (object && any) ? 255 : 0;
    }
}

// one thread per job: decode the accumulator into the caller's struct
// grid = ceil(njobs/64), block = 64
__global__ __launch_bounds__(64) void k_diag_finish(const WarpJob* jobs, int njobs)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= njobs) return;
    const WarpJob j = jobs[b];
    if (!j.acc) return;
    const DiagAcc a = *j.acc;
    ArapFlow_MeshStats s;
    s.vertices = a.vertices; s.outside = a.outside; s.triangles = a.triangles;
    s.folded = a.folded; s.nonfinite = a.nonfinite; s.reserved = 0u;
    s.det_min = a.ndet_min ? diag_unkey(~a.ndet_min) : __uint_as_float(0x7f800000u);
    s.det_max = a.det_max ? diag_unkey(a.det_max) : __uint_as_float(0xff800000u);
    s.disp2_max = a.disp2_max ? diag_unkey(a.disp2_max) : 0.f;
    *j.stats = s;
}

}  // namespace arap
