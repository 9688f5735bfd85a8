// arap_chain.h -- flow chaining: estimated point tracks from per-link flow estimates, the baseline a flow estimator is
// scored by on the track files (gfx950).
//
// Definitions: DESIGN.md "Track scoring", "Flow chaining"; the numpy twin is tests/tscore_ref.py.  Link j of `flows` is
// the estimated flow from sequence frame j to j + 1 on the integer pixels of frame j, link j of `bwd` (optional) the one
// from frame j + 1 back to j.  One lane per query point, the links in sequence: a link is one bilinear sample of the
// forward flow at the point's sub-pixel position -- four 8-byte gathers -- and with `bwd` one more of the backward flow at
// where it lands, for the forward-backward check.  A point that leaves the frame (or goes NaN) is lost for good and stays
// where it left; the test is made before any floorf, so every gather is inside its link's plane.
#pragma once
#include "../../include/arap_opt.h"
#include "arap_occ.h"

namespace arap {

struct ChainJob {
    const float2 *flows, *bwd;            // [L][H][W]; bwd or NULL
    const float2* points;                 // [P]
    float2* pos;                          // [L + 1][P]
    uint8_t* occ;                         // [L + 1][P]
    int W, H;
    unsigned L, P;
};

// S(A, a), a inside the frame: bilinear, the right and bottom neighbours clamped to the edge; arap_bg.h's sampler order
__device__ __forceinline__ float2 chain_sample(const float2* A, float2 a, int W, int H)
{
    const int x0 = (int)floorf(a.x), y0 = (int)floorf(a.y);
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    const float fx = a.x - (float)x0, fy = a.y - (float)y0;
    const float2* const r0 = A + (size_t)y0 * W;
    const float2* const r1 = A + (size_t)y1 * W;
    const float2 c00 = r0[x0], c01 = r0[x1], c10 = r1[x0], c11 = r1[x1];
    const float tx = fmaf(fx, c01.x - c00.x, c00.x), bx = fmaf(fx, c11.x - c10.x, c10.x);
    const float ty = fmaf(fx, c01.y - c00.y, c00.y), by = fmaf(fx, c11.y - c10.y, c10.y);
    return make_float2(fmaf(fy, bx - tx, tx), fmaf(fy, by - ty, ty));
}

// grid = (ceil(P / 256)), block = 256
__global__ __launch_bounds__(256) void k_chain_flows(ChainJob j)
{
    const unsigned k = blockIdx.x * 256u + threadIdx.x;
    if (k >= j.P) return;
    const size_t N = (size_t)j.W * j.H;
    float2 p = j.points[k];
    bool lost = !in_frame(p, j.W, j.H);
    j.pos[k] = p;
    j.occ[k] = lost ? 255 : 0;
    for (unsigned l = 0; l < j.L; ++l) {
        uint8_t o = 255;
        if (!lost) {
            const float2 f = chain_sample(j.flows + l * N, p, j.W, j.H);
            const float2 b = make_float2(p.x + f.x, p.y + f.y);
            p = b;
            if (!in_frame(b, j.W, j.H)) {
                lost = true;
            } else if (j.bwd) {
                const float2 g = chain_sample(j.bwd + l * N, b, j.W, j.H);
                const float sx = f.x + g.x, sy = f.y + g.y;
                const float d2 = (sx * sx) + (sy * sy);
                const float m2 = ((f.x * f.x) + (f.y * f.y)) + ((g.x * g.x) + (g.y * g.y));
                o = !(d2 <= fmaf(0.01f, m2, 0.5f)) ? 255 : 0;
            } else {
                o = 0;
            }
        }
        const size_t at = (size_t)(l + 1) * j.P + k;
        j.pos[at] = p;
        j.occ[at] = o;
    }
}

}  // namespace arap
