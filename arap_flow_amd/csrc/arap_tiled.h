// arap_tiled.h -- LDS-staged phase A (k_pcg_a's arithmetic, operation for operation) on TX x TY tiles: one body,
// pcg_a_tile_body, behind two entry points:
//   k_pcg_a_lds<TX, TY>  : the general two-kernel path (any UrShape, LM term), tile = blockIdx; templated on the tile
//                          shape so that BASELINE config 5's tile sweep {16x16, 32x8, 64x4, 32x16, 64x8} can be measured
//   k_pcg_a_grid<TX, TY> : (arap_stream.h) the pixel-grid edge term and an XCD-aware tile order
//
// Each workgroup stages the NEW search direction p_l = z + beta p_{l-1} and cos/sin(A) of its tile plus a one-vertex
// halo in LDS (interior cells by their own thread, halo cells by the border threads, which redo the neighbour's update
// expression), then every thread reads its four neighbours from LDS.  Compared with k_pcg_a, which re-reads z, p and
// cos/sin of the four neighbours through L1/L2, a vertex's data is fetched from global memory (TX+2)(TY+2)/(TX TY)
// times instead of 5 times.
#pragma once
#include "arap_kernels.h"

namespace arap {

// Tile (btx, bty) of frame b by a workgroup of TX x TY threads that is number lb of the frame's nlb (order-fixed sum).
// GRID: UrShape is the pixel grid (no UrShape loads, jtj_edge_grid) and the plan is a Gauss-Newton one (no LM term).
template <int TX, int TY, bool GRID>
__device__ __forceinline__ void pcg_a_tile_body(const PlanDev& pd, int l, int btx, int bty, int b, unsigned lb, unsigned nlb)
{
    constexpr int LW = TX + 2, LH = TY + 2;
    __shared__ float2 sP[LH * LW];
    __shared__ float2 sC[LH * LW];
    __shared__ float sA[LH * LW];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int x = btx * TX + tx, y = bty * TY + ty;
    const int W = pd.W, H = pd.H;
    const bool in = x < W && y < H;
    const int i = x + W * y;
    const size_t gb = (size_t)b * pd.N;
    const unsigned f = in ? pd.flags[gb + i] : 0u;
    double* const sigma_l = red_slot(pd, b, 2 * l + 1);
    if (!__syncthreads_or((int)(f & F_ACT))) {                   // nothing active in this tile (it still reports: block_reduce_fixed)
        block_reduce_fixed<1>(pd, b, lb, nlb, 0.0, 0.0, sigma_l, nullptr);
        return;
    }
    const Slot sl = pd.slots[b];
    const PBuf pin = p_in(pd, l), pout = p_out(pd, l);
    const float beta = pcg_beta(pd, b, l);
    // p_l of vertex j (any in-image vertex; values at excluded vertices are never used)
    auto stage = [&](int j, int cell) {
        float2 pO = pin.O[gb + j];
        float pA = pin.A[gb + j];
        if (l > 0) next_dir(pO, pA, pd.zO[gb + j], pd.zA[gb + j], beta);
        sP[cell] = pO;
        sA[cell] = pA;
        sC[cell] = pd.cs[gb + j];
        return make_float4(pO.x, pO.y, pA, 0.f);
    };
    const int cell = (ty + 1) * LW + (tx + 1);
    float4 own = make_float4(0.f, 0.f, 0.f, 0.f);
    if (in) {
        own = stage(i, cell);
        if (f & F_ACT) { pout.O[gb + i] = make_float2(own.x, own.y); pout.A[gb + i] = own.z; }
        if (ty == 0 && y > 0) stage(i - W, cell - LW);
        if ((ty == TY - 1 || y == H - 1) && y + 1 < H) stage(i + W, cell + LW);
        if (tx == 0 && x > 0) stage(i - 1, cell - 1);
        if ((tx == TX - 1 || x == W - 1) && x + 1 < W) stage(i + 1, cell + 1);
    }
    __syncthreads();
    double d = 0.0;
    if (f & F_ACT) {
        const float wr2 = sl.wr * sl.wr;
        const float2 pO = make_float2(own.x, own.y);
        const float pA = own.z;
        const float2 csi = sC[cell];
        float ax = 0.f, ay = 0.f, aa = 0.f;
        if constexpr (GRID) {
            constexpr int DX = 1, DY = LW;                      // cell offsets of the x and y neighbours
            if (f & F_E0) jtj_edge_grid<0>(csi, pO, pA, sC[cell + DX], sP[cell + DX], sA[cell + DX], wr2, ax, ay, aa);
            if (f & F_E1) jtj_edge_grid<1>(csi, pO, pA, sC[cell - DX], sP[cell - DX], sA[cell - DX], wr2, ax, ay, aa);
            if (f & F_E2) jtj_edge_grid<2>(csi, pO, pA, sC[cell + DY], sP[cell + DY], sA[cell + DY], wr2, ax, ay, aa);
            if (f & F_E3) jtj_edge_grid<3>(csi, pO, pA, sC[cell - DY], sP[cell - DY], sA[cell - DY], wr2, ax, ay, aa);
        } else {
            const float2 Ui = sl.U[i];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if (!(f & (1u << s))) continue;
                const int nc = cell + (s == 0 ? 1 : (s == 1 ? -1 : (s == 2 ? LW : -LW)));
                const float2 Un = sl.U[i + noff(s, W)];
                jtj_edge(Ui.x - Un.x, Ui.y - Un.y, csi, pO, pA, sC[nc], sP[nc], sA[nc], wr2, ax, ay, aa);
            }
        }
        if (f & F_FIT) {
            const float wf2 = sl.wf * sl.wf;
            ax = fmaf(wf2, pO.x, ax);
            ay = fmaf(wf2, pO.y, ay);
        }
        if (!GRID && pd.lm) {                          // applyJTJ + CtC*P (o.t:2076-2082)
            const float2 c = pd.CtCO[gb + i];
            ax = fmaf(c.x, pO.x, ax);
            ay = fmaf(c.y, pO.y, ay);
            aa = fmaf(pd.CtCA[gb + i], pA, aa);
        }
        pd.ApO[gb + i] = make_float2(ax, ay);
        pd.ApA[gb + i] = aa;
        d = (double)dot3(pO.x, pO.y, pA, ax, ay, aa);
    }
    block_reduce_fixed<1>(pd, b, lb, nlb, d, 0.0, sigma_l, nullptr);
}

template <int TX, int TY>
__global__ __launch_bounds__(TX* TY) void k_pcg_a_lds(PlanDev pd, int l)
{
    pcg_a_tile_body<TX, TY, false>(pd, l, blockIdx.x, blockIdx.y, blockIdx.z, blockIdx.y * gridDim.x + blockIdx.x,
                                   gridDim.x * gridDim.y);
}

}  // namespace arap
