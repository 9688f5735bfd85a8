// arap_pcg.h -- the device pieces every kernel of the kernel-per-phase PCG path shares (arap_kernels.h, arap_tiled.h,
// arap_stream.h, arap_lm.h): the J^T J edge term in its generic and pixel-grid form, the raw diagonal, the table of the
// Offset preconditioner, the PCG scalars (reduction slots, alpha, beta), the double buffer of the search direction, the
// direction update, and the 16-byte quad accesses of phase B.
//
// Each helper states its IEEE operations in the order the oracle (oracle/arap_oracle.c) and the resident kernel
// (arap_resident.h) perform them: a reordered fmaf or a swapped operand here is a different result everywhere.
#pragma once
#include "arap_device.h"

namespace arap {

// ---- PCG scalars ---------------------------------------------------------------------------------------------------
// reduction slots of a Gauss-Newton step: 0 = rho_0 ; 2l+1 = sigma_l ; 2l+2 = rho_{l+1}
__device__ __forceinline__ double* red_slot(const PlanDev& pd, int b, int k)
{
    return pd.red + ((size_t)b * pd.nslots + k) * NSHARD;
}

__device__ __forceinline__ float pcg_scalar(const PlanDev& pd, int b, int k) { return read_scalar(red_slot(pd, b, k)); }

// num / den if den > 0 else 0: how PCGStep2 forms alpha and PCGStep3 beta (solverGPUGaussNewton.t:446-489, :537-550)
__device__ __forceinline__ float guarded_ratio(float num, float den)
{
    float q = 0.f;
    if (den > 0.f) q = num / den;
    return q;
}

// beta of iteration l = rho_l / rho_{l-1} (0 in iteration 0, whose direction is p_init)
__device__ __forceinline__ float pcg_beta(const PlanDev& pd, int b, int l)
{
    if (l <= 0) return 0.f;
    const float rhoNew = pcg_scalar(pd, b, 2 * l);
    const float rhoOld = pcg_scalar(pd, b, 2 * l - 2);
    return guarded_ratio(rhoNew, rhoOld);
}

// alpha of iteration l = rho_l / sigma_l
__device__ __forceinline__ float pcg_alpha(const PlanDev& pd, int b, int l)
{
    const float rho = pcg_scalar(pd, b, 2 * l);
    const float sigma = pcg_scalar(pd, b, 2 * l + 1);
    return guarded_ratio(rho, sigma);
}

// ---- the search direction -------------------------------------------------------------------------------------------
// p is double-buffered: phase A of iteration l reads p_in (p_{l-1}; p_init for l == 0) and writes p_out (p_l), because the
// stencil needs the neighbours' p_l, which every phase-A kernel recomputes from their z and p_{l-1}.  Phase B and the
// update kernels of iteration l read p_out(pd, l).
struct PBuf {
    float2* O;
    float* A;
};
__device__ __forceinline__ PBuf p_in(const PlanDev& pd, int l) { return (l & 1) ? PBuf{pd.pO1, pd.pA1} : PBuf{pd.pO0, pd.pA0}; }
__device__ __forceinline__ PBuf p_out(const PlanDev& pd, int l) { return (l & 1) ? PBuf{pd.pO0, pd.pA0} : PBuf{pd.pO1, pd.pA1}; }

// p = z + beta p (PCGStep3)
__device__ __forceinline__ void next_dir(float2& pO, float& pA, float2 zO, float zA, float beta)
{
    pO.x = fmaf(beta, pO.x, zO.x);
    pO.y = fmaf(beta, pO.y, zO.y);
    pA = fmaf(beta, pA, zA);
}

// ---- J^T J, one edge (applyJTJ, o.t:2029-2089; derivation: DESIGN.md "The math") ---------------------------------------
// q = R'(A(c)) d and h = R'(A(n)) d given: the term of the edge c -> n added to (ax, ay, aa)
__device__ __forceinline__ void jtj_edge_qh(float qx, float qy, float hx, float hy, float2 pO, float pA, float2 qO, float qA,
                                            float wr2, float& ax, float& ay, float& aa)
{
    const float px = pO.x - qO.x, py = pO.y - qO.y;
    const float tx = fmaf(-qx, pA, px), ty = fmaf(-qy, pA, py);
    ax = fmaf(wr2, fmaf(-hx, qA, px + tx), ax);
    ay = fmaf(wr2, fmaf(-hy, qA, py + ty), ay);
    aa = fmaf(-wr2, fmaf(qx, tx, qy * ty), aa);
}

// any UrShape: d = U(c) - U(n); own (cos, sin) and direction (csi, pO, pA), the neighbour's (csn, qO, qA)
__device__ __forceinline__ void jtj_edge(float dx, float dy, float2 csi, float2 pO, float pA, float2 csn, float2 qO, float qA,
                                         float wr2, float& ax, float& ay, float& aa)
{
    const float ci = csi.x, si = csi.y, cn = csn.x, sn = csn.y;
    const float qx = fmaf(-si, dx, -(ci * dy)), qy = fmaf(ci, dx, -(si * dy));
    const float hx = fmaf(-sn, dx, -(cn * dy)), hy = fmaf(cn, dx, -(sn * dy));
    jtj_edge_qh(qx, qy, hx, hy, pO, pA, qO, qA, wr2, ax, ay, aa);
}

// UrShape = the pixel grid (every frame-solver plan): d = -s for stencil entry S, so q and h are signed copies of
// (si, ci) / (sn, cn) -- a product with -1 / 0 / 1 and the addition of a zero are exact, so every value equals the
// generic term's (only the sign of an exact zero may differ).  THE sign table of the grid edge; the resident kernel's
// RES_EDGE (arap_resident.h) spells the same four rows on packed pairs.
//      S   s         q            h
//      0  ( 1, 0)   ( si,-ci)    ( sn,-cn)
//      1  (-1, 0)   (-si, ci)    (-sn, cn)
//      2  ( 0, 1)   ( ci, si)    ( cn, sn)
//      3  ( 0,-1)   (-ci,-si)    (-cn,-sn)
template <int S>
__device__ __forceinline__ void jtj_edge_grid(float2 csi, float2 pO, float pA, float2 csn, float2 qO, float qA, float wr2,
                                              float& ax, float& ay, float& aa)
{
    static_assert(S >= 0 && S < 4, "stencil entry");
    const float ci = csi.x, si = csi.y, cn = csn.x, sn = csn.y;
    if (S == 0) jtj_edge_qh(si, -ci, sn, -cn, pO, pA, qO, qA, wr2, ax, ay, aa);
    if (S == 1) jtj_edge_qh(-si, ci, -sn, cn, pO, pA, qO, qA, wr2, ax, ay, aa);
    if (S == 2) jtj_edge_qh(ci, si, cn, sn, pO, pA, qO, qA, wr2, ax, ay, aa);
    if (S == 3) jtj_edge_qh(-ci, -si, -cn, -sn, pO, pA, qO, qA, wr2, ax, ay, aa);
}

// ---- diag(J^T J) ---------------------------------------------------------------------------------------------------
// one valid edge's share, q = R'(A(c)) d (k_gn_init interleaves these two lines with the gradient's)
__device__ __forceinline__ void jtj_diag_edge(float wr, float qx, float qy, float& dO, float& dA)
{
    dO = dO + (wr * wr + wr * wr);
    dA = fmaf(wr * wr, fmaf(qx, qx, qy * qy), dA);
}

// raw diag(J^T J) of vertex i of frame image index g (flag byte f), in the accumulation order of k_gn_init
__device__ __forceinline__ void jtj_diag(const PlanDev& pd, const Slot& sl, size_t g, int i, unsigned f, float& DO, float& DA)
{
    const float wr = sl.wr, wf = sl.wf;
    const float2 csi = pd.cs[g];
    const float2 Ui = sl.U[i];
    float dO = 0.f, dA = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        if (!(f & (1u << s))) continue;
        const float2 Un = sl.U[i + noff(s, pd.W)];
        const float dx = Ui.x - Un.x, dy = Ui.y - Un.y;
        const float qx = fmaf(-csi.y, dx, -(csi.x * dy)), qy = fmaf(csi.x, dx, -(csi.y * dy));
        jtj_diag_edge(wr, qx, qy, dO, dA);
    }
    if (f & F_FIT) dO = fmaf(wf, wf, dO);
    DO = dO; DA = dA;
}

// ---- M^-1 of the Offset components ---------------------------------------------------------------------------------
// D_O = sum over valid edges of (wr*wr + wr*wr), plus wf*wf if the fit term is on (k_gn_init): a function of (degree,
// fit) only, so the kernels that do not read preO take it from ten entries in LDS.  fill() by threads 0..9 of the
// workgroup, a barrier, then of(flag byte).  (k_pcg_resident keeps its own fill inside its carved LDS block: same loop.)
struct MoLut {
    float t[12];
    __device__ __forceinline__ void fill(const Slot& sl, int tid)
    {
        if (tid < 10) {
            const int deg = tid % 5, fit = tid / 5;
            float dO = 0.f;
            for (int k = 0; k < deg; ++k) dO = dO + (sl.wr * sl.wr + sl.wr * sl.wr);
            if (fit) dO = fmaf(sl.wf, sl.wf, dO);
            t[tid] = ginv(dO);
        }
    }
    __device__ __forceinline__ float of(unsigned f) const { return t[__popc(f & 15u) + 5 * (int)((f >> 4) & 1u)]; }
};

// ---- phase B on quads: four consecutive vertices per lane, every access 16 bytes -----------------------------------------
// quad q of an Offset-shaped image is two float4, of an Angle-shaped image one
__device__ __forceinline__ void ld_quadO(float (&v)[8], const float2* img, int q)
{
    const float4* p = (const float4*)img;
    *(float4*)&v[0] = p[2 * q]; *(float4*)&v[4] = p[2 * q + 1];
}
__device__ __forceinline__ void ld_quadA(float (&v)[4], const float* img, int q) { *(float4*)v = ((const float4*)img)[q]; }
__device__ __forceinline__ void st_quadO(float2* img, int q, const float (&v)[8])
{
    float4* p = (float4*)img;
    p[2 * q] = *(const float4*)&v[0]; p[2 * q + 1] = *(const float4*)&v[4];
}
__device__ __forceinline__ void st_quadA(float* img, int q, const float (&v)[4]) { ((float4*)img)[q] = *(const float4*)v; }

}  // namespace arap
