// arap_stream.h -- the streaming (state in HBM / Infinity Cache) PCG kernels of the FRAME SOLVER's two-kernel path:
// what runs when a solve has more active tiles than the resident kernel holds (1920x1080 with every vertex active:
// 8100 tiles) or when the resident path pauses after a timed-out launch.
//
// Same arithmetic as k_pcg_a / k_pcg_b (arap_kernels.h), operation for operation, from the same pieces (arap_pcg.h); what
// differs is the traffic:
//   * k_pcg_a_grid: phase A specialised to the pixel-grid UrShape the frame solver always has (CombinedSolver.h:207-221:
//     d = U(c) - U(n) = -s, no UrShape loads: 8 B + 4 cached neighbour loads per vertex less; jtj_edge_grid), the tile body
//     of arap_tiled.h (the new direction and cos/sin staged in LDS with a one-vertex halo), and an XCD-AWARE TILE ORDER:
//     workgroups are dealt round-robin to
//     the 8 XCDs, whose L2s do not share lines, so with the plain blockIdx -> tile map the two tiles either side of a
//     tile boundary sit on different XCDs and every halo row is fetched through the fabric a second time (measured at
//     1920x1080, mask == 0: FETCH_SIZE x 2 = 155 MB against 85 MB algorithmic).  Here XCD j works through the j-th
//     eighth of the tile list, top to bottom: vertically adjacent tiles share an L2 and are in flight together.
//   * k_pcg_b4_lean: phase B with 16-byte accesses that reads neither z (it is only written; read back only for a quad
//     with an excluded vertex, whose z must survive) nor the Offset preconditioner (a function of the vertex's degree
//     and fit flag: MoLut, as in the resident kernel): 53 B read + 36 B written per vertex instead of 73 + 36.
//   * k_pcg_a_march / k_pcg_a_march2 (one body, pcg_a_march_body) and k_pcg_b4_r: see below.
#pragma once
#include "arap_tiled.h"

namespace arap {

// tile (tx, ty) and frame of a workgroup of a 1-D launch of nb * 8 * chunk blocks, chunk = ceil(tiles / 8)
__device__ __forceinline__ bool xcd_tile(int tilesX, int tilesY, int chunk, int& tx, int& ty, int& b, unsigned& lb)
{
    const int bid = blockIdx.x;
    b = bid / (8 * chunk);
    const int r = bid - b * 8 * chunk;
    lb = (unsigned)r;                                 // linear index among the frame's 8 * chunk workgroups
    const int tile = (r & 7) * chunk + (r >> 3);
    if (tile >= tilesX * tilesY) return false;
    ty = tile / tilesX;
    tx = tile - ty * tilesX;
    return true;
}

template <int TX, int TY>
__global__ __launch_bounds__(TX* TY) void k_pcg_a_grid(PlanDev pd, int l, int tilesX, int tilesY, int chunk)
{
    int btx, bty, b;
    unsigned lb;
    const bool has_tile = xcd_tile(tilesX, tilesY, chunk, btx, bty, b, lb);
    const unsigned nlb = 8u * (unsigned)chunk;
    if (!has_tile) { block_reduce_fixed<1>(pd, b, lb, nlb, 0.0, 0.0, red_slot(pd, b, 2 * l + 1), nullptr); return; }
    pcg_a_tile_body<TX, TY, true>(pd, l, btx, bty, b, lb, nlb);
}

// Phase A as a MARCH down a 64-column strip: a workgroup of 4 wavefronts (one row of 64 vertices each) owns RB
// consecutive 4-row blocks of one strip.  A ring of four blocks in LDS holds the new direction and cos/sin; in step k
// the loads of block k+2 are issued, block k is computed from LDS (its upper neighbours are the last row of block k-1,
// the lower ones the first row of block k+1: consecutive ring rows) and block k+2 is then written to the ring.  Every
// vertex is fetched once (plus one halo row above and below the RB blocks, and the two halo columns), the global loads
// of the next block fly while the current one is computed, and the phase's dot product costs one atomic per workgroup.
// Blocks whose 64x4 tile holds no active vertex (pd.tileact, rebuilt by k_gn_prep) are neither loaded nor computed.
//
// LEAN -- the lean schedule (frame-solver plans): 126 instead of 146 bytes per vertex and iteration.
// What the two phases of an iteration must do is fixed by the two sums (sigma = p.Ap needs every p, rho' = z.r needs the
// new r everywhere); WHERE the element-wise work is done is free.  k_pcg_a_march2 / k_pcg_b4_r move it so that fewer
// bytes travel (same operations on the same operands: the bits do not change):
//   * z = M^-1 r is never stored: phase B needs it only for its dot product, and phase A forms it again from r, M^-1_A
//     and the flag byte (M^-1_O is a function of the flags: MoLut) for every vertex it stages  (-12 B written, +4 B read)
//   * delta += alpha p of iteration l-1 is done by phase A of iteration l, which has p_{l-1} in hand anyway; phase B no
//     longer reads p or touches delta (the last iteration's update is folded into k_gn_update)     (-12 B read)
// Phase A': reads p3 r3 M^-1_A cs2 flags delta3, writes p3 Ap3 delta3 (85 B); phase B': reads r3 Ap3 M^-1_A flags, writes
// r3 (41 B).
template <int RB, bool LEAN>
__device__ __forceinline__ void pcg_a_march_body(const PlanDev& pd, int l, int stripsX, int chunksY, int chunk8)
{
    constexpr int LW = TILE_X + 2, RROWS = 16;                    // ring: 4 blocks x 4 rows
    __shared__ float2 sP[RROWS][LW];
    __shared__ float2 sC[RROWS][LW];
    __shared__ float sA[RROWS][LW];
    __shared__ unsigned char sF[RROWS][TILE_X];
    struct NoLut {};                                              // nothing to fill or look up: a use outside LEAN does not compile
    __shared__ std::conditional_t<LEAN, MoLut, NoLut> mo;         // the table is in the LEAN instance's LDS only
    int sx, cy, b;
    unsigned lb;
    const bool has_strip = xcd_tile(stripsX, chunksY, chunk8, sx, cy, b, lb);
    const unsigned nlb = 8u * (unsigned)chunk8;
    double* const sigma_l = red_slot(pd, b, 2 * l + 1);
    // the tag of this launch's granules (order-fixed sum at the end): fetched now, used after the march
    const unsigned rtag = red_tag(pd, b, lb);
    if (!has_strip) { block_reduce_fixed<1>(pd, b, lb, nlb, 0.0, 0.0, sigma_l, nullptr, rtag); return; }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int W = pd.W, H = pd.H;
    const size_t gb = (size_t)b * pd.N;
    const int x = sx * TILE_X + lane;
    const int ybase = cy * (4 * RB);
    const int nblk = min(RB, (H - ybase + 3) >> 2);               // blocks this workgroup owns
    const uint8_t* tact = pd.tileact + (size_t)b * pd.tilesX * pd.tilesY + sx;
    const int tyb = ybase >> 2;                                   // tile row of block 0
    auto active = [&](int blk) {                                  // does block blk (-1 .. nblk) hold an active vertex?
        const int ty = tyb + blk;
        return ty >= 0 && ty < pd.tilesY && tact[(size_t)ty * pd.tilesX] != 0;
    };
    // anything to do at all?  (uniform: tileact is per tile)
    {
        bool any = false;
        for (int k = 0; k < nblk; ++k) any = any || active(k);
        if (!any) { block_reduce_fixed<1>(pd, b, lb, nlb, 0.0, 0.0, sigma_l, nullptr, rtag); return; }
    }
    const Slot sl = pd.slots[b];
    if constexpr (LEAN) mo.fill(sl, threadIdx.x);
    const PBuf pin = p_in(pd, l), pout = p_out(pd, l);
    float beta = 0.f, alpha_prev = 0.f;                           // (LEAN: read AFTER the first stages' loads have been issued: below)
    if constexpr (!LEAN) beta = pcg_beta(pd, b, l);
    // ---- staging of one block row per wavefront: loads (registers) ... later: p_l = z + beta p_{l-1} -> ring --------
    // v = what z is formed from: z itself, or (LEAN) r with M^-1_A in m and the flags; h* = the same for the halo column.
    // dO, dA, mA, hmA and hf are loaded and read under LEAN only: registers the other instance never holds (its VGPR
    // count in the code object's metadata, 72, is the check: tools/loop_diff.py)
    struct Stage {
        float2 pO, vO, cs, hpO, hvO, hcs, dO;
        float pA, vA, mA, hpA, hvA, hmA, dA;
        unsigned f, hf;
        int i, hcol, hi;        // own vertex index (-1: nothing to stage), halo column cell (-1: none) and vertex index
        bool owned;
    };
    auto issue = [&](int blk) {
        Stage s;
        s.i = -1; s.hcol = -1; s.hi = -1; s.f = 0u; s.hf = 0u; s.owned = blk >= 0 && blk < nblk;
        s.pO = s.vO = s.cs = s.hpO = s.hvO = s.hcs = s.dO = make_float2(0.f, 0.f);
        s.pA = s.vA = s.mA = s.hpA = s.hvA = s.hmA = s.dA = 0.f;
        const int y = ybase + 4 * blk + w;
        // block -1 contributes its last row only (halo above), block nblk its first row only (halo below)
        const bool row_wanted = blk <= nblk && (blk >= 0 || w == 3) && (blk < nblk || w == 0);
        if (!row_wanted || y < 0 || y >= H || !active(blk)) return s;
        if (x < W) {
            s.i = x + W * y;
            s.f = pd.flags[gb + s.i];
            s.pO = pin.O[gb + s.i]; s.pA = pin.A[gb + s.i]; s.cs = pd.cs[gb + s.i];
            if (l > 0) {
                if constexpr (LEAN) {
                    s.vO = pd.rO[gb + s.i]; s.vA = pd.rA[gb + s.i]; s.mA = pd.preA[gb + s.i];
                    if (s.owned) { s.dO = pd.deltaO[gb + s.i]; s.dA = pd.deltaA[gb + s.i]; }
                } else {
                    s.vO = pd.zO[gb + s.i]; s.vA = pd.zA[gb + s.i];
                }
            }
            // halo columns: the strip's left neighbour column by lane 0, the right one by the last in-image lane
            if (lane == 0 && x > 0) { s.hi = s.i - 1; s.hcol = 0; }
            if ((lane == TILE_X - 1 || x == W - 1) && x + 1 < W) { s.hi = s.i + 1; s.hcol = lane + 2; }
            if (s.hi >= 0) {
                s.hpO = pin.O[gb + s.hi]; s.hpA = pin.A[gb + s.hi]; s.hcs = pd.cs[gb + s.hi];
                if (l > 0) {
                    if constexpr (LEAN) { s.hf = pd.flags[gb + s.hi]; s.hvO = pd.rO[gb + s.hi]; s.hvA = pd.rA[gb + s.hi]; s.hmA = pd.preA[gb + s.hi]; }
                    else { s.hvO = pd.zO[gb + s.hi]; s.hvA = pd.zA[gb + s.hi]; }
                }
            }
        }
        return s;
    };
    // p_l = z + beta p_{l-1};  LEAN: z = M^-1 r first, as phase B formed it
    auto direction = [&](float2& pO, float& pA, float2 vO, float vA, float mA, unsigned f) {
        if (l <= 0) return;
        if constexpr (LEAN) {
            const float m = mo.of(f);
            vO = make_float2(m * vO.x, m * vO.y);
            vA = mA * vA;
        }
        next_dir(pO, pA, vO, vA, beta);
    };
    auto finish = [&](int blk, const Stage& s) {
        if (s.i < 0) return;
        const int r = ((blk & 3) << 2) | w;
        float2 pO = s.pO;
        float pA = s.pA;
        if constexpr (LEAN) {
            if (l > 0 && s.owned && (s.f & F_ACT)) {                 // delta += alpha_{l-1} p_{l-1}
                pd.deltaO[gb + s.i] = make_float2(fmaf(alpha_prev, pO.x, s.dO.x), fmaf(alpha_prev, pO.y, s.dO.y));
                pd.deltaA[gb + s.i] = fmaf(alpha_prev, pA, s.dA);
            }
        }
        direction(pO, pA, s.vO, s.vA, s.mA, s.f);
        sP[r][lane + 1] = pO; sA[r][lane + 1] = pA; sC[r][lane + 1] = s.cs;
        sF[r][lane] = (unsigned char)s.f;
        if (s.owned && (s.f & F_ACT)) { pout.O[gb + s.i] = pO; pout.A[gb + s.i] = pA; }
        if (s.hcol >= 0) {
            float2 hO = s.hpO;
            float hA = s.hpA;
            direction(hO, hA, s.hvO, s.hvA, s.hmA, s.hf);
            sP[r][s.hcol] = hO; sA[r][s.hcol] = hA; sC[r][s.hcol] = s.hcs;
        }
    };
    // ---- prologue: halo row above, blocks 0 and 1 -------------------------------------------------------------------
    {
        const Stage a = issue(-1), c0 = issue(0), c1 = issue(1);
        if constexpr (LEAN) {
            // the loads of the first three stages have gone out; the three scalars (two dependent round trips each: shards,
            // then nothing else) are fetched while they fly -- beta and alpha are needed only when a stage is finished
            if (l > 0) {
                const float rhoNew = pcg_scalar(pd, b, 2 * l);
                const float rhoOld = pcg_scalar(pd, b, 2 * l - 2);
                const float sigOld = pcg_scalar(pd, b, 2 * l - 1);
                beta = guarded_ratio(rhoNew, rhoOld);
                alpha_prev = guarded_ratio(rhoOld, sigOld);       // alpha of iteration l - 1
            }
            __syncthreads();                                      // mo
        }
        finish(-1, a); finish(0, c0); finish(1, c1);
    }
    __syncthreads();
    const float wr2 = sl.wr * sl.wr, wf2 = sl.wf * sl.wf;
    double d = 0.0;
    // A block's Ap is stored one block late, the last block's after the workgroup's ticket has been taken (red_arrive:
    // a ticket behind streaming stores comes back only when they have drained)
    float2 pendO = make_float2(0.f, 0.f);
    float pendA = 0.f;
    int pendI = -1;
    // (LEAN, two stages of loads in flight -- block k + 3 issued while block k is computed -- measured no faster: 38.7 vs 38.3 us
    //  at 1920x1080 mask == 0: the phase is not bound by the latency of a stage's loads)
    for (int k = 0; k < nblk; ++k) {
        const Stage nx = issue(k + 2);                            // (block nblk: the halo row below; beyond: nothing)
        if (pendI >= 0) { pd.ApO[gb + pendI] = pendO; pd.ApA[gb + pendI] = pendA; pendI = -1; }
        const int y = ybase + 4 * k + w;
        if (active(k) && x < W && y < H) {
            const int r = ((k & 3) << 2) | w, ru = (r + RROWS - 1) & (RROWS - 1), rd = (r + 1) & (RROWS - 1);
            const unsigned f = sF[r][lane];
            if (f & F_ACT) {
                const int c = lane + 1;
                const float2 pO = sP[r][c];
                const float pA = sA[r][c];
                const float2 csi = sC[r][c];
                float ax = 0.f, ay = 0.f, aa = 0.f;
                if (f & F_E0) jtj_edge_grid<0>(csi, pO, pA, sC[r][c + 1], sP[r][c + 1], sA[r][c + 1], wr2, ax, ay, aa);
                if (f & F_E1) jtj_edge_grid<1>(csi, pO, pA, sC[r][c - 1], sP[r][c - 1], sA[r][c - 1], wr2, ax, ay, aa);
                if (f & F_E2) jtj_edge_grid<2>(csi, pO, pA, sC[rd][c], sP[rd][c], sA[rd][c], wr2, ax, ay, aa);
                if (f & F_E3) jtj_edge_grid<3>(csi, pO, pA, sC[ru][c], sP[ru][c], sA[ru][c], wr2, ax, ay, aa);
                if (f & F_FIT) {
                    ax = fmaf(wf2, pO.x, ax);
                    ay = fmaf(wf2, pO.y, ay);
                }
                pendI = x + W * y;
                pendO = make_float2(ax, ay);
                pendA = aa;
                d += (double)dot3(pO.x, pO.y, pA, ax, ay, aa);
            }
        }
        finish(k + 2, nx);
        __syncthreads();
    }
    const RedTicket rt = red_arrive<1>(pd, b, lb, nlb, d, 0.0, rtag);
    if (pendI >= 0) { pd.ApO[gb + pendI] = pendO; pd.ApA[gb + pendI] = pendA; }
    red_finish<1>(pd, b, rt, sigma_l, nullptr);
}

template <int RB>
__global__ __launch_bounds__(256) void k_pcg_a_march(PlanDev pd, int l, int stripsX, int chunksY, int chunk8)
{
    pcg_a_march_body<RB, false>(pd, l, stripsX, chunksY, chunk8);
}

#ifndef ARAP_MARCH2_WAVES
#define ARAP_MARCH2_WAVES 1
#endif
template <int RB>
__global__ __launch_bounds__(256, ARAP_MARCH2_WAVES) void k_pcg_a_march2(PlanDev pd, int l, int stripsX, int chunksY, int chunk8)
{
    pcg_a_march_body<RB, true>(pd, l, stripsX, chunksY, chunk8);
}

// Phase B of the lean schedule: r -= alpha Ap; rho' = (M^-1 r) . r.  Four consecutive vertices per lane, 16-byte accesses.
__global__ __launch_bounds__(256) void k_pcg_b4_r(PlanDev pd, int l)
{
    __shared__ MoLut mo;
    const int b = blockIdx.y;
    const unsigned rtag = red_tag(pd, b, blockIdx.x);
    const int q = blockIdx.x * 256 + threadIdx.x;
    const int nq = pd.N >> 2;
    const size_t gb = (size_t)b * pd.N;
    mo.fill(pd.slots[b], threadIdx.x);
    double d = 0.0;
    const unsigned fw = q < nq ? ((const unsigned*)(pd.flags + gb))[q] : 0u;
    const bool any_active = (fw & 0x20202020u) != 0u;
    float apo[8], r[8], apa[4], ma[4], ra[4];
    if (any_active) {                                       // the data loads go out first; alpha is fetched while they fly
        ld_quadO(apo, pd.ApO + gb, q); ld_quadO(r, pd.rO + gb, q);
        ld_quadA(apa, pd.ApA + gb, q); ld_quadA(ma, pd.preA + gb, q); ld_quadA(ra, pd.rA + gb, q);
    }
    __builtin_amdgcn_sched_barrier(0);
    const float alpha = pcg_alpha(pd, b, l);
    __syncthreads();
    if (any_active) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned fk = (fw >> (8 * k)) & 0xffu;
            if (!(fk & F_ACT)) continue;
            const float m = mo.of(fk);
            r[2 * k] = fmaf(-alpha, apo[2 * k], r[2 * k]);
            r[2 * k + 1] = fmaf(-alpha, apo[2 * k + 1], r[2 * k + 1]);
            ra[k] = fmaf(-alpha, apa[k], ra[k]);
            const float zx = m * r[2 * k], zy = m * r[2 * k + 1], za = ma[k] * ra[k];
            d += (double)dot3(zx, zy, za, r[2 * k], r[2 * k + 1], ra[k]);
        }
    }
    const RedTicket rt = red_arrive<1>(pd, b, blockIdx.x, gridDim.x, d, 0.0, rtag);
    if (any_active) { st_quadO(pd.rO + gb, q, r); st_quadA(pd.rA + gb, q, ra); }
    red_finish<1>(pd, b, rt, red_slot(pd, b, 2 * l + 2), nullptr);
}

// Phase B (k_pcg_b4's update, four consecutive vertices per lane, 16-byte accesses) without the z and preO reads.
// grid = (ceil(N/4/256), frames), block = 256.  Gauss-Newton plans with N % 4 == 0 only.
__global__ __launch_bounds__(256) void k_pcg_b4_lean(PlanDev pd, int l)
{
    __shared__ MoLut mo;
    const int b = blockIdx.y;
    const unsigned rtag = red_tag(pd, b, blockIdx.x);
    const int q = blockIdx.x * 256 + threadIdx.x;          // quad index
    const int nq = pd.N >> 2;
    const size_t gb = (size_t)b * pd.N;
    mo.fill(pd.slots[b], threadIdx.x);
    const PBuf p = p_out(pd, l);
    const float alpha = pcg_alpha(pd, b, l);
    __syncthreads();
    double d = 0.0;
    const unsigned fw = q < nq ? ((const unsigned*)(pd.flags + gb))[q] : 0u;      // 4 flag bytes
    const bool any_active = (fw & 0x20202020u) != 0u;
    float po[8], apo[8], dl[8], r[8], z[8], pa[4], apa[4], ma[4], dla[4], ra[4], za[4];
    if (any_active) {
        ld_quadO(po, p.O + gb, q); ld_quadO(apo, pd.ApO + gb, q); ld_quadO(dl, pd.deltaO + gb, q); ld_quadO(r, pd.rO + gb, q);
        ld_quadA(pa, p.A + gb, q); ld_quadA(apa, pd.ApA + gb, q); ld_quadA(ma, pd.preA + gb, q);
        ld_quadA(dla, pd.deltaA + gb, q); ld_quadA(ra, pd.rA + gb, q);
        const bool all_active = (fw & 0x20202020u) == 0x20202020u;
        if (!all_active) { ld_quadO(z, pd.zO + gb, q); ld_quadA(za, pd.zA + gb, q); }      // an excluded vertex keeps whatever its z holds
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned fk = (fw >> (8 * k)) & 0xffu;
            if (!(fk & F_ACT)) continue;
            const float m = mo.of(fk);
            dl[2 * k] = fmaf(alpha, po[2 * k], dl[2 * k]);
            dl[2 * k + 1] = fmaf(alpha, po[2 * k + 1], dl[2 * k + 1]);
            dla[k] = fmaf(alpha, pa[k], dla[k]);
            r[2 * k] = fmaf(-alpha, apo[2 * k], r[2 * k]);
            r[2 * k + 1] = fmaf(-alpha, apo[2 * k + 1], r[2 * k + 1]);
            ra[k] = fmaf(-alpha, apa[k], ra[k]);
            z[2 * k] = m * r[2 * k];
            z[2 * k + 1] = m * r[2 * k + 1];
            za[k] = ma[k] * ra[k];
            d += (double)dot3(z[2 * k], z[2 * k + 1], za[k], r[2 * k], r[2 * k + 1], ra[k]);
        }
    }
    // the workgroup's share of rho_{l+1} goes out, and its ticket is taken, BEFORE the nine streaming stores below (the
    // ticket's return would otherwise wait for them to drain: arap_device.h, red_arrive)
    const RedTicket rt = red_arrive<1>(pd, b, blockIdx.x, gridDim.x, d, 0.0, rtag);
    if (any_active) {
        st_quadO(pd.deltaO + gb, q, dl); st_quadO(pd.rO + gb, q, r); st_quadO(pd.zO + gb, q, z);
        st_quadA(pd.deltaA + gb, q, dla); st_quadA(pd.rA + gb, q, ra); st_quadA(pd.zA + gb, q, za);
    }
    red_finish<1>(pd, b, rt, red_slot(pd, b, 2 * l + 2), nullptr);
}

}  // namespace arap
