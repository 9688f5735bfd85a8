// abi_tscore.h -- track scoring and flow chaining (ArapFlow_TrackScore, arap_tscore.h; ArapFlow_ChainFlows,
// arap_chain.h): the argument checks and the one launch of each call.
#pragma once

extern "C" {

int ArapFlow_TrackScore(Opt_State* st, unsigned F, unsigned P, const void* gt_pos, const void* gt_occ, const void* est_pos,
                        const void* est_occ, float sx, float sy, void* table)
{
    if (!st || !gt_pos || !gt_occ || !est_pos || !est_occ || !table) return -1;
    if (P == 0 || P > (1u << 24) || F < 2 || F > (unsigned)TSCORE_MAX_FRAMES) return -1;
    if (!std::isfinite(sx) || !std::isfinite(sy) || !(sx > 0.f) || !(sy > 0.f)) return -1;
    const uint64_t all = (uint64_t)F * P, bytes = (uint64_t)F * TSCORE_CELLS * 8;
    const std::pair<const void*, uint64_t> bufs[] = {{table, bytes}, {gt_pos, all * 8}, {gt_occ, all}, {est_pos, all * 8},
                                                     {est_occ, all}};
    if (buffers_overlap(bufs, 1, 5)) return -1;
    TScoreJob j{};
    j.gt_pos = (const float2*)gt_pos; j.est_pos = (const float2*)est_pos;
    j.gt_occ = (const uint8_t*)gt_occ; j.est_occ = (const uint8_t*)est_occ;
    j.table = (unsigned long long*)table;
    j.F = F; j.P = P; j.sx = sx; j.sy = sy;
    // 256-point chunks, one a block, while that gives at most TSCORE_BLOCKS blocks, one a compute unit; beyond, 1024-point
    // chunks, and more than one a block beyond TSCORE_BLOCKS of those: what the table's atomics cost grows with the number of
    // blocks (at most 2^14 chunks of 1024: K <= 32 covers them in 512 blocks)
    const bool small = P <= (unsigned)TSCORE_BLOCKS * TSCORE_THREADS_SMALL;
    const unsigned threads = small ? TSCORE_THREADS_SMALL : TSCORE_THREADS, chunks = (P + threads - 1u) / threads;
    j.K = std::min(std::max((chunks + TSCORE_BLOCKS - 1u) / TSCORE_BLOCKS, 1u), (unsigned)TSCORE_MAX_CHUNKS);
    // the clear, then the one launch, through abi_seg.h's per-kernel timing macro (ArapFlow_SetKernelTiming sees it)
    HC(hipMemsetAsync(table, 0, bytes, st->stream));
    const dim3 grid((chunks + j.K - 1u) / j.K), block(threads);
    if (small) SEG_LAUNCH(st, "k_track_score", k_track_score<TSCORE_THREADS_SMALL>, grid, block, j);
    else SEG_LAUNCH(st, "k_track_score", k_track_score<TSCORE_THREADS>, grid, block, j);
    return (int)hipGetLastError();
}

int ArapFlow_ChainFlows(Opt_State* st, unsigned W, unsigned H, unsigned L, const void* flows, const void* bwd, unsigned P,
                        const void* points, void* out_pos, void* out_occ)
{
    if (!st || !flows || !points || !out_pos || !out_occ) return -1;
    if (L == 0 || L >= (unsigned)TSCORE_MAX_FRAMES || P == 0 || P > (1u << 24)) return -1;
    const uint64_t N = (uint64_t)W * H;
    if (N == 0 || N >= (1ull << 31)) return -1;
    const uint64_t all = (uint64_t)(L + 1) * P;
    const std::pair<const void*, uint64_t> bufs[] = {{out_pos, all * 8}, {out_occ, all}, {flows, L * N * 8}, {bwd, L * N * 8},
                                                     {points, (uint64_t)P * 8}};
    if (buffers_overlap(bufs, 2, 5)) return -1;
    ChainJob j{};
    j.flows = (const float2*)flows; j.bwd = (const float2*)bwd; j.points = (const float2*)points;
    j.pos = (float2*)out_pos; j.occ = (uint8_t*)out_occ;
    j.W = (int)W; j.H = (int)H; j.L = L; j.P = P;
    SEG_LAUNCH(st, "k_chain_flows", k_chain_flows, dim3((P + 255u) / 256u), dim3(256), j);
    return (int)hipGetLastError();
}

}  // extern "C"
