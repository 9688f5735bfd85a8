// abi_score.h -- the error table of an estimated flow against a pair (ArapFlow_FlowScore, arap_score.h): the argument
// checks, the launch shape that keeps a lane's counts within their bytes, and the one launch of a call.
#pragma once

// blocks per pair: one group of 4 pixels (one pixel where the buffers are not aligned for the group loads) per thread
// while that gives the device at most about eight blocks a compute unit over all pairs, more per thread beyond, and
// never more per thread than a lane's accumulators hold (SCORE_GROUP_ITERS, SCORE_PIXEL_ITERS)
static unsigned score_blocks(uint64_t N, unsigned n, bool vec)
{
    const uint64_t units = vec ? N / 4 : N, per = vec ? SCORE_GROUP_ITERS : SCORE_PIXEL_ITERS;
    const uint64_t one_each = (units + 255) / 256, target = std::max<uint64_t>(1, 2048 / n);
    const uint64_t least = (units + 256 * per - 1) / (256 * per);
    return (unsigned)std::max<uint64_t>(1, std::max(std::min(one_each, target), least));
}

extern "C" {

int ArapFlow_FlowScore(Opt_State* st, unsigned W, unsigned H, unsigned n, const void* gt, const void* est, const void* occ,
                       const void* dist, const void* skip, void* table, void* err)
{
    if (!st || !gt || !est || !table || !sizes_ok(W, H, n)) return -1;
    const uint64_t N = (uint64_t)W * H, all = n * N;
    const std::pair<const void*, uint64_t> bufs[] = {{table, (uint64_t)n * SCORE_ROWS * SCORE_FIELDS * 8}, {err, all * 4},
                                                     {gt, all * 8}, {est, all * 8}, {occ, all}, {dist, all * 2}, {skip, all}};
    if (buffers_overlap(bufs, 2, 7)) return -1;
    ScoreJob j{};
    j.gt = (const float2*)gt; j.est = (const float2*)est;
    j.occ = (const uint8_t*)occ; j.dist = (const uint16_t*)dist; j.skip = (const uint8_t*)skip;
    j.table = (unsigned long long*)table; j.err = (float*)err;
    j.N = (unsigned)N; j.n = n;
    j.vec = (((uintptr_t)gt | (uintptr_t)est | (uintptr_t)err) & 15) == 0 && ((uintptr_t)dist & 7) == 0 &&
            (((uintptr_t)occ | (uintptr_t)skip) & 3) == 0;
    // the clear, then the one launch, through abi_seg.h's per-kernel timing macro (ArapFlow_SetKernelTiming sees k_flow_score)
    HC(hipMemsetAsync(table, 0, bufs[0].second, st->stream));
    const dim3 grid(score_blocks(N, n, j.vec != 0), std::min(n, 65535u)), block(256);
    if (occ || dist || skip) SEG_LAUNCH(st, "k_flow_score", k_flow_score<true>, grid, block, j);
    else SEG_LAUNCH(st, "k_flow_score", k_flow_score<false>, grid, block, j);
    return (int)hipGetLastError();
}

}  // extern "C"
