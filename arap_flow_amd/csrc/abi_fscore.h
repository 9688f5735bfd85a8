// abi_fscore.h -- the PSNR / integer-SSIM table of estimated frames (ArapFlow_FrameScore, arap_fscore.h): the argument
// checks, the launch shape and the one launch of a call.
#pragma once

extern "C" {

int ArapFlow_FrameScore(Opt_State* st, unsigned W, unsigned H, unsigned n, const void* ref, const void* est, const void* occ,
                        const void* dist, const void* skip, const void* obj, void* table, void* ssim)
{
    if (!st || !ref || !est || !table || !sizes_ok(W, H, n)) return -1;
    const uint64_t all = (uint64_t)n * W * H;
    const std::pair<const void*, uint64_t> bufs[] = {{table, (uint64_t)n * FSCORE_ROWS * FSCORE_FIELDS * 8}, {ssim, all * 4},
                                                     {ref, all * 3}, {est, all * 3}, {occ, all}, {dist, all * 2}, {skip, all},
                                                     {obj, all}};
    if (buffers_overlap(bufs, 2, 8)) return -1;
    FScoreJob j{};
    j.ref = (const uint8_t*)ref; j.est = (const uint8_t*)est;
    j.occ = (const uint8_t*)occ; j.dist = (const uint16_t*)dist; j.skip = (const uint8_t*)skip; j.obj = (const uint8_t*)obj;
    j.table = (unsigned long long*)table; j.ssim = (float*)ssim;
    j.W = W; j.H = H; j.n = n;
    j.tx = (W + FSCORE_TW - 1) / FSCORE_TW;
    const uint64_t tiles = (uint64_t)j.tx * ((H + FSCORE_TH - 1) / FSCORE_TH);           // < 2^31: a tile has a pixel
    j.tiles = (unsigned)tiles;
    j.vec = (((uintptr_t)ref | (uintptr_t)est) & 15) == 0;
    // a block per tile and pair up to FSCORE_BLOCKS blocks in all; a block loops over the rest (arap_fscore.h says why)
    const unsigned gy = std::min(n, 65535u), gx = (unsigned)std::min<uint64_t>(tiles, std::max(1u, (unsigned)FSCORE_BLOCKS / gy));
    // the clear, then the one launch, through abi_seg.h's per-kernel timing macro (ArapFlow_SetKernelTiming sees k_frame_score)
    HC(hipMemsetAsync(table, 0, bufs[0].second, st->stream));
    const dim3 grid(gx, gy), block(256);
    if (occ || dist || skip || obj) SEG_LAUNCH(st, "k_frame_score", k_frame_score<true>, grid, block, j);
    else SEG_LAUNCH(st, "k_frame_score", k_frame_score<false>, grid, block, j);
    return (int)hipGetLastError();
}

}  // extern "C"
