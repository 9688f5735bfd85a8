// abi_seg.h -- the segment maps of a pair on caller-owned images (ArapFlow_SegMaps, arap_seg.h): the layout of the call's
// scratch buffer, its argument checks and the enqueue of the passes a call asks for, none of the others.
#pragma once

static_assert(SEG_MAX_RADIUS == ARAPFLOW_SEG_MAX_RADIUS && SEG_MAX_RADIUS + 1 <= 255, "the column distance is a byte");

// Scratch of one call: the key image, the full flow of the frame at work, the boundary map of a frame whose map is no
// output, the column distances, each aligned to 256 bytes, and the rasteriser's WarpJob in a last 256 bytes
struct SegScratch { size_t key, flow, mb, g, job, total; };
static SegScratch seg_scratch(uint64_t W, uint64_t H)
{
    const uint64_t N = W * H;
    SegScratch L{};
    L.flow = L.key + align_up(N * 8, 256);
    L.mb = L.flow + align_up(N * 8, 256);
    L.g = L.mb + align_up(N, 256);
    L.job = L.g + align_up(N, 256);
    L.total = L.job + 256;
    return L;
}

static bool seg_sizes_ok(unsigned W, unsigned H, unsigned n)
{
    return W != 0 && H != 0 && n != 0 && n <= 255 && (uint64_t)W * H < (1ull << 31);
}

// a launch on the state's stream; between two events, under the kernel's own name, when the state collects per-kernel
// times (ArapFlow_SetKernelTiming): what tells a caller which passes a call ran
#define SEG_LAUNCH(st_, kname_, kern, grid, blk, ...)                                        \
    do {                                                                                    \
        if ((st_)->timing) {                                                                \
            KernelTimer::Rec r_;                                                            \
            r_.name = kname_;                                                               \
            HC(hipEventCreate(&r_.a)); HC(hipEventCreate(&r_.b));                           \
            HC(hipEventRecord(r_.a, (st_)->stream));                                        \
            hipLaunchKernelGGL(kern, grid, blk, 0, (st_)->stream, __VA_ARGS__);             \
            HC(hipEventRecord(r_.b, (st_)->stream));                                        \
            (st_)->ktimer.recs.push_back(r_);                                               \
        } else {                                                                            \
            hipLaunchKernelGGL(kern, grid, blk, 0, (st_)->stream, __VA_ARGS__);             \
        }                                                                                   \
    } while (0)

// the passes behind one frame's full flow at `F`: the boundary map into `mb` (the caller's, or scratch) and, when asked,
// the distance
static void enqueue_seg_frame(Opt_State* st, const float2* F, float tau2, int radius, uint8_t* mb, uint8_t* g, void* dist,
                              int W, int H)
{
    const dim3 grid((W + 63) / 64, (H + 3) / 4), block(64, 4);
    SEG_LAUNCH(st, "k_seg_jump", k_seg_jump, grid, block, F, tau2, mb, W, H);
    if (!dist) return;
    SEG_LAUNCH(st, "k_seg_cols", k_seg_cols, dim3((W + SEG_COLS - 1) / SEG_COLS), dim3(SEG_COLS, SEG_RUNS), (const uint8_t*)mb, g, radius, W, H);
    SEG_LAUNCH(st, "k_seg_rows", k_seg_rows, grid, block, (const uint8_t*)g, (uint16_t*)dist, radius, W, H);
}

extern "C" {

// per pixel: 8 (key) + 8 (full flow) + 1 (boundary map) + 1 (column distance) = 18 bytes, however many layers
uint64_t ArapFlow_SegMapsScratchBytes(unsigned W, unsigned H, unsigned n)
{
    return seg_sizes_ok(W, H, n) ? seg_scratch(W, H).total : 0;
}

int ArapFlow_SegMaps(Opt_State* st, unsigned W, unsigned H, unsigned n, const void* masks_red, const void* flows,
                     const float M1[6], const float M2[6], float tau, unsigned radius, void* idx1, void* idx2, void* mb1,
                     void* mb2, void* dist1, void* dist2, void* scratch)
{
    if (!st || !masks_red || !flows || !scratch || !seg_sizes_ok(W, H, n)) return -1;
    if (!idx1 && !idx2 && !mb1 && !mb2 && !dist1 && !dist2) return -1;
    if (!std::isfinite(tau) || tau < 0.f || radius > (unsigned)SEG_MAX_RADIUS || (M1 != nullptr) != (M2 != nullptr)) return -1;
    float G[6], Ginv[6];
    const bool moving = M1 != nullptr;
    if (moving && ArapFlow_BackgroundMaps(M1, M2, G, Ginv) != 0) return -1;
    const uint64_t N64 = (uint64_t)W * H;
    const SegScratch L = seg_scratch(W, H);
    const std::pair<const void*, uint64_t> bufs[] = {{idx1, N64}, {idx2, N64}, {mb1, N64}, {mb2, N64}, {dist1, 2 * N64},
                                                     {dist2, 2 * N64}, {masks_red, n * N64}, {flows, n * N64 * 8},
                                                     {scratch, L.total}};
    if (buffers_overlap(bufs, 6, 9)) return -1;
    char* const c = (char*)scratch;
    float2* const F = (float2*)(c + L.flow);
    uint8_t* const g = (uint8_t*)(c + L.g);
    LayerSet ls{};
    ls.masks = (const uint8_t*)masks_red; ls.flows = (const float2*)flows; ls.n = (int)n;
    const float tau2 = tau * tau;
    const int iW = (int)W, iH = (int)H, N = iW * iH, r = (int)radius;
    const dim3 grid((W + 63) / 64, (H + 3) / 4), block(64, 4);
    const BgMap mG = moving ? bg_map(G) : BgMap{}, mGinv = moving ? bg_map(Ginv) : BgMap{};
    if (idx1 || mb1 || dist1) {
        float2* const f = mb1 || dist1 ? F : nullptr;
        if (moving) SEG_LAUNCH(st, "k_seg_index1", k_seg_index1<true>, grid, block, ls, mG, (uint8_t*)idx1, f, iW, iH);
        else SEG_LAUNCH(st, "k_seg_index1", k_seg_index1<false>, grid, block, ls, mG, (uint8_t*)idx1, f, iW, iH);
        if (f) enqueue_seg_frame(st, F, tau2, r, mb1 ? (uint8_t*)mb1 : (uint8_t*)(c + L.mb), g, dist1, iW, iH);
    }
    if (idx2 || mb2 || dist2) {
        float2* const f = mb2 || dist2 ? F : nullptr;
        WarpJob j{};
        j.key = (unsigned long long*)(c + L.key);
        j.bwd = f;
        WarpJob* dj = (WarpJob*)(c + L.job);
        HC(hipMemsetAsync(j.key, 0, (size_t)N * 8, st->stream));
        HC(hipMemcpyAsync(dj, &j, sizeof(j), hipMemcpyHostToDevice, st->stream));     // (pageable: staged before the call returns)
        SEG_LAUNCH(st, "k_layers_raster", k_layers_raster, dim3((W + 63) / 64, (H + 3) / 4, n), block, (const WarpJob*)dj, ls, iW, iH);
        if (f) SEG_LAUNCH(st, "k_layers_keys", k_layers_keys, dim3((unsigned)((N + 255) / 256)), dim3(256), (const WarpJob*)dj, ls, iW, N);
        if (moving) SEG_LAUNCH(st, "k_seg_index2", k_seg_index2<true>, grid, block, (const unsigned long long*)j.key, mGinv, (uint8_t*)idx2, f, iW, iH);
        else if (idx2) SEG_LAUNCH(st, "k_seg_index2", k_seg_index2<false>, grid, block, (const unsigned long long*)j.key, mGinv, (uint8_t*)idx2, f, iW, iH);
        // (the job has neither out_rgb nor out_mask: the resolve only leaves the keys clean, as every call of the family does)
        SEG_LAUNCH(st, "k_warp_resolve", k_warp_resolve, dim3((unsigned)((N + 255) / 256)), dim3(256), (const WarpJob*)dj, N);
        if (f) enqueue_seg_frame(st, F, tau2, r, mb2 ? (uint8_t*)mb2 : (uint8_t*)(c + L.mb), g, dist2, iW, iH);
    }
    return (int)hipGetLastError();
}

}  // extern "C"
