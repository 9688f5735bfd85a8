// abi_mscore.h -- map scoring on caller-owned maps (ArapFlow_LabelScore, ArapFlow_MapScore, arap_mscore.h): the layout of
// the scratch both calls share, their argument checks and the enqueue of the launches a call asks for, none of the others.
#pragma once

// Scratch of one boundary match, whatever n: the two byte maps, the column distances (shared by the two transforms, which
// run one after the other) and the two squared distances, each aligned to 256 bytes
struct MScoreScratch { size_t a, b, g, da, db, total; };
static MScoreScratch mscore_scratch(uint64_t N)
{
    MScoreScratch L{};
    L.b = L.a + align_up(N, 256);
    L.g = L.b + align_up(N, 256);
    L.da = L.g + align_up(N, 256);
    L.db = L.da + align_up(N * 2, 256);
    L.total = L.db + align_up(N * 2, 256);
    return L;
}

static MScoreJob mscore_job(const void* gt, const void* est, const void* skip, void* out, unsigned W, unsigned H, unsigned n,
                            unsigned L)
{
    MScoreJob j{};
    j.gt = (const uint8_t*)gt; j.est = (const uint8_t*)est; j.skip = (const uint8_t*)skip;
    j.out = (unsigned long long*)out;
    j.N = W * H; j.n = n; j.L = L;
    j.vec = (((uintptr_t)gt | (uintptr_t)est | (uintptr_t)skip) & 15) == 0;
    return j;
}

// the grid of k_mscore_count: a block per 4096 pixels (a group of 16 per lane) and map up to MSCORE_BLOCKS blocks in all
static dim3 mscore_count_grid(unsigned N, unsigned n)
{
    const unsigned gy = std::min(n, 65535u);
    return dim3(std::min((N + 4095u) / 4096u, std::max(1u, (unsigned)MSCORE_BLOCKS / gy)), gy);
}

// one boundary match of map `i`: the sets of `key` (a label, or a threshold), both distance transforms, the count into out[0..3]
template <bool LABELS>
static void enqueue_mscore_match(Opt_State* st, const MScoreJob& j, unsigned i, unsigned key, int radius, char* scratch,
                                 unsigned long long* out, int W, int H)
{
    const MScoreScratch L = mscore_scratch(j.N);
    uint8_t *const A = (uint8_t*)(scratch + L.a), *const B = (uint8_t*)(scratch + L.b), *const g = (uint8_t*)(scratch + L.g);
    uint16_t *const dA = (uint16_t*)(scratch + L.da), *const dB = (uint16_t*)(scratch + L.db);
    const size_t base = (size_t)i * j.N;
    const dim3 grid((W + 63) / 64, (H + 3) / 4), block(64, 4), cols((W + SEG_COLS - 1) / SEG_COLS), colb(SEG_COLS, SEG_RUNS);
    SEG_LAUNCH(st, "k_mscore_sets", k_mscore_sets<LABELS>, grid, block, j.gt + base, j.est + base,
               j.skip ? j.skip + base : (const uint8_t*)nullptr, key, A, B, W, H);
    SEG_LAUNCH(st, "k_seg_cols", k_seg_cols, cols, colb, (const uint8_t*)A, g, radius, W, H);
    SEG_LAUNCH(st, "k_seg_rows", k_seg_rows, grid, block, (const uint8_t*)g, dA, radius, W, H);
    SEG_LAUNCH(st, "k_seg_cols", k_seg_cols, cols, colb, (const uint8_t*)B, g, radius, W, H);
    SEG_LAUNCH(st, "k_seg_rows", k_seg_rows, grid, block, (const uint8_t*)g, dB, radius, W, H);
    SEG_LAUNCH(st, "k_mscore_hits", k_mscore_hits, dim3(std::min((j.N + 255u) / 256u, (unsigned)MSCORE_BLOCKS)), dim3(256),
               (const uint8_t*)A, (const uint8_t*)B, (const uint16_t*)dA, (const uint16_t*)dB, out, j.N);
}

extern "C" {

// per pixel: 1 + 1 (the two sets) + 1 (column distance) + 2 + 2 (the two squared distances) = 7 bytes, whatever n, L and m
uint64_t ArapFlow_MapScoreScratchBytes(unsigned W, unsigned H)
{
    return sizes_ok(W, H, 1) ? mscore_scratch((uint64_t)W * H).total : 0;
}

int ArapFlow_LabelScore(Opt_State* st, unsigned W, unsigned H, unsigned n, unsigned L, unsigned radius, const void* gt,
                        const void* est, const void* skip, void* table, void* scratch)
{
    if (!st || !gt || !est || !table || !scratch || !sizes_ok(W, H, n)) return -1;
    if (L == 0 || L > 255 || radius > (unsigned)SEG_MAX_RADIUS) return -1;
    const uint64_t all = (uint64_t)n * W * H, bytes = (uint64_t)n * (L + 1) * LSCORE_FIELDS * 8;
    const std::pair<const void*, uint64_t> bufs[] = {{table, bytes}, {scratch, mscore_scratch((uint64_t)W * H).total},
                                                     {gt, all}, {est, all}, {skip, all}};
    if (buffers_overlap(bufs, 2, 5)) return -1;
    const MScoreJob j = mscore_job(gt, est, skip, table, W, H, n, L);
    HC(hipMemsetAsync(table, 0, bytes, st->stream));
    SEG_LAUNCH(st, "k_mscore_labels", k_mscore_count<true>, mscore_count_grid(j.N, n), dim3(256), j);
    for (unsigned i = 0; i < n; ++i)
        for (unsigned k = 1; k <= L; ++k)
            enqueue_mscore_match<true>(st, j, i, k, (int)radius, (char*)scratch,
                                       j.out + ((size_t)i * (L + 1) + k) * LSCORE_FIELDS + 3, (int)W, (int)H);
    return (int)hipGetLastError();
}

int ArapFlow_MapScore(Opt_State* st, unsigned W, unsigned H, unsigned n, const void* gt, const void* est, const void* skip,
                      unsigned m, const unsigned* thr, unsigned radius, void* hist, void* match, void* scratch)
{
    if (!st || !gt || !est || !hist || !sizes_ok(W, H, n)) return -1;
    if (m > (unsigned)MSCORE_MAX_THR || radius > (unsigned)SEG_MAX_RADIUS) return -1;
    if (m && (!thr || !match || !scratch)) return -1;
    for (unsigned k = 0; k < m; ++k)
        if (thr[k] == 0 || thr[k] > 255) return -1;
    const uint64_t all = (uint64_t)n * W * H, hbytes = (uint64_t)n * MSCORE_HIST_WORDS * 8, mbytes = (uint64_t)n * m * 4 * 8;
    const std::pair<const void*, uint64_t> bufs[] = {{hist, hbytes}, {m ? match : nullptr, mbytes},
                                                     {m ? scratch : nullptr, mscore_scratch((uint64_t)W * H).total},
                                                     {gt, all}, {est, all}, {skip, all}};
    if (buffers_overlap(bufs, 3, 6)) return -1;
    const MScoreJob j = mscore_job(gt, est, skip, hist, W, H, n, 0);
    HC(hipMemsetAsync(hist, 0, hbytes, st->stream));
    if (m) HC(hipMemsetAsync(match, 0, mbytes, st->stream));
    if (st->mscore_plain) SEG_LAUNCH(st, "k_mscore_hist", (k_mscore_count<false, true>), mscore_count_grid(j.N, n), dim3(256), j);
    else SEG_LAUNCH(st, "k_mscore_hist", k_mscore_count<false>, mscore_count_grid(j.N, n), dim3(256), j);
    for (unsigned i = 0; i < n; ++i)
        for (unsigned k = 0; k < m; ++k)
            enqueue_mscore_match<false>(st, j, i, thr[k], (int)radius, (char*)scratch,
                                        (unsigned long long*)match + ((size_t)i * m + k) * 4, (int)W, (int)H);
    return (int)hipGetLastError();
}

}  // extern "C"
