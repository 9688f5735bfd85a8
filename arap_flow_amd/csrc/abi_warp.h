// abi_warp.h -- the warp entry points on caller-owned images (ArapFlow_Warp / WarpEx / WarpStep / WarpLayers /
// WarpLayersStep): the layout of their scratch buffer, stated once for the size functions and for the code that carves
// it up, and the one enqueue of rasterise -> optional outputs -> resolve that the frame solver's warp shares.
// Then the point tracks of a sequence (ArapFlow_TrackPoints, arap_track.h), with a scratch layout of their own.
// Last, the moving-background post-pass (ArapFlow_BackgroundMaps / Background / BackgroundSeq, arap_bg.h), which needs no
// scratch, the random textures of a frame's objects (ArapFlow_Texture, arap_tex.h) and the motion-blurred frames
// (ArapFlow_BlurSchedule / BlurLayers, arap_blur.h), with a scratch layout of their own, and the relit frames
// (ArapFlow_LightTables / Relight, arap_light.h), which need only a 768-byte table.
#pragma once

// the optional outputs (arap_occ.h) of `njobs` jobs at `dj`, between k_warp_raster and k_warp_resolve.  `cells`:
// the jobs' cell arrays, `cell_bytes` contiguous bytes, zeroed here
static void enqueue_warp_outputs(hipStream_t stream, const WarpJob* dj, unsigned njobs, int W, int H, int outputs,
                                 void* cells, size_t cell_bytes)
{
    const int N = W * H;
    const dim3 g1((N + 255) / 256, 1, njobs);
    hipLaunchKernelGGL(k_warp_keys, g1, dim3(256), 0, stream, dj, W, N);
    if (!(outputs & ARAPFLOW_OUT_OCCLUSION)) return;
    HC(hipMemsetAsync(cells, 0, cell_bytes, stream));
    hipLaunchKernelGGL(k_occ_count, g1, dim3(256), 0, stream, dj, W, H, N);
    hipLaunchKernelGGL(k_occ_scan, dim3(1, 1, njobs), dim3(1024), 0, stream, dj, N);
    hipLaunchKernelGGL(k_occ_scatter, g1, dim3(256), 0, stream, dj, W, H, N);
    hipLaunchKernelGGL(k_occ_tri, dim3((W + 63) / 64, (H + 3) / 4, njobs), dim3(64, 4), 0, stream, dj, W, H);
}

// the fold diagnostics (arap_diag.h) of `njobs` jobs at `dj`, anywhere after their fields are final.  `accs`: the jobs'
// accumulators, `acc_bytes` contiguous bytes, zeroed here; NULL when the jobs ask for the fold map alone
static void enqueue_warp_diag(hipStream_t stream, const WarpJob* dj, unsigned njobs, int W, int H, void* accs,
                              size_t acc_bytes)
{
    if (accs) HC(hipMemsetAsync(accs, 0, acc_bytes, stream));
    hipLaunchKernelGGL(k_warp_diag, dim3((W + 63) / 64, (H + 3) / 4, njobs), dim3(64, 4), 0, stream, dj, W, H);
    if (accs) hipLaunchKernelGGL(k_diag_finish, dim3((njobs + 63) / 64), dim3(64), 0, stream, dj, (int)njobs);
}

// Scratch of one warp job: the key image, then -- for the occlusion map (WARP_OCC) -- cell counts, ranks and bins, then
// the layered warp's owner image (WARP_OWNER), then the layered step's query points (WARP_PTS), each aligned to 256
// bytes, and the WarpJob itself in a last 256 bytes.
// Offsets from the start of the buffer; a part that is absent has zero bytes (its offset equals the next one's).
enum { WARP_OCC = 1, WARP_OWNER = 2, WARP_PTS = 4 };
struct WarpScratch { size_t key, cell, rank, bin, owner, pts, job, total; };
static WarpScratch warp_scratch(uint64_t W, uint64_t H, int parts)
{
    const uint64_t N = W * H;
    const bool occ = parts & WARP_OCC, own = parts & WARP_OWNER, pts = parts & WARP_PTS;
    WarpScratch L{};
    L.cell = L.key + align_up(N * 8, 256);
    L.rank = L.cell + (occ ? align_up(4 * (N + 1), 256) : 0);
    L.bin = L.rank + (occ ? align_up(4 * N, 256) : 0);
    L.owner = L.bin + (occ ? align_up(16 * N, 256) : 0);
    L.pts = L.owner + (own ? align_up(N, 256) : 0);
    L.job = L.pts + (pts ? align_up(16 * N, 256) : 0);
    L.total = L.job + 256;
    return L;
}

// The start of every call on caller-owned images: point the job (inputs and outputs filled in by the caller) at its
// scratch, clear the key image and -- `clear_cells`: the layered calls, when the occlusion map is asked; the
// single-layer chain clears them itself, in enqueue_warp_outputs, as it does for the frame solver -- the cell counts,
// upload the job.  Returns where the job is on the device.
static WarpJob* warp_job_begin(hipStream_t stream, WarpJob& j, const WarpScratch& L, void* scratch, size_t N,
                               bool clear_cells)
{
    char* c = (char*)scratch;
    j.key = (unsigned long long*)(c + L.key);
    if (L.rank != L.cell) { j.cell = (unsigned*)(c + L.cell); j.rank = (unsigned*)(c + L.rank); j.bin = (int4*)(c + L.bin); }
    WarpJob* dj = (WarpJob*)(c + L.job);
    HC(hipMemsetAsync(j.key, 0, N * 8, stream));
    if (clear_cells) HC(hipMemsetAsync(j.cell, 0, 4 * (N + 1), stream));
    HC(hipMemcpyAsync(dj, &j, sizeof(j), hipMemcpyHostToDevice, stream));
    return dj;
}

// rasterise `njobs` jobs at `dj`, write the optional outputs (ARAPFLOW_OUT_* bits) and, for jobs with a second field
// (`step`: arap_mid.h), the flow towards it, resolve
static void enqueue_warp(hipStream_t stream, const WarpJob* dj, unsigned njobs, int W, int H, int outputs, void* cells,
                         size_t cell_bytes, bool step = false)
{
    const int N = W * H;
    hipLaunchKernelGGL(k_warp_raster, dim3((W + 63) / 64, (H + 3) / 4, njobs), dim3(64, 4), 0, stream, dj, W, H);
    if (outputs) enqueue_warp_outputs(stream, dj, njobs, W, H, outputs, cells, cell_bytes);
    if (step) hipLaunchKernelGGL(k_warp_step, dim3((N + 255) / 256, 1, njobs), dim3(256), 0, stream, dj, W, N);
    hipLaunchKernelGGL(k_warp_resolve, dim3((N + 255) / 256, 1, njobs), dim3(256), 0, stream, dj, N);
}

// one single-layer warp of a flow field (and, with `flow_b`, the step towards a second one) with a scratch buffer of
// `L` bytes: the body of ArapFlow_Warp / WarpEx / WarpStep
static int warp_flow(Opt_State* st, unsigned W, unsigned H, const void* rgb, const void* mask_red, const void* flow,
                     const void* flow_b, void* out_rgb, void* out_mask, void* out_bwd, void* out_occ_bwd, void* out_occ,
                     void* out_step, void* scratch, const WarpScratch& L)
{
    WarpJob j{};
    j.flow_in = (const float2*)flow; j.flow_b = (const float2*)flow_b;
    j.rgb = (const uint8_t*)rgb; j.mask = (const uint8_t*)mask_red;
    j.out_rgb = (uint8_t*)out_rgb; j.out_mask = (uint8_t*)out_mask;
    j.bwd = (float2*)out_bwd; j.occ_bwd = (uint8_t*)out_occ_bwd; j.occ = (uint8_t*)out_occ;
    j.step = (float2*)out_step;
    const size_t N = (size_t)W * H;
    const WarpJob* dj = warp_job_begin(st->stream, j, L, scratch, N, false);
    const int outputs = (out_bwd || out_occ_bwd ? ARAPFLOW_OUT_BACKWARD : 0) | (out_occ ? ARAPFLOW_OUT_OCCLUSION : 0);
    enqueue_warp(st->stream, dj, 1, (int)W, (int)H, outputs, j.cell, 4 * (N + 1), out_step != nullptr);
    return (int)hipGetLastError();
}

// The layered chain, stated once:  k_layers_raster (layers placed by `raster`) -> `pixel_pass`, the call's own passes per
// pixel of the key image -> [k_occ_scan -> `scatter` -> k_layers_tri (layers placed by `query`)] -> k_warp_resolve.
// The bracket runs when the occlusion map is asked; by then the pixel pass has counted the query points into the cells.
// pixel_pass and scatter are called with the per-pixel grid.
template <class PixelPass, class Scatter>
static int enqueue_layers(hipStream_t stream, const WarpJob* dj, const LayerSet& raster, const LayerSet& query, unsigned W,
                          unsigned H, bool occ, PixelPass pixel_pass, Scatter scatter)
{
    const int N = (int)(W * H);
    const dim3 g1((unsigned)((N + 255) / 256)), g2((W + 63) / 64, (H + 3) / 4, (unsigned)raster.n);
    hipLaunchKernelGGL(k_layers_raster, g2, dim3(64, 4), 0, stream, dj, raster, (int)W, (int)H);
    pixel_pass(g1);
    if (occ) {
        hipLaunchKernelGGL(k_occ_scan, dim3(1, 1, 1), dim3(1024), 0, stream, dj, N);
        scatter(g1);
        hipLaunchKernelGGL(k_layers_tri, g2, dim3(64, 4), 0, stream, dj, query, (int)W, (int)H);
    }
    hipLaunchKernelGGL(k_warp_resolve, g1, dim3(256), 0, stream, dj, N);
    return (int)hipGetLastError();
}

// what the two layered calls ask of their arguments alike; the limits are the key's and the bin's field widths
// (arap_warp.h, arap_occ.h)
static bool layers_args_ok(const Opt_State* st, unsigned W, unsigned H, unsigned n, const void* rgb, const void* masks_red,
                           const void* flows, const void* out_rgb, const void* out_occ, const void* scratch)
{
    if (!st || !masks_red || !flows || !scratch || W == 0 || H == 0 || n == 0 || n > 255) return false;
    if (out_rgb && !rgb) return false;
    const uint64_t N = (uint64_t)W * H;
    return N < (1ull << 31) && !(out_occ && N > (1ull << 24));
}

// G = B^-1 o A of two affine maps, in double, rounded once to float; false when B's linear part has det == 0
static bool bg_compose(const float A[6], const float B[6], float G[6])
{
    const double a = B[0], b = B[1], d = B[3], e = B[4];
    const double det = a * e - b * d;
    if (det == 0.0) return false;
    const double ia = e / det, ib = -b / det, id = -d / det, ie = a / det;          // B^-1, linear part
    const double tx = (double)A[2] - (double)B[2], ty = (double)A[5] - (double)B[5];
    G[0] = (float)(ia * A[0] + ib * A[3]); G[1] = (float)(ia * A[1] + ib * A[4]); G[2] = (float)(ia * tx + ib * ty);
    G[3] = (float)(id * A[0] + ie * A[3]); G[4] = (float)(id * A[1] + ie * A[4]); G[5] = (float)(id * tx + ie * ty);
    return true;
}

static BgMap bg_map(const float m[6]) { return BgMap{m[0], m[1], m[2], m[3], m[4], m[5]}; }

extern "C" {

uint64_t ArapFlow_WarpScratchBytes(unsigned W, unsigned H) { return warp_scratch(W, H, 0).total; }

int ArapFlow_Warp(Opt_State* st, unsigned W, unsigned H, const void* rgb, const void* mask_red, const void* flow,
                  void* out_rgb, void* out_mask, void* scratch)
{
    if (!st || !mask_red || !flow || !out_mask || !scratch) return -1;
    return warp_flow(st, W, H, rgb, mask_red, flow, nullptr, out_rgb, out_mask, nullptr, nullptr, nullptr, nullptr, scratch,
                     warp_scratch(W, H, 0));
}

uint64_t ArapFlow_WarpExScratchBytes(unsigned W, unsigned H) { return warp_scratch(W, H, WARP_OCC).total; }

int ArapFlow_WarpEx(Opt_State* st, unsigned W, unsigned H, const void* rgb, const void* mask_red, const void* flow,
                    void* out_rgb, void* out_mask, void* out_bwd, void* out_occ_bwd, void* out_occ, void* scratch)
{
    if (!st || !mask_red || !flow || !out_mask || !scratch || W == 0 || H == 0) return -1;
    return warp_flow(st, W, H, rgb, mask_red, flow, nullptr, out_rgb, out_mask, out_bwd, out_occ_bwd, out_occ, nullptr,
                     scratch, warp_scratch(W, H, WARP_OCC));
}

int ArapFlow_WarpStep(Opt_State* st, unsigned W, unsigned H, const void* rgb, const void* mask_red, const void* flow_a,
                      const void* flow_b, void* out_rgb, void* out_mask, void* out_step)
{
    if (!st || !mask_red || !flow_a || !flow_b || !out_mask || !out_step || W == 0 || H == 0) return -1;
    if (out_rgb && !rgb) return -1;
    if ((uint64_t)W * H >= (1ull << 31)) return -1;                              // (the key's triangle index)
    HC(hipSetDevice(st->device));
    const WarpScratch L = warp_scratch(W, H, 0);
    void* scratch = nullptr;                 // the call owns its scratch: it returns when the outputs are written
    if (hipMalloc(&scratch, L.total) != hipSuccess) return (int)hipErrorOutOfMemory;
    const int rc = warp_flow(st, W, H, rgb, mask_red, flow_a, flow_b, out_rgb, out_mask, nullptr, nullptr, nullptr,
                             out_step, scratch, L);
    HC(hipStreamSynchronize(st->stream));
    HC(hipFree(scratch));
    return rc;
}

int ArapFlow_WarpDiag(Opt_State* st, unsigned W, unsigned H, const void* mask_red, const void* flow, void* out_fold,
                      ArapFlow_MeshStats* out_stats)
{
    if (!st || !mask_red || !flow || (!out_fold && !out_stats) || W == 0 || H == 0) return -1;
    if ((uint64_t)W * H >= (1ull << 31)) return -1;                              // (a vertex index in an int)
    HC(hipSetDevice(st->device));
    if (!st->diag && hipMalloc(&st->diag, 512) != hipSuccess) return (int)hipErrorOutOfMemory;
    WarpJob j{};
    j.flow_in = (const float2*)flow; j.mask = (const uint8_t*)mask_red;
    j.fold = (uint8_t*)out_fold;
    if (out_stats) { j.acc = (DiagAcc*)((char*)st->diag + 256); j.stats = out_stats; }
    WarpJob* dj = (WarpJob*)st->diag;
    HC(hipMemcpyAsync(dj, &j, sizeof(j), hipMemcpyHostToDevice, st->stream));     // (pageable: staged before the call returns)
    enqueue_warp_diag(st->stream, dj, 1, (int)W, (int)H, j.acc, sizeof(DiagAcc));
    return (int)hipGetLastError();
}

uint64_t ArapFlow_WarpLayersScratchBytes(unsigned W, unsigned H, unsigned n)
{
    (void)n;                                 // one key image and one joint binning, however many layers
    return warp_scratch(W, H, WARP_OCC | WARP_OWNER).total;
}

int ArapFlow_WarpLayers(Opt_State* st, unsigned W, unsigned H, unsigned n, const void* rgb, const void* masks_red,
                        const void* flows, void* out_rgb, void* out_mask, void* out_bwd, void* out_occ_bwd,
                        void* out_occ, void* scratch)
{
    if (!layers_args_ok(st, W, H, n, rgb, masks_red, flows, out_rgb, out_occ, scratch)) return -1;
    if (!out_rgb && !out_mask && !out_bwd && !out_occ_bwd && !out_occ) return -1;
    const WarpScratch L = warp_scratch(W, H, WARP_OCC | WARP_OWNER);
    WarpJob j{};
    j.rgb = (const uint8_t*)rgb;
    j.out_rgb = (uint8_t*)out_rgb; j.out_mask = (uint8_t*)out_mask;
    j.bwd = (float2*)out_bwd; j.occ_bwd = (uint8_t*)out_occ_bwd; j.occ = (uint8_t*)out_occ;
    LayerSet ls{};
    ls.masks = (const uint8_t*)masks_red; ls.flows = (const float2*)flows; ls.n = (int)n;
    ls.owner = (uint8_t*)scratch + L.owner;
    hipStream_t stream = st->stream;
    const int iW = (int)W, iH = (int)H, N = iW * iH;
    const WarpJob* dj = warp_job_begin(stream, j, L, scratch, (size_t)N, out_occ != nullptr);
    return enqueue_layers(stream, dj, ls, ls, W, H, out_occ != nullptr,
        [&](dim3 g1) {
            if (out_bwd || out_occ_bwd || out_occ) hipLaunchKernelGGL(k_layers_keys, g1, dim3(256), 0, stream, dj, ls, iW, N);
            if (out_occ) hipLaunchKernelGGL(k_layers_count, g1, dim3(256), 0, stream, dj, ls, iW, iH, N);
        },
        [&](dim3 g1) { hipLaunchKernelGGL(k_layers_scatter, g1, dim3(256), 0, stream, dj, ls, iW, iH, N); });
}

// per pixel: 8 (key) + 4 (cell) + 4 (rank) + 16 (bin) + 16 (query point) = 48 bytes, however many layers
uint64_t ArapFlow_WarpLayersStepScratchBytes(unsigned W, unsigned H, unsigned n)
{
    (void)n;
    return warp_scratch(W, H, WARP_OCC | WARP_PTS).total;
}

int ArapFlow_WarpLayersStep(Opt_State* st, unsigned W, unsigned H, unsigned n, const void* rgb, const void* masks_red,
                            const void* flows_a, const void* flows_b, void* out_rgb, void* out_mask, void* out_step,
                            void* out_occ, void* scratch)
{
    if (!layers_args_ok(st, W, H, n, rgb, masks_red, flows_a, out_rgb, out_occ, scratch) || !flows_b) return -1;
    if (!out_rgb && !out_mask && !out_step && !out_occ) return -1;
    const WarpScratch L = warp_scratch(W, H, WARP_OCC | WARP_PTS);
    WarpJob j{};
    j.rgb = (const uint8_t*)rgb;
    j.out_rgb = (uint8_t*)out_rgb; j.out_mask = (uint8_t*)out_mask;
    j.step = (float2*)out_step; j.occ = (uint8_t*)out_occ;
    int4* pts = (int4*)((char*)scratch + L.pts);
    LayerSet la{}, lb{};                     // the layers placed by a and by b: the same masks
    la.masks = lb.masks = (const uint8_t*)masks_red; la.n = lb.n = (int)n;
    la.flows = (const float2*)flows_a; lb.flows = (const float2*)flows_b;
    hipStream_t stream = st->stream;
    const int iW = (int)W, iH = (int)H, N = iW * iH;
    const WarpJob* dj = warp_job_begin(stream, j, L, scratch, (size_t)N, out_occ != nullptr);
    return enqueue_layers(stream, dj, la, lb, W, H, out_occ != nullptr,
        [&](dim3 g1) {
            if (out_step || out_occ)
                hipLaunchKernelGGL(k_lstep_step, g1, dim3(256), 0, stream, dj, la, lb.flows, pts, iW, iH, N);
        },
        [&](dim3 g1) { hipLaunchKernelGGL(k_lstep_scatter, g1, dim3(256), 0, stream, dj, pts, iW, iH, N); });
}

// Scratch of one track call: per state the cell counts, the ranks, the bins, the query points and a flag array for a
// caller that wants no occ, each block of T aligned parts contiguous; then the owners and the T WarpJobs.
struct TrackScratch { size_t cell, rank, bin, pts, occ, own, job, total, cell_stride, rank_stride, bin_stride, occ_stride; };
static TrackScratch track_scratch(uint64_t W, uint64_t H, uint64_t T, uint64_t P)
{
    const uint64_t N = W * H;
    TrackScratch L{};
    L.cell_stride = align_up(4 * (N + 1), 256);
    L.rank_stride = align_up(4 * P, 256);
    L.bin_stride = align_up(16 * P, 256);
    L.occ_stride = align_up(P, 256);
    L.rank = L.cell + T * L.cell_stride;
    L.bin = L.rank + T * L.rank_stride;
    L.pts = L.bin + T * L.bin_stride;
    L.occ = L.pts + align_up(T * 16 * P, 256);
    L.own = L.occ + T * L.occ_stride;
    L.job = L.own + align_up(sizeof(TrackOwner) * P, 256);
    L.total = L.job + align_up(T * sizeof(WarpJob), 256);
    return L;
}

// the limits are the bin's field widths (arap_occ.h) and the snapshot count of a sequence
static bool track_sizes_ok(unsigned W, unsigned H, unsigned T, unsigned P)
{
    if (W == 0 || H == 0 || T == 0 || T > ARAPFLOW_MAX_SNAPSHOTS + 1 || P == 0 || P > (1u << 24)) return false;
    return (uint64_t)W * H < (1ull << 31);
}

uint64_t ArapFlow_TrackPointsScratchBytes(unsigned W, unsigned H, unsigned T, unsigned P)
{
    return track_sizes_ok(W, H, T, P) ? track_scratch(W, H, T, P).total : 0;
}

int ArapFlow_TrackPoints(Opt_State* st, unsigned W, unsigned H, unsigned n, const void* masks_red, unsigned T,
                         const void* flows, unsigned P, const void* points, void* out_pos, void* out_occ, void* scratch)
{
    if (!st || !masks_red || !flows || !points || !scratch || n == 0 || n > 255 || !track_sizes_ok(W, H, T, P)) return -1;
    if (!out_pos && !out_occ) return -1;
    const TrackScratch L = track_scratch(W, H, T, P);
    char* c = (char*)scratch;
    WarpJob jobs[ARAPFLOW_MAX_SNAPSHOTS + 1] = {};
    for (unsigned s = 0; s < T; ++s) {
        WarpJob& j = jobs[s];
        j.occ = out_occ ? (uint8_t*)out_occ + (size_t)s * P : (uint8_t*)(c + L.occ + s * L.occ_stride);
        j.cell = (unsigned*)(c + L.cell + s * L.cell_stride);
        j.rank = (unsigned*)(c + L.rank + s * L.rank_stride);
        j.bin = (int4*)(c + L.bin + s * L.bin_stride);
    }
    TrackSet ts{};
    ts.masks = (const uint8_t*)masks_red; ts.flows = (const float2*)flows; ts.points = (const float2*)points;
    ts.pos = (float2*)out_pos;
    ts.own = (TrackOwner*)(c + L.own); ts.pts = (int4*)(c + L.pts);
    ts.n = (int)n; ts.P = (int)P;
    hipStream_t stream = st->stream;
    const WarpJob* dj = (const WarpJob*)(c + L.job);
    HC(hipMemsetAsync(c + L.cell, 0, T * L.cell_stride, stream));
    HC(hipMemcpyAsync(c + L.job, jobs, T * sizeof(WarpJob), hipMemcpyHostToDevice, stream));   // (pageable: staged before the call returns)
    const int iW = (int)W, iH = (int)H;
    const dim3 g1((P + 255) / 256), gT((P + 255) / 256, 1, T);
    hipLaunchKernelGGL(k_track_locate, g1, dim3(256), 0, stream, ts, iW, iH);
    hipLaunchKernelGGL(k_track_state, gT, dim3(256), 0, stream, dj, ts, iW, iH);
    hipLaunchKernelGGL(k_occ_scan, dim3(1, 1, T), dim3(1024), 0, stream, dj, iW * iH);
    hipLaunchKernelGGL(k_track_scatter, gT, dim3(256), 0, stream, dj, ts, iW, iH);
    hipLaunchKernelGGL(k_track_tri, dim3((W + 63) / 64, (H + 3) / 4, T * n), dim3(64, 4), 0, stream, dj, ts, iW, iH);
    return (int)hipGetLastError();
}

int ArapFlow_BackgroundMaps(const float M1[6], const float M2[6], float G[6], float Ginv[6])
{
    if (!M1 || !M2 || !G || !Ginv) return -1;
    for (int k = 0; k < 6; ++k)
        if (!std::isfinite(M1[k]) || !std::isfinite(M2[k])) return -1;
    const double d1 = (double)M1[0] * M1[4] - (double)M1[1] * M1[3], d2 = (double)M2[0] * M2[4] - (double)M2[1] * M2[3];
    if (d1 == 0.0 || d2 == 0.0) return -1;
    if (memcmp(M1, M2, 6 * sizeof(float)) == 0) {            // the same camera: the exact identity, nothing inverted
        const float I[6] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f};
        memcpy(G, I, sizeof(I));
        memcpy(Ginv, I, sizeof(I));
        return 0;
    }
    return bg_compose(M1, M2, G) && bg_compose(M2, M1, Ginv) ? 0 : -1;
}

int ArapFlow_Background(Opt_State* st, unsigned W, unsigned H, const void* bg, unsigned bgW, unsigned bgH, const float M1[6],
                        const float M2[6], const void* rgb1, const void* mask_red, const void* rgb2, const void* cover2,
                        const void* flow, const void* occ, const void* bwd, const void* occ_bwd, void* out_rgb1,
                        void* out_rgb2, void* flow_full, void* occ_full, void* bwd_full, void* occ_bwd_full)
{
    if (!st || !bg || !mask_red || !cover2 || W == 0 || H == 0 || bgW == 0 || bgH == 0) return -1;
    if ((uint64_t)W * H >= (1ull << 31) || bgW >= (1u << 31) || bgH >= (1u << 31)) return -1;
    if ((out_rgb1 && !rgb1) || (out_rgb2 && !rgb2) || (flow_full && !flow) || (occ_full && !occ) || (bwd_full && !bwd) ||
        (occ_bwd_full && !occ_bwd))
        return -1;
    const bool one = out_rgb1 || flow_full || occ_full, two = out_rgb2 || bwd_full || occ_bwd_full;
    if (!one && !two) return -1;
    float G[6], Ginv[6];
    if (ArapFlow_BackgroundMaps(M1, M2, G, Ginv) != 0) return -1;
    const BgPicture pic{(const uint8_t*)bg, (int)bgW, (int)bgH};
    const dim3 grid((W + 63) / 64, (H + 3) / 4), block(64, 4);
    if (one) {
        const BgSide s{(const uint8_t*)mask_red, (const uint8_t*)cover2, (const uint8_t*)rgb1, (const float2*)flow,
                       (const uint8_t*)occ, (uint8_t*)out_rgb1, (float2*)flow_full, (uint8_t*)occ_full, bg_map(M1), bg_map(G)};
        hipLaunchKernelGGL(k_bg_frame1, grid, block, 0, st->stream, s, pic, (int)W, (int)H);
    }
    if (two) {
        const BgSide s{(const uint8_t*)cover2, (const uint8_t*)mask_red, (const uint8_t*)rgb2, (const float2*)bwd,
                       (const uint8_t*)occ_bwd, (uint8_t*)out_rgb2, (float2*)bwd_full, (uint8_t*)occ_bwd_full, bg_map(M2),
                       bg_map(Ginv)};
        hipLaunchKernelGGL(k_bg_frame2, grid, block, 0, st->stream, s, pic, (int)W, (int)H);
    }
    return (int)hipGetLastError();
}

static_assert(BG_SEQ_MAX == ARAPFLOW_MAX_SNAPSHOTS + 2, "frame 1, every snapshot, frame 2");

int ArapFlow_BackgroundSeq(Opt_State* st, unsigned W, unsigned H, const void* bg, unsigned bgW, unsigned bgH, unsigned nframes,
                           const float* maps, const void* mask_red, const void* const* covers, const void* const* rgbs,
                           const void* const* flows, const void* const* occs, void* const* out_rgbs, void* const* out_flows,
                           void* const* out_occs)
{
    if (!st || !bg || !mask_red || !maps || !covers || W == 0 || H == 0 || bgW == 0 || bgH == 0) return -1;
    if (nframes < 2 || nframes > (unsigned)BG_SEQ_MAX) return -1;
    if ((uint64_t)W * H >= (1ull << 31) || bgW >= (1u << 31) || bgH >= (1u << 31)) return -1;
    auto at = [](auto* list, unsigned f) { return list ? list[f] : nullptr; };   // a null list: every entry null
    BgSeq seq{};
    bool any = false;
    for (unsigned f = 0; f < nframes; ++f) {
        const bool link = f + 1 < nframes;
        BgSide& s = seq.f[f];
        s.own = (const uint8_t*)(f ? covers[f] : mask_red);
        if (!s.own) return -1;
        s.rgb = (const uint8_t*)at(rgbs, f);
        s.out_rgb = (uint8_t*)at(out_rgbs, f);
        s.M = bg_map(maps + 6 * f);
        if (link) {
            s.other = (const uint8_t*)covers[f + 1];
            s.flow = (const float2*)at(flows, f);
            s.occ = (const uint8_t*)at(occs, f);
            s.out_flow = (float2*)at(out_flows, f);
            s.out_occ = (uint8_t*)at(out_occs, f);
            float G[6], Ginv[6];
            if (!s.other || ArapFlow_BackgroundMaps(maps + 6 * f, maps + 6 * (f + 1), G, Ginv) != 0) return -1;
            s.G = bg_map(G);
        }
        if ((s.out_rgb && !s.rgb) || (s.out_flow && !s.flow) || (s.out_occ && !s.occ)) return -1;
        any = any || s.out_rgb || s.out_flow || s.out_occ;
    }
    if (!any) return -1;
    const BgPicture pic{(const uint8_t*)bg, (int)bgW, (int)bgH};
    const dim3 grid((W + 63) / 64, (H + 3) / 4, nframes), block(64, 4);
    hipLaunchKernelGGL(k_bg_seq, grid, block, 0, st->stream, seq, pic, (int)W, (int)H);
    return (int)hipGetLastError();
}

static_assert(sizeof(TexLayer) == sizeof(ArapFlow_TexLayer) && sizeof(TexLayer) == 52 &&
              offsetof(TexLayer, m) == offsetof(ArapFlow_TexLayer, m) && offsetof(TexLayer, p0) == offsetof(ArapFlow_TexLayer, p0) &&
              offsetof(TexLayer, c0) == offsetof(ArapFlow_TexLayer, c0) && offsetof(TexLayer, c2) == offsetof(ArapFlow_TexLayer, c2),
              "the kernel reads the caller's table as it is");
static_assert(TEX_CHECKER == ARAPFLOW_TEX_CHECKER && TEX_BRICK == ARAPFLOW_TEX_BRICK && TEX_VORONOI == ARAPFLOW_TEX_VORONOI &&
              TEX_NOISE == ARAPFLOW_TEX_NOISE && TEX_WAVE == ARAPFLOW_TEX_WAVE && TEX_KINDS == ARAPFLOW_TEX_WAVE + 1, "kinds");

int ArapFlow_Texture(Opt_State* st, unsigned W, unsigned H, unsigned n, const void* rgb, const void* masks_red,
                     const ArapFlow_TexLayer* layers, void* out_rgb)
{
    if (!st || !rgb || !layers || !out_rgb || W == 0 || H == 0 || n == 0 || n > 255) return -1;
    const uint64_t N = (uint64_t)W * H;
    if (N >= (1ull << 31)) return -1;
    for (unsigned l = 0; l < n; ++l) {
        const ArapFlow_TexLayer& q = layers[l];
        if (q.kind >= TEX_KINDS || !std::isfinite(q.p0) || !std::isfinite(q.p1)) return -1;
        for (int k = 0; k < 6; ++k)
            if (!std::isfinite(q.m[k])) return -1;
    }
    auto overlaps = [&](const void* in, uint64_t bytes) {               // [in, in + bytes) and out_rgb's 3 N bytes
        const uintptr_t a = (uintptr_t)in, o = (uintptr_t)out_rgb;
        return in && a < o + 3 * N && o < a + bytes;
    };
    if (overlaps(rgb, 3 * N) || overlaps(masks_red, n * N)) return -1;
    HC(hipSetDevice(st->device));
    if (!st->tex && hipMalloc(&st->tex, 255 * sizeof(TexLayer)) != hipSuccess) return (int)hipErrorOutOfMemory;
    HC(hipMemcpyAsync(st->tex, layers, n * sizeof(TexLayer), hipMemcpyHostToDevice, st->stream));   // (pageable: staged before the call returns)
    hipLaunchKernelGGL(k_tex_fill, dim3((W + 63) / 64, (H + 3) / 4), dim3(64, 4), 0, st->stream, (const uint8_t*)rgb,
                       (const uint8_t*)masks_red, (const TexLayer*)st->tex, (int)n, (uint8_t*)out_rgb, (int)W, (int)H);
    return (int)hipGetLastError();
}

static_assert(BLUR_CHUNK == ARAPFLOW_BLUR_CHUNK && BLUR_MAX_SAMPLES == ARAPFLOW_MAX_BLUR_SAMPLES, "blur limits");

// Scratch of one blur call: min(samples, BLUR_CHUNK) key images, then -- when the samples need more than one chunk -- the
// carried sums, each aligned to 256 bytes
struct BlurScratch { size_t key, carry, total; };
static BlurScratch blur_scratch(uint64_t W, uint64_t H, uint64_t samples)
{
    const uint64_t N = W * H, g = samples < (uint64_t)BLUR_CHUNK ? samples : (uint64_t)BLUR_CHUNK;
    BlurScratch L{};
    L.carry = L.key + align_up(g * N * 8, 256);
    L.total = L.carry + (samples > (uint64_t)BLUR_CHUNK ? align_up(N * 8, 256) : 0);
    return L;
}

static bool blur_sizes_ok(unsigned W, unsigned H, unsigned n, unsigned samples)
{
    if (W == 0 || H == 0 || n == 0 || n > 255 || samples == 0 || samples > (unsigned)BLUR_MAX_SAMPLES) return false;
    return (uint64_t)W * H < (1ull << 31);
}

int ArapFlow_BlurSchedule(float centre, float shutter, unsigned samples, const float Ma[6], const float Mb[6], float* times,
                          float* maps)
{
    if (!times || samples == 0 || samples > (unsigned)BLUR_MAX_SAMPLES) return -1;
    if (!std::isfinite(centre) || !std::isfinite(shutter) || shutter < 0.f) return -1;
    if (maps) {
        if (!Ma || !Mb) return -1;
        for (int k = 0; k < 6; ++k)
            if (!std::isfinite(Ma[k]) || !std::isfinite(Mb[k])) return -1;
    }
    const bool still = maps && memcmp(Ma, Mb, 6 * sizeof(float)) == 0;       // the same camera: every sample uses Ma itself
    for (unsigned k = 0; k < samples; ++k) {
        const float t = (float)((double)centre + (double)shutter * (((double)k + 0.5) / (double)samples - 0.5));
        times[k] = t;
        if (!maps) continue;
        const float u = 1.0f - t;
        for (int i = 0; i < 6; ++i) maps[6 * k + i] = still ? Ma[i] : u * Ma[i] + t * Mb[i];
    }
    return 0;
}

// per pixel: 8 per sample of a chunk (at most 8 * ARAPFLOW_BLUR_CHUNK) + 8 when samples > ARAPFLOW_BLUR_CHUNK
uint64_t ArapFlow_BlurLayersScratchBytes(unsigned W, unsigned H, unsigned n, unsigned samples)
{
    return blur_sizes_ok(W, H, n, samples) ? blur_scratch(W, H, samples).total : 0;
}

int ArapFlow_BlurLayers(Opt_State* st, unsigned W, unsigned H, unsigned n, const void* rgb, const void* masks_red,
                        const void* flows_a, const void* flows_b, float centre, float shutter, unsigned samples,
                        const void* bg, unsigned bgW, unsigned bgH, const float Ma[6], const float Mb[6], void* out_rgb,
                        void* out_alpha, void* scratch)
{
    if (!st || !rgb || !masks_red || !flows_b || !scratch || (!out_rgb && !out_alpha)) return -1;
    if (!blur_sizes_ok(W, H, n, samples)) return -1;
    if (bg && (!Ma || !Mb || bgW == 0 || bgH == 0 || bgW >= (1u << 31) || bgH >= (1u << 31))) return -1;
    float times[BLUR_MAX_SAMPLES], maps[BLUR_MAX_SAMPLES * 6];
    if (ArapFlow_BlurSchedule(centre, shutter, samples, Ma, Mb, times, bg ? maps : nullptr) != 0) return -1;
    const uint64_t N = (uint64_t)W * H;
    const BlurScratch L = blur_scratch(W, H, samples);
    const std::pair<const void*, uint64_t> ins[] = {{rgb, 3 * N}, {masks_red, n * N}, {flows_a, n * N * 8}, {flows_b, n * N * 8},
                                                    {bg, 3ull * bgW * bgH}, {scratch, L.total}};
    const std::pair<const void*, uint64_t> outs[] = {{out_rgb, 3 * N}, {out_alpha, N}};
    for (const auto& o : outs)
        for (const auto& in : ins) {
            const uintptr_t a = (uintptr_t)in.first, b = (uintptr_t)o.first;
            if (in.first && o.first && a < b + o.second && b < a + in.second) return -1;
        }
    char* const c = (char*)scratch;
    BlurFrame f{};
    f.rgb = (const uint8_t*)rgb; f.masks = (const uint8_t*)masks_red;
    f.flows_a = (const float2*)flows_a; f.flows_b = (const float2*)flows_b;
    f.keys = (unsigned long long*)(c + L.key);
    f.carry = L.total != L.carry ? (ushort4*)(c + L.carry) : nullptr;
    f.out_rgb = (uint8_t*)out_rgb; f.out_alpha = (uint8_t*)out_alpha;
    f.bg = BgPicture{(const uint8_t*)bg, (int)bgW, (int)bgH};
    f.n = (int)n; f.samples = (int)samples;
    hipStream_t stream = st->stream;
    HC(hipMemsetAsync(f.keys, 0, L.carry - L.key, stream));
    const bool still = bg && memcmp(Ma, Mb, 6 * sizeof(float)) == 0;
    for (unsigned k0 = 0; k0 < samples; k0 += (unsigned)BLUR_CHUNK) {
        BlurChunk ch{};
        ch.g = (int)std::min(samples - k0, (unsigned)BLUR_CHUNK);          // the last chunk: what is left
        ch.first = k0 == 0; ch.last = k0 + (unsigned)ch.g == samples; ch.same_map = still;
        for (int s = 0; s < ch.g; ++s) {
            ch.t[s] = times[k0 + s];
            if (bg) ch.M[s] = bg_map(maps + 6 * (k0 + s));
        }
        hipLaunchKernelGGL(k_blur_raster, dim3((W + 63) / 64, (H + 3) / 4, n * (unsigned)ch.g), dim3(64, 4), 0, stream, f, ch,
                           (int)W, (int)H);
        hipLaunchKernelGGL(k_blur_accum, dim3((W + 63) / 64, (H + 3) / 4), dim3(64, 4), 0, stream, f, ch, (int)W, (int)H);
    }
    return (int)hipGetLastError();
}

static_assert(LIGHT_MAX_R == ARAPFLOW_LIGHT_MAX_R && LIGHT_MAX_SHIFT == ARAPFLOW_LIGHT_MAX_SHIFT, "light limits");

// the ranges of include/arap_opt.h, one test for ArapFlow_LightTables and ArapFlow_Relight
static bool light_frame_ok(const ArapFlow_LightFrame& q)
{
    for (float c : q.m)
        if (!std::isfinite(c)) return false;
    for (float g : q.gain)
        if (!std::isfinite(g) || !(g > 0.f)) return false;
    if (!std::isfinite(q.gamma) || !(q.gamma > 0.f)) return false;
    if (!std::isfinite(q.amp) || !(q.amp >= 0.f) || !(q.vig >= 0.f && q.vig <= 1.f)) return false;
    if (!std::isfinite(q.sigma0) || !(q.sigma0 >= 0.f) || !std::isfinite(q.sigma1) || !(q.sigma1 >= 0.f)) return false;
    if (q.sh_dx < -LIGHT_MAX_SHIFT || q.sh_dx > LIGHT_MAX_SHIFT || q.sh_dy < -LIGHT_MAX_SHIFT || q.sh_dy > LIGHT_MAX_SHIFT) return false;
    return q.sh_r >= 0 && q.sh_r <= LIGHT_MAX_R && q.sh_g >= 0 && q.sh_g <= 256;
}

int ArapFlow_LightTables(const ArapFlow_LightFrame* frame, unsigned W, unsigned H, uint8_t lut[3][256], float geom[3])
{
    if (!frame || !lut || !geom || W == 0 || H == 0 || (uint64_t)W * H >= (1ull << 31) || !light_frame_ok(*frame)) return -1;
    for (int c = 0; c < 3; ++c)
        for (int i = 0; i < 256; ++i) {
            const double t = (double)frame->gain[c] * pow((double)i / 255.0, (double)frame->gamma);
            lut[c][i] = (uint8_t)floor(255.0 * fmin(fmax(t, 0.0), 1.0) + 0.5);
        }
    const double cx = ((double)W - 1.0) / 2.0, cy = ((double)H - 1.0) / 2.0, r2 = cx * cx + cy * cy;
    geom[0] = (float)cx; geom[1] = (float)cy; geom[2] = r2 > 0.0 ? (float)(1.0 / r2) : 0.0f;
    return 0;
}

int ArapFlow_Relight(Opt_State* st, unsigned W, unsigned H, const void* rgb, const void* cover, int cover_is_mask,
                     const ArapFlow_LightFrame* frame, void* out_rgb)
{
    if (!st || !rgb || !frame || !out_rgb) return -1;
    uint8_t lut[3][256];
    float geom[3];
    if (ArapFlow_LightTables(frame, W, H, lut, geom) != 0) return -1;
    const bool shadow = frame->sh_g > 0;
    if (shadow && !cover) return -1;
    const uint64_t N = (uint64_t)W * H;
    auto overlaps = [&](const void* in, uint64_t bytes) {               // [in, in + bytes) and out_rgb's 3 N bytes
        const uintptr_t a = (uintptr_t)in, o = (uintptr_t)out_rgb;
        return in && a < o + 3 * N && o < a + bytes;
    };
    if (overlaps(rgb, 3 * N) || overlaps(cover, N)) return -1;
    LightParams q{};
    q.seed = frame->seed; q.m = bg_map(frame->m);
    q.amp = frame->amp; q.vig = frame->vig;
    q.cx = geom[0]; q.cy = geom[1]; q.inv_r2 = geom[2];
    q.sh_dx = frame->sh_dx; q.sh_dy = frame->sh_dy; q.sh_r = frame->sh_r; q.sh_g = frame->sh_g;
    q.sigma0 = frame->sigma0; q.sigma1 = frame->sigma1;
    HC(hipSetDevice(st->device));
    if (!st->light && hipMalloc(&st->light, sizeof(lut)) != hipSuccess) return (int)hipErrorOutOfMemory;
    HC(hipMemcpyAsync(st->light, lut, sizeof(lut), hipMemcpyHostToDevice, st->stream));   // (pageable: staged before the call returns)
    const dim3 grid((W + 63) / 64, (H + 3) / 4), block(64, 4);
    const auto kernel = !shadow ? k_relight<false, false> : cover_is_mask ? k_relight<true, true> : k_relight<true, false>;
    hipLaunchKernelGGL(kernel, grid, block, 0, st->stream, (const uint8_t*)rgb, (const uint8_t*)cover, (const uint8_t*)st->light,
                       q, (uint8_t*)out_rgb, (int)W, (int)H);
    return (int)hipGetLastError();
}

}  // extern "C"
