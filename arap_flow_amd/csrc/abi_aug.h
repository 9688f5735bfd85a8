// abi_aug.h -- training batches (ArapFlow_AugmentTables, ArapFlow_AugmentPairs; arap_aug.h): the tables a sample's
// description gives, stated once for the host function, the device call, the twin and the tests; the argument checks;
// the per-sample device table the state owns; the one launch of a call.
#pragma once

static_assert(AUG_MAX_BATCH == ARAPFLOW_AUG_MAX_BATCH && AUG_MAX_ERASE == ARAPFLOW_AUG_MAX_ERASE, "augmentation limits");
static_assert(sizeof(ArapFlow_AugSample) == 160, "ArapFlow_AugSample layout");

// The per-frame pieces of the tables, shared by ArapFlow_AugmentTables and ArapFlow_ClipTables (abi_clip.h).
// a frame inside its ranges: a finite map, a finite gain and gamma > 0
static bool aug_frame_ok(const float T[6], const float gain[3], float gamma)
{
    for (int i = 0; i < 6; ++i)
        if (!std::isfinite(T[i])) return false;
    if (!std::isfinite(gamma) || !(gamma > 0.f)) return false;
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(gain[c]) || !(gain[c] > 0.f)) return false;
    return true;
}

// P = the inverse of T as a map, in double, each value rounded once; false (nothing written) where det(T) == 0
static bool aug_frame_inverse(const float T[6], float P[6])
{
    const double a = T[0], b = T[1], c = T[2], d = T[3], e = T[4], f = T[5];
    const double det = a * e - b * d;
    if (det == 0.0) return false;
    P[0] = (float)(e / det); P[1] = (float)(-b / det); P[2] = (float)((b * f - e * c) / det);
    P[3] = (float)(-d / det); P[4] = (float)(a / det); P[5] = (float)((d * c - a * f) / det);
    return true;
}

// a frame's tone table with the normalisation folded in, in double, each value rounded once
static void aug_frame_lut(const float gain[3], float gamma, const float scale[3], const float bias[3], float lut[3][256])
{
    for (int i = 0; i < 256; ++i) {
        const double p = pow((double)i / 255.0, (double)gamma);                  // (one pow for the three channels)
        for (int ch = 0; ch < 3; ++ch) {
            const double t = (double)gain[ch] * p;
            lut[ch][i] = (float)((255.0 * fmin(fmax(t, 0.0), 1.0)) * (double)scale[ch] + (double)bias[ch]);
        }
    }
}

// P2 and the two tone tables of a sample; false for a sample outside its ranges
static bool aug_tables(const ArapFlow_AugSample& s, const float scale[3], const float bias[3], float P2[6], float lut[2][3][256])
{
    if (!aug_frame_ok(s.T1, s.gain1, s.gamma1) || !aug_frame_ok(s.T2, s.gain2, s.gamma2)) return false;
    if (!aug_frame_inverse(s.T2, P2)) return false;
    aug_frame_lut(s.gain1, s.gamma1, scale, bias, lut[0]);
    aug_frame_lut(s.gain2, s.gamma2, scale, bias, lut[1]);
    return true;
}

extern "C" {

int ArapFlow_AugmentTables(const ArapFlow_AugSample* sample, const float scale[3], const float bias[3], float P2[6],
                           float lut[2][3][256])
{
    if (!sample || !scale || !bias || !P2 || !lut) return -1;
    return aug_tables(*sample, scale, bias, P2, lut) ? 0 : -1;
}

int ArapFlow_AugmentPairs(Opt_State* st, unsigned W, unsigned H, unsigned w, unsigned h, unsigned B, const void* rgb1,
                          const void* rgb2, const void* flow, const void* skip, const ArapFlow_AugSample* samples,
                          const float scale[3], const float bias[3], float tau, void* img1, void* img2, void* out_flow,
                          void* valid)
{
    if (!st || !samples || !scale || !bias || !(img1 || img2 || out_flow || valid)) return -1;
    if (W == 0 || H == 0 || w == 0 || h == 0 || B == 0 || B > (unsigned)AUG_MAX_BATCH || !(tau >= 0.f)) return -1;
    const uint64_t N = (uint64_t)W * H, n = (uint64_t)w * h;
    if (N >= (1ull << 31) || n >= (1ull << 31) || B * n >= (1ull << 31)) return -1;
    // an input no asked output needs is not read: it takes no part in the checks
    if (!img1) rgb1 = nullptr;
    if (!img2) rgb2 = nullptr;
    if (!out_flow && !valid) flow = skip = nullptr;
    if ((img1 && !rgb1) || (img2 && !rgb2) || ((out_flow || valid) && !flow)) return -1;
    const std::pair<const void*, uint64_t> bufs[] = {{img1, B * n * 12}, {img2, B * n * 12}, {out_flow, B * n * 8}, {valid, B * n},
                                                     {rgb1, B * N * 3}, {rgb2, B * N * 3}, {flow, B * N * 8}, {skip, B * N}};
    if (buffers_overlap(bufs, 4, 8)) return -1;
    std::vector<AugSampleDev> tab(B);
    for (unsigned i = 0; i < B; ++i) {
        const ArapFlow_AugSample& s = samples[i];
        AugSampleDev& t = tab[i];
        if (s.n_erase > (unsigned)AUG_MAX_ERASE || !aug_tables(s, scale, bias, t.P2, t.lut)) return -1;
        std::memcpy(t.T1, s.T1, sizeof(t.T1));
        std::memcpy(t.T2, s.T2, sizeof(t.T2));
        std::memcpy(t.fill, s.fill, sizeof(t.fill));
        t.n_erase = (int)s.n_erase;
        std::memcpy(t.erase, s.erase, sizeof(t.erase));
        t.pad[0] = t.pad[1] = 0;
    }
    HC(hipSetDevice(st->device));
    if (st->aug_cap < B) {                                  // (hipFree waits for the calls that still read the old table)
        if (st->aug) (void)hipFree(st->aug);
        st->aug = nullptr; st->aug_cap = 0;
        if (hipMalloc(&st->aug, B * sizeof(AugSampleDev)) != hipSuccess) return (int)hipErrorOutOfMemory;
        st->aug_cap = B;
    }
    // pageable: the runtime has copied `tab` away when this returns and writes the table in the stream's order; it does not
    // wait for the stream (tests/test_gpu_aug.py observes that).  One table per state: calls on one stream follow each other,
    // a caller who moves the state to another stream orders the two streams (data.AugmentLoader does)
    HC(hipMemcpyAsync(st->aug, tab.data(), B * sizeof(AugSampleDev), hipMemcpyHostToDevice, st->stream));
    AugJob j{};
    j.rgb1 = (const uint8_t*)rgb1; j.rgb2 = (const uint8_t*)rgb2; j.flow = (const float2*)flow; j.skip = (const uint8_t*)skip;
    j.tab = (const AugSampleDev*)st->aug;
    j.img1 = (float*)img1; j.img2 = (float*)img2; j.out_flow = (float*)out_flow; j.valid = (uint8_t*)valid;
    j.W = (int)W; j.H = (int)H; j.w = (int)w; j.h = (int)h;
    j.tiles_x = (int)((w + AUG_TILE_W - 1) / AUG_TILE_W);
    j.tau = tau;
    j.vec = w % AUG_PX == 0 && (((uintptr_t)img1 | (uintptr_t)img2 | (uintptr_t)out_flow) & 15) == 0 && ((uintptr_t)valid & 3) == 0;
    const dim3 grid((unsigned)j.tiles_x * ((h + AUG_TILE_H - 1) / AUG_TILE_H), 1, B), block(256);
    // a tap's three bytes in one dword load, unless the frame is a single pixel (the dword would leave it)
    if (N >= 2 && !st->aug_bytes) SEG_LAUNCH(st, "k_augment", k_augment<true>, grid, block, j);
    else SEG_LAUNCH(st, "k_augment", k_augment<false>, grid, block, j);
    return (int)hipGetLastError();
}

}  // extern "C"
