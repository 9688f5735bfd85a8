// abi_clip.h -- training clips (ArapFlow_ClipTables, ArapFlow_AugmentClips; arap_clip.h): a frame's tables from the
// per-frame pieces of abi_aug.h; the argument checks; the per-frame device table and the link table the state owns; the
// one or two launches of a call.
#pragma once

static_assert(CLIP_MAX_FRAMES == ARAPFLOW_CLIP_MAX_FRAMES && CLIP_MAX_LINKS == ARAPFLOW_CLIP_MAX_LINKS, "clip limits");
static_assert(sizeof(ArapFlow_ClipFrame) == 120, "ArapFlow_ClipFrame layout");
static_assert(CLIP_MAX_LINKS * sizeof(int2) <= sizeof(ClipFrameDev), "the link table fits the slot behind the frames' entries");

// P = T^-1 and the tone table of a frame; false for a frame outside its ranges, and for every frame with det(T) == 0
static bool clip_tables(const ArapFlow_ClipFrame& s, const float scale[3], const float bias[3], float P[6], float lut[3][256])
{
    if (!aug_frame_ok(s.T, s.gain, s.gamma) || !aug_frame_inverse(s.T, P)) return false;
    aug_frame_lut(s.gain, s.gamma, scale, bias, lut);
    return true;
}

extern "C" {

int ArapFlow_ClipTables(const ArapFlow_ClipFrame* frame, const float scale[3], const float bias[3], float P[6], float lut[3][256])
{
    if (!frame || !scale || !bias || !P || !lut) return -1;
    return clip_tables(*frame, scale, bias, P, lut) ? 0 : -1;
}

int ArapFlow_AugmentClips(Opt_State* st, unsigned W, unsigned H, unsigned w, unsigned h, unsigned B, unsigned T, unsigned L,
                          unsigned P, const void* frames, const int32_t* links, const void* flows, const void* skip,
                          const void* pos, const void* occ, const ArapFlow_ClipFrame* samples, const float scale[3],
                          const float bias[3], float tau, void* video, void* out_flows, void* valid, void* tracks, void* vis)
{
    const bool want_links = out_flows || valid, want_points = tracks || vis;
    if (!st || !samples || !scale || !bias || !(video || want_links || want_points)) return -1;
    if (W == 0 || H == 0 || w == 0 || h == 0 || B == 0 || T == 0 || !(tau >= 0.f)) return -1;
    if (B > (unsigned)AUG_MAX_BATCH || T > (unsigned)CLIP_MAX_FRAMES || B * T > (unsigned)CLIP_MAX_UNITS || L > (unsigned)CLIP_MAX_LINKS) return -1;
    const uint64_t N = (uint64_t)W * H, n = (uint64_t)w * h, BT = (uint64_t)B * T, BL = (uint64_t)B * L;
    if (N >= (1ull << 31) || n >= (1ull << 31) || BT * n >= (1ull << 31) || BL * n >= (1ull << 31) || BT * P >= (1ull << 31)) return -1;
    if ((want_links && (L == 0 || !links)) || (want_points && P == 0)) return -1;
    // an input no asked output needs is not read: it takes no part in the checks
    if (!video) frames = nullptr;
    if (!want_links) { links = nullptr; flows = skip = nullptr; }
    if (!want_points) pos = nullptr;
    if (!vis) occ = nullptr;
    if ((video && !frames) || (want_links && !flows) || (want_points && !pos) || (vis && !occ)) return -1;
    if (links)
        for (unsigned l = 0; l < L; ++l) {
            const int32_t i = links[2 * l], k = links[2 * l + 1];
            if (i < 0 || k < 0 || i >= (int32_t)T || k >= (int32_t)T || i == k) return -1;
        }
    const std::pair<const void*, uint64_t> bufs[] = {{video, BT * n * 12}, {out_flows, BL * n * 8}, {valid, BL * n}, {tracks, BT * P * 8},
                                                     {vis, BT * P}, {frames, BT * N * 3}, {flows, BL * N * 8}, {skip, BL * N},
                                                     {pos, BT * P * 8}, {occ, BT * P}};
    if (buffers_overlap(bufs, 5, 10)) return -1;
    // the frames' entries, and behind them in one more slot the link table: one copy brings both
    std::vector<ClipFrameDev> tab(BT + 1);
    for (unsigned i = 0; i < BT; ++i) {
        const ArapFlow_ClipFrame& s = samples[i];
        ClipFrameDev& t = tab[i];
        if (s.n_erase > (unsigned)AUG_MAX_ERASE || !clip_tables(s, scale, bias, t.P, t.lut)) return -1;
        std::memcpy(t.T, s.T, sizeof(t.T));
        std::memcpy(t.fill, s.fill, sizeof(t.fill));
        t.n_erase = (int)s.n_erase;
        std::memcpy(t.erase, s.erase, sizeof(t.erase));
    }
    const size_t link_bytes = links ? L * sizeof(int2) : 0;
    if (link_bytes) std::memcpy(&tab[BT], links, link_bytes);
    HC(hipSetDevice(st->device));
    if (st->clip_cap < BT) {                                // (hipFree waits for the calls that still read the old table)
        if (st->clip) (void)hipFree(st->clip);
        st->clip = nullptr; st->clip_cap = 0;
        if (hipMalloc(&st->clip, (BT + 1) * sizeof(ClipFrameDev)) != hipSuccess) return (int)hipErrorOutOfMemory;
        st->clip_cap = (unsigned)BT;
    }
    // pageable, as in ArapFlow_AugmentPairs: the runtime has copied `tab` away when this returns and writes the table in the
    // stream's order.  One table per state: a caller who moves the state to another stream orders the two streams
    HC(hipMemcpyAsync(st->clip, tab.data(), BT * sizeof(ClipFrameDev) + link_bytes, hipMemcpyHostToDevice, st->stream));
    const ClipFrameDev* dev = (const ClipFrameDev*)st->clip;
    if (video || want_links) {
        ClipJob j{};
        j.frames = (const uint8_t*)frames; j.flows = (const float2*)flows; j.skip = (const uint8_t*)skip;
        j.tab = dev; j.links = (const int2*)(dev + BT);
        j.video = (float*)video; j.out_flows = (float*)out_flows; j.valid = (uint8_t*)valid;
        j.W = (int)W; j.H = (int)H; j.w = (int)w; j.h = (int)h; j.T = (int)T; j.L = (int)L;
        j.tiles_x = (int)((w + AUG_TILE_W - 1) / AUG_TILE_W);
        j.unit0 = video ? 0 : (int)T;
        j.tau = tau;
        j.vec = w % AUG_PX == 0 && (((uintptr_t)video | (uintptr_t)out_flows) & 15) == 0 && ((uintptr_t)valid & 3) == 0;
        const unsigned units = (video ? T : 0u) + (want_links ? L : 0u);
        const dim3 grid((unsigned)j.tiles_x * ((h + AUG_TILE_H - 1) / AUG_TILE_H), units, B), block(256);
        // a tap's three bytes in one dword load, unless the frame is a single pixel (the dword would leave it)
        if (N >= 2 && !st->aug_bytes) SEG_LAUNCH(st, "k_augment_clip", k_augment_clip<true>, grid, block, j);
        else SEG_LAUNCH(st, "k_augment_clip", k_augment_clip<false>, grid, block, j);
    }
    if (want_points) {
        ClipTrackJob j{};
        j.pos = (const float*)pos; j.occ = (const uint8_t*)occ; j.tab = dev;
        j.tracks = (float*)tracks; j.vis = (uint8_t*)vis;
        j.T = (int)T; j.P = (int)P; j.w = (int)w; j.h = (int)h;
        j.vec = (((uintptr_t)pos | (uintptr_t)tracks) & 7) == 0;
        SEG_LAUNCH(st, "k_clip_tracks", k_clip_tracks, dim3((P + 255u) / 256u, T, B), dim3(256), j);
    }
    return (int)hipGetLastError();
}

}  // extern "C"
