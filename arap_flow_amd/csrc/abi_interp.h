// abi_interp.h -- frames from flows (ArapFlow_InterpFrames, arap_interp.h): the scratch size, the argument checks and the
// clear and two launches of a call.
#pragma once

static_assert(INTERP_MAX_TIMES == ARAPFLOW_INTERP_MAX_TIMES && INTERP_FILL == ARAPFLOW_INTERP_FILL, "arap_opt.h states both");

// W * H != 0, W * H < 2^31, 1 <= K <= 32 and K * W * H < 2^31
static bool interp_sizes_ok(unsigned W, unsigned H, unsigned K)
{
    const uint64_t N = (uint64_t)W * H;
    return N != 0 && N < (1ull << 31) && K != 0 && K <= (unsigned)INTERP_MAX_TIMES && K * N < (1ull << 31);
}

extern "C" {

// the K key images, 8 bytes a pixel and time, aligned to 256 bytes
uint64_t ArapFlow_InterpScratchBytes(unsigned W, unsigned H, unsigned K)
{
    return interp_sizes_ok(W, H, K) ? align_up((uint64_t)K * W * H * 8, 256) : 0;
}

int ArapFlow_InterpFrames(Opt_State* st, unsigned W, unsigned H, const void* A, const void* B, const void* fwd, const void* bwd,
                          unsigned K, const float* times, void* out, void* src, void* scratch)
{
    if (!st || !A || !B || !fwd || !times || !out || !scratch || !interp_sizes_ok(W, H, K)) return -1;
    for (unsigned k = 0; k < K; ++k)
        if (!std::isfinite(times[k]) || !(times[k] > 0.f) || !(times[k] < 1.f)) return -1;
    const uint64_t N = (uint64_t)W * H, all = K * N, keys = all * 8;
    const std::pair<const void*, uint64_t> bufs[] = {{out, all * 3}, {src, all}, {scratch, align_up(keys, 256)}, {A, N * 3}, {B, N * 3},
                                                     {fwd, N * 8}, {bwd, N * 8}};
    if (buffers_overlap(bufs, 3, 7)) return -1;
    InterpJob j{};
    j.A = (const uint8_t*)A; j.B = (const uint8_t*)B; j.fwd = (const float2*)fwd; j.bwd = (const float2*)bwd;
    j.key = (unsigned long long*)scratch; j.out = (uint8_t*)out; j.src = (uint8_t*)src;
    j.W = (int)W; j.H = (int)H; j.K = K;
    j.runs = (W + INTERP_RUN - 1u) / INTERP_RUN;
    for (unsigned k = 0; k < K; ++k) j.t[k] = times[k];
    // the clear, then the two launches, through abi_seg.h's per-kernel timing macro (ArapFlow_SetKernelTiming sees both);
    // runs * H <= W * H < 2^31 blocks
    HC(hipMemsetAsync(scratch, 0xff, keys, st->stream));
    SEG_LAUNCH(st, "k_interp_splat", k_interp_splat, dim3((unsigned)((N + 255u) / 256u), bwd ? 2u : 1u), dim3(256), j);
    SEG_LAUNCH(st, "k_interp_gather", k_interp_gather, dim3(j.runs * H, K), dim3(INTERP_RUN), j);
    return (int)hipGetLastError();
}

}  // extern "C"
