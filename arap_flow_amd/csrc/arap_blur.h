// arap_blur.h -- motion-blurred frames: the integer mean of S layered warps of one mesh at S moments of an exposure
// window (gfx950).
//
// Definitions: DESIGN.md "Motion blur".  Every layer l has two states, given as flows a_l and b_l (a == NULL: all zero).
// Sample k of the window has a time t_k (ArapFlow_BlurSchedule, host) and is the layered warp of the flow field
//     f = u * a + t * b,   u = 1.0f - t          (float32, one IEEE operation per operator)
// -- positions flow_pos(x, y, f), keys, winner rule and colour expression of arap_warp.h / arap_layers.h, unchanged: the
// quad body is warp_quad with the position policy BlurPos below, and no float expression of the rasteriser is stated
// here.  The frame is the integer sum of the samples' colours, with the background picture's sample (bg_sample /
// bg_apply of arap_bg.h, the sample's own map) where a sample leaves the pixel uncovered, divided by S with round half up;
// the alpha is the count of covering samples scaled to 255 the same way.
//
// Samples are processed in chunks of at most BLUR_CHUNK, one key image per sample of the chunk:
//     k_blur_raster   grid (ceil(W/64), ceil(H/4), n * g): layer l of sample s of the chunk into key image s
//     k_blur_accum    per pixel: reads the g keys and re-zeroes them, adds colour and coverage in registers, adds the
//                     background of uncovered samples, and either writes the final bytes (the last chunk) or carries the
//                     sums to the next chunk in a uint16 x 4 image (32 * 255 fits).
// The last chunk is sized to what is left.  The chunk's times and maps travel by value in the kernel arguments, read with
// scalar loads (blockIdx.z and the sample loop are uniform).  No image per sample, no RGB resolve per sample, no float
// addition across samples, no LDS; the only atomics are the key's 64-bit atomicMax.  Every output is a function of the
// inputs alone.
//
// Scratch per pixel: 8 * min(S, BLUR_CHUNK) (keys) and, when S > BLUR_CHUNK, 8 (the carried sums).
// Limits: those of arap_layers.h (n <= 255, N < 2^31), S <= BLUR_MAX_SAMPLES.
#pragma once
#include "arap_bg.h"
#include "arap_layers.h"

namespace arap {

constexpr int BLUR_CHUNK = 8;               // ARAPFLOW_BLUR_CHUNK
constexpr int BLUR_MAX_SAMPLES = 32;        // ARAPFLOW_MAX_BLUR_SAMPLES

struct BlurFrame {                          // what every chunk of a call shares
    const uint8_t* rgb;                     // [N][3]
    const uint8_t* masks;                   // [n][N]  0 = object
    const float2* flows_a;                  // [n][N] or NULL: all zero
    const float2* flows_b;                  // [n][N]
    unsigned long long* keys;               // [min(S, BLUR_CHUNK)][N] scratch, all zero between kernels of different chunks
    ushort4* carry;                         // [N] scratch: (r, g, b, cnt) summed over the chunks before, or NULL when S <= BLUR_CHUNK
    uint8_t* out_rgb;                       // [N][3] or NULL
    uint8_t* out_alpha;                     // [N] or NULL
    BgPicture bg;                           // rgb == NULL: no background, an uncovered sample adds 0
    int n, samples;
};

struct BlurChunk {                          // the samples of one chunk
    float t[BLUR_CHUNK];
    BgMap M[BLUR_CHUNK];                    // read only with a background
    int g;                                  // samples in this chunk, 1 .. BLUR_CHUNK
    int first, last;                        // no sums carried in / the final bytes are written
    int same_map;                           // every map of the CALL is M[0] (a still camera): one picture sample serves all
};

// the position policy of sample time t: vertex (x, y) of the layer whose flows are a (or NULL) and b
struct BlurPos {
    const float2* a;
    const float2* b;
    float u, t;
    __device__ __forceinline__ float2 operator()(const WarpJob&, int x, int y, int i) const
    {
        const float2 fa = a ? a[i] : make_float2(0.f, 0.f), fb = b[i];
        return flow_pos(x, y, make_float2(u * fa.x + t * fb.x, u * fa.y + t * fb.y));
    }
};

// layer blockIdx.z % n of sample blockIdx.z / n of the chunk into that sample's key image
// grid = (ceil(W/64), ceil(H/4), n * g), block = (64,4)
__global__ __launch_bounds__(256) void k_blur_raster(BlurFrame f, BlurChunk c, int W, int H)
{
    const int s = (int)blockIdx.z / f.n, l = (int)blockIdx.z - s * f.n;
    const size_t N = (size_t)W * H;
    WarpJob v{};
    v.rgb = f.rgb;
    v.mask = f.masks + (size_t)l * N;
    v.key = f.keys + (size_t)s * N;
    const float t = c.t[s];
    const BlurPos pos{f.flows_a ? f.flows_a + (size_t)l * N : nullptr, f.flows_b + (size_t)l * N, 1.0f - t, t};
    raster_quad(v, W, H, blockIdx.x * 64 + threadIdx.x, blockIdx.y * 4 + threadIdx.y, (unsigned)l, pos);
}

// round half up of a / S for the numerator twice a (DESIGN.md "Motion blur": (2 a + S) / (2 S))
__device__ __forceinline__ uint8_t blur_mean(unsigned a, unsigned S) { return (uint8_t)((2u * a + S) / (2u * S)); }

// grid = (ceil(W/64), ceil(H/4)), block = (64,4)
__global__ __launch_bounds__(256) void k_blur_accum(BlurFrame f, BlurChunk c, int W, int H)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t N = (size_t)W * H, i = (size_t)y * W + x;
    unsigned r = 0, g = 0, b = 0, cnt = 0;
    if (!c.first) {
        const ushort4 q = f.carry[i];
        r = q.x; g = q.y; b = q.z; cnt = q.w;
    }
    unsigned open = 0;                       // bit s: sample s of the chunk leaves the pixel uncovered
    for (int s = 0; s < c.g; ++s) {
        unsigned long long* const kp = f.keys + (size_t)s * N + i;
        const unsigned long long k = *kp;
        if (k == 0ull) { open |= 1u << s; continue; }
        *kp = 0ull;
        r += (unsigned)(k >> 16) & 0xffu; g += (unsigned)(k >> 8) & 0xffu; b += (unsigned)k & 0xffu;
        ++cnt;
    }
    if (f.bg.rgb && open) {
        if (c.same_map) {
            uint8_t v[3];
            bg_sample(f.bg, bg_apply(c.M[0], x, y), v);
            const unsigned m = (unsigned)__popc(open);
            r += m * v[0]; g += m * v[1]; b += m * v[2];
        } else {
            for (int s = 0; s < c.g; ++s) {
                if (!(open >> s & 1u)) continue;
                uint8_t v[3];
                bg_sample(f.bg, bg_apply(c.M[s], x, y), v);
                r += v[0]; g += v[1]; b += v[2];
            }
        }
    }
    if (!c.last) {
        f.carry[i] = make_ushort4((unsigned short)r, (unsigned short)g, (unsigned short)b, (unsigned short)cnt);
        return;
    }
    const unsigned S = (unsigned)f.samples;
    if (f.out_rgb) {
        f.out_rgb[3 * i + 0] = blur_mean(r, S);
        f.out_rgb[3 * i + 1] = blur_mean(g, S);
        f.out_rgb[3 * i + 2] = blur_mean(b, S);
    }
    if (f.out_alpha) f.out_alpha[i] = blur_mean(255u * cnt, S);
}

}  // namespace arap
