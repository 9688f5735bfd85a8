// arap_bg.h -- moving background: full-frame RGB, flow and occlusion behind the warp's objects (gfx950).
//
// Definitions: DESIGN.md "Moving background".  A post-pass of the warp family on caller-owned images: one kernel per
// frame domain of a pair, and one for a whole sequence of frames (k_bg_seq); one pass per pixel, no atomics, no scratch.  Every output is optional (a null pointer: not computed,
// its inputs not read) and a function of the inputs alone.  On an object pixel of its domain an output is a copy of the
// object-side input; on a background pixel it comes from the affine maps: the sampling map M of the domain (pixel ->
// point of the background picture) and the point map G to the other frame.
//
// Launch shape of the family: dim3(64, 4) blocks over (ceil(W/64), ceil(H/4)), so a wave is 64 neighbours of one row:
// the streams are coalesced and the four taps of a small rotation touch few rows of the picture per wave.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace arap {

// (x, y) -> (a x + b y + c, d x + e y + f)
struct BgMap { float a, b, c, d, e, f; };

struct BgPicture { const uint8_t* rgb; int w, h; };     // [h][w][3]

// one frame domain.  Frame 1: own = mask_red (object: == 0), other = cover2 (hides: != 0), G = frame 1 -> frame 2.
// Frame 2: own = cover2 (object: != 0), other = mask_red (hid: == 0), G = frame 2 -> frame 1.
struct BgSide {
    const uint8_t* own;             // [N]
    const uint8_t* other;           // [N]
    const uint8_t* rgb;             // [N][3], read on object pixels for out_rgb
    const float2* flow;             // [N], read on object pixels for out_flow
    const uint8_t* occ;             // [N], read on object pixels for out_occ
    uint8_t* out_rgb;               // [N][3] or NULL
    float2* out_flow;               // [N] or NULL
    uint8_t* out_occ;               // [N] or NULL
    BgMap M, G;
};

__device__ __forceinline__ float2 bg_apply(const BgMap& m, int x, int y)
{
    const float fx = (float)x, fy = (float)y;
    return make_float2(fmaf(m.a, fx, fmaf(m.b, fy, m.c)), fmaf(m.d, fx, fmaf(m.e, fy, m.f)));
}

// S(bg, b): bilinear, clamp to edge, round half up.  (The integer clamps after the float ones only matter for a
// picture wider than 2^24, where (float)(w - 1) may round up.)
__device__ __forceinline__ void bg_sample(const BgPicture& bg, float2 b, uint8_t out[3])
{
    const float bx = fminf(fmaxf(b.x, 0.0f), (float)(bg.w - 1));
    const float by = fminf(fmaxf(b.y, 0.0f), (float)(bg.h - 1));
    const int x0 = min((int)floorf(bx), bg.w - 1), y0 = min((int)floorf(by), bg.h - 1);
    const int x1 = min(x0 + 1, bg.w - 1), y1 = min(y0 + 1, bg.h - 1);
    const float fx = bx - (float)x0, fy = by - (float)y0;
    const uint8_t* r0 = bg.rgb + (size_t)y0 * bg.w * 3;
    const uint8_t* r1 = bg.rgb + (size_t)y1 * bg.w * 3;
    const uint8_t *p00 = r0 + (size_t)x0 * 3, *p01 = r0 + (size_t)x1 * 3;
    const uint8_t *p10 = r1 + (size_t)x0 * 3, *p11 = r1 + (size_t)x1 * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float c00 = (float)p00[c], c01 = (float)p01[c], c10 = (float)p10[c], c11 = (float)p11[c];
        const float top = fmaf(fx, c01 - c00, c00), bot = fmaf(fx, c11 - c10, c10);
        const float v = fmaf(fy, bot - top, top);
        out[c] = (uint8_t)(v + 0.5f);
    }
}

// one pixel of one domain.  The two template flags only select the mask conventions: OWN_COVER, the domain's own mask
// is a cover (object: != 0) and not a solver mask (object: == 0); OTHER_COVER, the same for the mask of the frame the
// point map leads to (a cover hides where it is != 0, a solver mask where it is == 0).
template <bool OWN_COVER, bool OTHER_COVER>
__device__ __forceinline__ void bg_pixel(const BgSide& s, const BgPicture& bg, int W, int H)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t i = (size_t)y * W + x;
    const uint8_t m = s.own[i];
    const bool object = OWN_COVER ? m != 0 : m == 0;
    if (s.out_rgb) {
        uint8_t v[3];
        if (object) { v[0] = s.rgb[3 * i]; v[1] = s.rgb[3 * i + 1]; v[2] = s.rgb[3 * i + 2]; }
        else bg_sample(bg, bg_apply(s.M, x, y), v);
        s.out_rgb[3 * i] = v[0]; s.out_rgb[3 * i + 1] = v[1]; s.out_rgb[3 * i + 2] = v[2];
    }
    if (!s.out_flow && !s.out_occ) return;
    if (object) {
        if (s.out_flow) s.out_flow[i] = s.flow[i];
        if (s.out_occ) s.out_occ[i] = s.occ[i];
        return;
    }
    const float2 p = bg_apply(s.G, x, y);
    if (s.out_flow) s.out_flow[i] = make_float2(p.x - (float)x, p.y - (float)y);
    if (!s.out_occ) return;
    bool hidden = !(p.x >= 0.f && p.x <= (float)(W - 1) && p.y >= 0.f && p.y <= (float)(H - 1));      // true on NaN
    if (!hidden) {
        const int nx = min((int)floorf(p.x + 0.5f), W - 1), ny = min((int)floorf(p.y + 0.5f), H - 1);
        const uint8_t o = s.other[(size_t)ny * W + nx];
        hidden = OTHER_COVER ? o != 0 : o == 0;
    }
    s.out_occ[i] = hidden ? 255 : 0;
}

// frame-1 domain: out_rgb1, flow_full, occ_full.  grid = (ceil(W/64), ceil(H/4)), block = (64,4)
__global__ __launch_bounds__(256) void k_bg_frame1(BgSide s, BgPicture bg, int W, int H) { bg_pixel<false, true>(s, bg, W, H); }

// frame-2 domain: out_rgb2, bwd_full, occ_bwd_full.  Same launch shape.
__global__ __launch_bounds__(256) void k_bg_frame2(BgSide s, BgPicture bg, int W, int H) { bg_pixel<true, false>(s, bg, W, H); }

// A sequence frame 1 -> t_1 -> .. -> t_n -> frame 2 (DESIGN.md "Moving background over in-between frames"): frame f is a
// BgSide whose `other` is the cover of frame f + 1 and whose G leads there.  Frame 0 reads its own mask as the solver's,
// every later frame as a cover; the last frame has no link (out_flow == out_occ == NULL: only out_rgb).  The table
// travels by value in the kernel arguments (112 bytes a frame), read with scalar loads: blockIdx.z is uniform.
constexpr int BG_SEQ_MAX = 10;             // ARAPFLOW_MAX_SNAPSHOTS + 2

struct BgSeq { BgSide f[BG_SEQ_MAX]; };

// every frame of a sequence in one launch.  grid = (ceil(W/64), ceil(H/4), frames), block = (64,4)
__global__ __launch_bounds__(256) void k_bg_seq(BgSeq seq, BgPicture bg, int W, int H)
{
    const BgSide& s = seq.f[blockIdx.z];
    if (!s.out_rgb && !s.out_flow && !s.out_occ) return;
    if (blockIdx.z == 0) bg_pixel<false, true>(s, bg, W, H);
    else bg_pixel<true, true>(s, bg, W, H);
}

}  // namespace arap
