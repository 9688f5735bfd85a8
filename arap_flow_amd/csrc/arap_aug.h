// arap_aug.h -- training batches: B pairs under their own affine maps, tone curves and eraser rectangles, cropped,
// normalised and laid out planar in one launch (gfx950).
//
// Definitions: DESIGN.md "Training batches" and include/arap_opt.h; the numpy twin is tests/aug_ref.py.  The library is
// built with -ffp-contract=off: every operator below is one IEEE f32 operation in the order the parentheses give, and no
// fmaf is written.  No atomics, no scratch, no reduction: an output is a function of its pixel's inputs alone.
//
// Launch shape: 256 threads, a block is a 64 x 16 tile of one sample's crop (grid.x runs over the tiles of a crop,
// grid.z over the samples).  A lane produces AUG_PX = 4 consecutive pixels of a row, a wave is 16 lanes x 4 rows = 64 x 4
// pixels: under a rotation of a few tenths of a radian its taps touch about 4 + 64 sin(angle) source rows, and the 16
// lanes of a row write 256 contiguous bytes of every float plane with 16-byte stores (`vec`: w % 4 == 0 and the plane
// bases aligned; otherwise the same pixels go out one by one behind their own bound checks).
//
// The block stages the sample's tone tables in LDS once (2 x 3 x 256 floats, 6 KB; only those of the images asked), so
// the 24 table reads a pixel makes are LDS reads.  The gather of the taps is the only irregular access: a tap's three
// bytes are one dword load at the pixel's byte address, straight from memory through L2 (measured against byte loads,
// which the instantiation DWORD = false keeps for a frame of one pixel: profiles/augment/README.md).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace arap {

constexpr int AUG_MAX_BATCH = 64, AUG_MAX_ERASE = 4;           // ARAPFLOW_AUG_MAX_BATCH, ARAPFLOW_AUG_MAX_ERASE
constexpr int AUG_TILE_W = 64, AUG_TILE_H = 16, AUG_PX = 4;

// a sample as the kernel reads it: what ArapFlow_AugmentTables derives next to what the caller gave.  160 bytes in front
// of the tables, so those start 16-byte aligned
struct AugSampleDev {
    float T1[6], T2[6], P2[6];
    float fill[3];
    int n_erase;
    int erase[AUG_MAX_ERASE][4];
    int pad[2];
    float lut[2][3][256];
};
static_assert(sizeof(AugSampleDev) == 160 + 6144, "AugSampleDev layout");

struct AugJob {
    const uint8_t* rgb1;            // [B][H][W][3], NULL unless img1
    const uint8_t* rgb2;            // [B][H][W][3], NULL unless img2
    const float2* flow;             // [B][H][W], NULL unless out_flow or valid
    const uint8_t* skip;            // [B][H][W] or NULL
    const AugSampleDev* tab;        // [B]
    float* img1;                    // [B][3][h][w] or NULL
    float* img2;
    float* out_flow;                // [B][2][h][w] or NULL
    uint8_t* valid;                 // [B][h][w] or NULL
    int W, H, w, h, tiles_x;
    float tau;
    int vec;                        // w % 4 == 0, the float planes 16-byte and `valid` 4-byte aligned
};

struct AugTaps { int x0, x1, y0, y1; float fx, fy; bool inside; };

__device__ __forceinline__ float2 aug_apply(const float* T, float x, float y)
{
    return make_float2((T[0] * x + T[1] * y) + T[2], (T[3] * x + T[4] * y) + T[5]);
}

// (the integer clamps after the float ones only matter for a plane wider than 2^24, where (float)(W - 1) may round up)
__device__ __forceinline__ AugTaps aug_taps(float2 q, int W, int H)
{
    AugTaps t;
    const float mx = (float)(W - 1), my = (float)(H - 1);
    t.inside = q.x >= 0.0f && q.x <= mx && q.y >= 0.0f && q.y <= my;          // false on NaN
    const float bx = fminf(fmaxf(q.x, 0.0f), mx), by = fminf(fmaxf(q.y, 0.0f), my);
    t.x0 = min((int)floorf(bx), W - 1); t.y0 = min((int)floorf(by), H - 1);
    t.x1 = min(t.x0 + 1, W - 1); t.y1 = min(t.y0 + 1, H - 1);
    t.fx = bx - (float)t.x0; t.fy = by - (float)t.y0;
    return t;
}

__device__ __forceinline__ float aug_mix(float c00, float c01, float c10, float c11, float fx, float fy)
{
    const float top = c00 + fx * (c01 - c00), bot = c10 + fx * (c11 - c10);
    return top + fy * (bot - top);
}

// the three bytes of pixel i of a frame of N >= 2 pixels in one dword load at any byte alignment (bits 0..23).  The dword
// of the frame's last pixel would end one byte behind the frame: it starts one byte early instead
__device__ __forceinline__ uint32_t aug_pixel_dword(const uint8_t* __restrict__ frame, size_t i, size_t N)
{
    const bool last = i == N - 1;
    uint32_t v;
    __builtin_memcpy(&v, frame + 3 * i - (last ? 1 : 0), 4);
    return last ? v >> 8 : v;
}

// the three channels of one image at one output pixel.  frame: the sample's [H][W][3]; lut: the frame's [3][256] in LDS
template <bool DWORD>
__device__ __forceinline__ void aug_image(const uint8_t* __restrict__ frame, const float* lut, float2 q, int W, int H, float out[3])
{
    const AugTaps t = aug_taps(q, W, H);
    if (DWORD) {
        const size_t N = (size_t)W * H, r0 = (size_t)t.y0 * W, r1 = (size_t)t.y1 * W;
        const uint32_t v00 = aug_pixel_dword(frame, r0 + t.x0, N), v01 = aug_pixel_dword(frame, r0 + t.x1, N);
        const uint32_t v10 = aug_pixel_dword(frame, r1 + t.x0, N), v11 = aug_pixel_dword(frame, r1 + t.x1, N);
#pragma unroll
        for (int c = 0; c < 3; ++c)
            out[c] = aug_mix(lut[256 * c + (v00 >> 8 * c & 255)], lut[256 * c + (v01 >> 8 * c & 255)], lut[256 * c + (v10 >> 8 * c & 255)],
                             lut[256 * c + (v11 >> 8 * c & 255)], t.fx, t.fy);
        return;
    }
    const uint8_t* r0 = frame + (size_t)t.y0 * W * 3;
    const uint8_t* r1 = frame + (size_t)t.y1 * W * 3;
    const uint8_t *p00 = r0 + (size_t)t.x0 * 3, *p01 = r0 + (size_t)t.x1 * 3;
    const uint8_t *p10 = r1 + (size_t)t.x0 * 3, *p11 = r1 + (size_t)t.x1 * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        out[c] = aug_mix(lut[256 * c + p00[c]], lut[256 * c + p01[c]], lut[256 * c + p10[c]], lut[256 * c + p11[c]], t.fx, t.fy);
}

// one tap of the flow: its value with (0, 0) for a bad one, and whether it is bad
__device__ __forceinline__ float2 aug_flow_tap(const float2* __restrict__ flow, const uint8_t* __restrict__ skip, size_t i, bool& bad)
{
    const float2 f = flow[i];
    const bool b = (skip && skip[i] != 0) || !(fabsf(f.x) <= 3.4028235e38f) || !(fabsf(f.y) <= 3.4028235e38f);
    bad = bad || b;
    return b ? make_float2(0.0f, 0.0f) : f;
}

// the flow and the validity of one output pixel (x, y).  flow, skip: the sample's planes.  Returns valid
__device__ __forceinline__ bool aug_flow(const float2* __restrict__ flow, const uint8_t* __restrict__ skip, const float* P2,
                                         float2 q, float x, float y, int W, int H, float tau, float2& out)
{
    const AugTaps t = aug_taps(q, W, H);
    const bool ux = t.fx > 0.0f, uy = t.fy > 0.0f, uxy = ux && uy;
    const size_t i00 = (size_t)t.y0 * W + t.x0;
    const size_t i01 = ux ? (size_t)t.y0 * W + t.x1 : i00, i10 = uy ? (size_t)t.y1 * W + t.x0 : i00;
    const size_t i11 = uxy ? (size_t)t.y1 * W + t.x1 : i00;
    bool bad = false;
    const float2 f00 = aug_flow_tap(flow, skip, i00, bad), f01 = aug_flow_tap(flow, skip, i01, bad);
    const float2 f10 = aug_flow_tap(flow, skip, i10, bad), f11 = aug_flow_tap(flow, skip, i11, bad);
    const float2 u = make_float2(aug_mix(f00.x, f01.x, f10.x, f11.x, t.fx, t.fy), aug_mix(f00.y, f01.y, f10.y, f11.y, t.fx, t.fy));
    float spread = fmaxf(fabsf(f01.x - f00.x), fabsf(f01.y - f00.y));
    spread = fmaxf(spread, fmaxf(fabsf(f10.x - f00.x), fabsf(f10.y - f00.y)));
    spread = fmaxf(spread, fmaxf(fabsf(f11.x - f00.x), fabsf(f11.y - f00.y)));
    out.x = (((P2[0] * q.x + P2[1] * q.y) + P2[2]) - x) + (P2[0] * u.x + P2[1] * u.y);
    out.y = (((P2[3] * q.x + P2[4] * q.y) + P2[5]) - y) + (P2[3] * u.x + P2[4] * u.y);
    const bool finite = fabsf(out.x) <= 3.4028235e38f && fabsf(out.y) <= 3.4028235e38f;
    const bool ok = t.inside && !bad && spread <= tau && finite;
    if (!ok) out = make_float2(0.0f, 0.0f);
    return ok;
}

// AUG_PX values of one row of a float plane: one 16-byte store, or one by one behind the crop's right edge
__device__ __forceinline__ void aug_store(float* __restrict__ row, int x, int w, bool vec, const float v[AUG_PX])
{
    if (vec) {
        *reinterpret_cast<float4*>(row + x) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < AUG_PX; ++k)
            if (x + k < w) row[x + k] = v[k];
    }
}

// grid = (tiles_x * ceil(h/16), 1, B), block = 256.  DWORD: a tap's three bytes in one dword load (W * H >= 2)
template <bool DWORD>
__global__ __launch_bounds__(256) void k_augment(AugJob j)
{
    __shared__ __align__(16) float lut[2 * 3 * 256];
    const int b = blockIdx.z, tid = threadIdx.x;
    const AugSampleDev& s = j.tab[b];
    {
        const float4* src = reinterpret_cast<const float4*>(&s.lut[0][0][0]);
        float4* dst = reinterpret_cast<float4*>(lut);
        const int lo = j.img1 ? 0 : 192, hi = j.img2 ? 384 : 192;                  // float4s: 192 a frame
        for (int i = lo + tid; i < hi; i += 256) dst[i] = src[i];
    }
    __syncthreads();                                                                // every thread of the block: the only return lies behind it
    const int tx = (int)(blockIdx.x % (unsigned)j.tiles_x), ty = (int)(blockIdx.x / (unsigned)j.tiles_x);
    const int lane = tid & 63, wave = tid >> 6;
    const int x = tx * AUG_TILE_W + (lane & 15) * AUG_PX, y = ty * AUG_TILE_H + wave * 4 + (lane >> 4);
    if (x >= j.w || y >= j.h) return;
    const int W = j.W, H = j.H, w = j.w, h = j.h;
    const bool vec = j.vec != 0;
    const size_t N = (size_t)W * H, n = (size_t)w * h, src0 = (size_t)b * N, row = (size_t)y * w;
    const float fy = (float)y;
    const int count = min(AUG_PX, w - x);

    if (j.img1) {
        float v[3][AUG_PX] = {};
#pragma unroll
        for (int k = 0; k < AUG_PX; ++k) {
            if (k >= count) break;
            float o[3];
            aug_image<DWORD>(j.rgb1 + src0 * 3, lut, aug_apply(s.T1, (float)(x + k), fy), W, H, o);
            v[0][k] = o[0]; v[1][k] = o[1]; v[2][k] = o[2];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) aug_store(j.img1 + ((size_t)b * 3 + c) * n + row, x, w, vec, v[c]);
    }
    if (j.img2) {
        float v[3][AUG_PX] = {};
#pragma unroll
        for (int k = 0; k < AUG_PX; ++k) {
            if (k >= count) break;
            float o[3];
            aug_image<DWORD>(j.rgb2 + src0 * 3, lut + 768, aug_apply(s.T2, (float)(x + k), fy), W, H, o);
            bool erased = false;
            for (int e = 0; e < s.n_erase; ++e)
                erased = erased || (x + k >= s.erase[e][0] && x + k < s.erase[e][2] && y >= s.erase[e][1] && y < s.erase[e][3]);
            v[0][k] = erased ? s.fill[0] : o[0]; v[1][k] = erased ? s.fill[1] : o[1]; v[2][k] = erased ? s.fill[2] : o[2];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) aug_store(j.img2 + ((size_t)b * 3 + c) * n + row, x, w, vec, v[c]);
    }
    if (j.out_flow || j.valid) {
        float v[2][AUG_PX] = {};
        uint8_t ok[AUG_PX] = {};
#pragma unroll
        for (int k = 0; k < AUG_PX; ++k) {
            if (k >= count) break;
            float2 o;
            const float fxk = (float)(x + k);
            ok[k] = aug_flow(j.flow + src0, j.skip ? j.skip + src0 : nullptr, s.P2, aug_apply(s.T1, fxk, fy), fxk, fy, W, H,
                             j.tau, o) ? 255 : 0;
            v[0][k] = o.x; v[1][k] = o.y;
        }
        if (j.out_flow) {
            aug_store(j.out_flow + ((size_t)b * 2 + 0) * n + row, x, w, vec, v[0]);
            aug_store(j.out_flow + ((size_t)b * 2 + 1) * n + row, x, w, vec, v[1]);
        }
        if (j.valid) {
            uint8_t* vr = j.valid + (size_t)b * n + row;
            if (vec) {
                *reinterpret_cast<uint32_t*>(vr + x) = (uint32_t)ok[0] | (uint32_t)ok[1] << 8 | (uint32_t)ok[2] << 16 | (uint32_t)ok[3] << 24;
            } else {
#pragma unroll
                for (int k = 0; k < AUG_PX; ++k)
                    if (x + k < w) vr[x + k] = ok[k];
            }
        }
    }
}

}  // namespace arap
