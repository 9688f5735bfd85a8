// arap_clip.h -- training clips: B clips of T frames, L flow links and P point tracks, every frame under its own affine
// map, tone curve and eraser rectangles, cropped, normalised and laid out planar in at most two launches (gfx950).
//
// Definitions: DESIGN.md "Training clips" and include/arap_opt.h; the numpy twin is tests/clip_ref.py.  The arithmetic is
// that of "Training batches": aug_apply, aug_taps, aug_image, aug_flow and aug_store of arap_aug.h are called, not copied.
// The library is built with -ffp-contract=off and no fmaf is written.  No atomics, no scratch, no reduction: an output is
// a function of its pixel's (its point's) inputs alone.
//
// k_augment_clip: 256 threads, a block is a 64 x 16 tile of one *unit* of one clip: grid = (tiles, units, B).  The units
// 0 .. T-1 are the frames, T .. T+L-1 the links; a launch that has no video starts at unit T, one without link outputs
// ends at T (`unit0`).  The unit is uniform per block (blockIdx.y), so the frame's table entry and the link's (i, j) come
// through scalar loads.  A frame block stages its 3 KB tone table in LDS; a link block stages nothing and has no barrier.
// A lane makes AUG_PX = 4 consecutive pixels of a row and stores them under the pair kernel's `vec` rule.
//
// k_clip_tracks: grid = (ceil(P / 256), T, B), a lane a point: its position through the inverse map of its own frame, its
// visibility from the source's flag, the crop and the frame's rectangles.
#pragma once
#include "arap_aug.h"

namespace arap {

constexpr int CLIP_MAX_FRAMES = 16, CLIP_MAX_LINKS = 32, CLIP_MAX_UNITS = 256;     // ARAPFLOW_CLIP_MAX_*; B * T <= 256

// a frame of a clip as the kernels read it: what ArapFlow_ClipTables derives next to what the caller gave.  128 bytes in
// front of the table, so that starts 16-byte aligned (no padding is needed for it)
struct ClipFrameDev {
    float T[6], P[6];
    float fill[3];
    int n_erase;
    int erase[AUG_MAX_ERASE][4];
    float lut[3][256];
};
static_assert(sizeof(ClipFrameDev) == 128 + 3072 && offsetof(ClipFrameDev, lut) % 16 == 0, "ClipFrameDev layout");

struct ClipJob {
    const uint8_t* frames;          // [B][T][H][W][3], NULL unless video
    const float2* flows;            // [B][L][H][W], NULL unless out_flows or valid
    const uint8_t* skip;            // [B][L][H][W] or NULL
    const ClipFrameDev* tab;        // [B][T]
    const int2* links;              // [L], behind the frames' entries in the same allocation
    float* video;                   // [B][T][3][h][w] or NULL
    float* out_flows;               // [B][L][2][h][w] or NULL
    uint8_t* valid;                 // [B][L][h][w] or NULL
    int W, H, w, h, tiles_x, T, L;
    int unit0;                      // the unit of blockIdx.y == 0: 0, or T for a launch without video
    float tau;
    int vec;                        // w % 4 == 0, the float planes 16-byte and `valid` 4-byte aligned
};

struct ClipTrackJob {
    const float* pos;               // [B][T][P][2]
    const uint8_t* occ;             // [B][T][P], NULL unless vis
    const ClipFrameDev* tab;        // [B][T]
    float* tracks;                  // [B][T][P][2] or NULL
    uint8_t* vis;                   // [B][T][P] or NULL
    int T, P, w, h;
    int vec;                        // pos and tracks 8-byte aligned
};

// grid = (tiles_x * ceil(h/16), units, B), block = 256.  DWORD: a tap's three bytes in one dword load (W * H >= 2)
template <bool DWORD>
__global__ __launch_bounds__(256) void k_augment_clip(ClipJob j)
{
    __shared__ __align__(16) float lut[3 * 256];
    const int b = blockIdx.z, unit = j.unit0 + (int)blockIdx.y, tid = threadIdx.x;
    const int tx = (int)(blockIdx.x % (unsigned)j.tiles_x), ty = (int)(blockIdx.x / (unsigned)j.tiles_x);
    const int lane = tid & 63, wave = tid >> 6;
    const int x = tx * AUG_TILE_W + (lane & 15) * AUG_PX, y = ty * AUG_TILE_H + wave * 4 + (lane >> 4);
    const int W = j.W, H = j.H, w = j.w, h = j.h;
    const bool vec = j.vec != 0;
    const size_t N = (size_t)W * H, n = (size_t)w * h, row = (size_t)y * w;
    const float fy = (float)y;
    const int count = min(AUG_PX, w - x);

    if (unit < j.T) {                                                               // a frame (uniform per block)
        const size_t f = (size_t)b * j.T + unit;
        const ClipFrameDev& s = j.tab[f];
        if (tid < 192) reinterpret_cast<float4*>(lut)[tid] = reinterpret_cast<const float4*>(&s.lut[0][0])[tid];
        __syncthreads();                                                            // every thread of a frame block: the return lies behind it
        if (x >= w || y >= h) return;
        float v[3][AUG_PX] = {};
#pragma unroll
        for (int k = 0; k < AUG_PX; ++k) {
            if (k >= count) break;
            float o[3];
            aug_image<DWORD>(j.frames + f * N * 3, lut, aug_apply(s.T, (float)(x + k), fy), W, H, o);
            bool erased = false;
            for (int e = 0; e < s.n_erase; ++e)
                erased = erased || (x + k >= s.erase[e][0] && x + k < s.erase[e][2] && y >= s.erase[e][1] && y < s.erase[e][3]);
            v[0][k] = erased ? s.fill[0] : o[0]; v[1][k] = erased ? s.fill[1] : o[1]; v[2][k] = erased ? s.fill[2] : o[2];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) aug_store(j.video + (f * 3 + c) * n + row, x, w, vec, v[c]);
        return;
    }
    // a link (i, j): the pair definition with T1 = T_i, P2 = P_j and the planes [b][l]
    if (x >= w || y >= h) return;
    const int l = unit - j.T;
    const int2 ij = j.links[l];
    const ClipFrameDev& si = j.tab[(size_t)b * j.T + ij.x];
    const ClipFrameDev& sj = j.tab[(size_t)b * j.T + ij.y];
    const size_t p = (size_t)b * j.L + l;
    float v[2][AUG_PX] = {};
    uint8_t ok[AUG_PX] = {};
#pragma unroll
    for (int k = 0; k < AUG_PX; ++k) {
        if (k >= count) break;
        float2 o;
        const float fxk = (float)(x + k);
        ok[k] = aug_flow(j.flows + p * N, j.skip ? j.skip + p * N : nullptr, sj.P, aug_apply(si.T, fxk, fy), fxk, fy, W, H, j.tau, o) ? 255 : 0;
        v[0][k] = o.x; v[1][k] = o.y;
    }
    if (j.out_flows) {
        aug_store(j.out_flows + (p * 2 + 0) * n + row, x, w, vec, v[0]);
        aug_store(j.out_flows + (p * 2 + 1) * n + row, x, w, vec, v[1]);
    }
    if (j.valid) {
        uint8_t* vr = j.valid + p * n + row;
        if (vec) {
            *reinterpret_cast<uint32_t*>(vr + x) = (uint32_t)ok[0] | (uint32_t)ok[1] << 8 | (uint32_t)ok[2] << 16 | (uint32_t)ok[3] << 24;
        } else {
#pragma unroll
            for (int k = 0; k < AUG_PX; ++k)
                if (x + k < w) vr[x + k] = ok[k];
        }
    }
}

// grid = (ceil(P/256), T, B), block = 256: one point a lane
__global__ __launch_bounds__(256) void k_clip_tracks(ClipTrackJob j)
{
    const unsigned k = blockIdx.x * 256u + threadIdx.x;                              // (P < 2^31: no wrap)
    if (k >= (unsigned)j.P) return;
    const size_t f = (size_t)blockIdx.z * j.T + blockIdx.y, i = f * (size_t)j.P + k;
    const ClipFrameDev& s = j.tab[f];
    const float2 p = j.vec ? reinterpret_cast<const float2*>(j.pos)[i] : make_float2(j.pos[2 * i], j.pos[2 * i + 1]);
    float2 o = aug_apply(s.P, p.x, p.y);
    const bool fin = fabsf(o.x) <= 3.4028235e38f && fabsf(o.y) <= 3.4028235e38f;      // false on NaN
    if (!fin) o = make_float2(0.0f, 0.0f);
    const bool in = fin && o.x >= 0.0f && o.x <= (float)(j.w - 1) && o.y >= 0.0f && o.y <= (float)(j.h - 1);
    if (j.tracks) {
        if (j.vec) reinterpret_cast<float2*>(j.tracks)[i] = o;
        else { j.tracks[2 * i] = o.x; j.tracks[2 * i + 1] = o.y; }
    }
    if (j.vis) {
        bool erased = false;
        if (in) {
            const int rx = (int)floorf(o.x + 0.5f), ry = (int)floorf(o.y + 0.5f);
            for (int e = 0; e < s.n_erase; ++e)
                erased = erased || (rx >= s.erase[e][0] && rx < s.erase[e][2] && ry >= s.erase[e][1] && ry < s.erase[e][3]);
        }
        j.vis[i] = (j.occ[i] == 0 && in && !erased) ? 255 : 0;
    }
}

}  // namespace arap
