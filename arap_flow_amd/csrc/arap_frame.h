// arap_frame.h -- the frame solver's per-slot images and the two kernels that prepare them for a solve (gfx950):
// k_frame_reset (resetGPU) and k_frame_ramp (setConstraintImage).  Launched by abi_solver.h: solver_enqueue.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace arap {

struct FrameDev {             // per-slot images owned by the frame solver
    float2 *O, *U, *C, *T, *flow;
    float *A, *M;
    uint8_t *mask, *rgb, *out_rgb, *out_mask;
    unsigned long long* key;
};

// resetGPU (CombinedSolver.h:207-221): U = O = (x,y), A = 0, Mask = (float)red
__global__ __launch_bounds__(256) void k_frame_reset(const FrameDev* fr, int W, int N)
{
    const FrameDev f = fr[blockIdx.z];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int y = i / W, x = i - y * W;
    const float2 g = make_float2((float)x, (float)y);
    f.U[i] = g;
    f.O[i] = g;
    f.A[i] = 0.f;
    f.M[i] = (float)f.mask[i];
}

// setConstraintImage(alpha) (CombinedSolver.h:223-242).  T holds, per source pixel, the target of the
// last constraint placed there (host pre-pass in SetFrame, same overwrite order as the reference's
// loop), or NaN where there is none / where the mask is non-zero.
__global__ __launch_bounds__(256) void k_frame_ramp(const FrameDev* fr, int W, int N, float alpha)
{
    const FrameDev f = fr[blockIdx.z];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float2 t = f.T[i];
    float2 c = make_float2(-1.0f, -1.0f);
    if (t.x == t.x) {
        const int y = i / W, x = i - y * W;
        c.x = (1.0f - alpha) * (float)x + alpha * t.x;
        c.y = (1.0f - alpha) * (float)y + alpha * t.y;
    }
    f.C[i] = c;
}

}  // namespace arap
