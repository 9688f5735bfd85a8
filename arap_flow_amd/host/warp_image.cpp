// warp_image -- C++ host program with the argv contract of ARAP/warping/src/main.cpp:302-336:
//   ./warp_image image mask flow warped_image warped_mask
// The rasterisation runs on the GPU (ArapFlow_Warp); output is bit exact against the reference's executable.
// Optional tokens after the five arguments (addition, DESIGN.md "Backward flow and occlusion"): bwd=PATH.flo,
// occ=PATH.png, occ_bwd=PATH.png; then ArapFlow_WarpEx also writes those maps.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <string>
#include <vector>

extern "C" {
#include "../../include/arap_opt.h"
}
#include "flo_io.h"
#include "png_io.h"

static void usage()
{
#define p(msg) printf(msg "\n");
    p("Usage:");
    p("./warp_image image mask flow warped_image warped_mask");
    p("Mask and warp image using the provided optical flow field.")
    p("\timage: path to image with png extension")
    p("\tmask: path to mask image with png extension, 0 for object, 1 for background")
    p("\tflo: path to optical flow image with flo extension")
    p("\twarped_image: path to output warped image (.png), all intermediate directories must exist")
    p("\twarped_mask: path to output warped mask (.png), all intermediate directories must exist")
#undef p
}

#define HCHECK(c) do { hipError_t e_ = (c); if (e_ != hipSuccess) { printf("HIP error %d at %s:%d\n", (int)e_, __FILE__, __LINE__); return 1; } } while (0)

int main(int argc, const char* argv[])
{
    std::string bwd_path, occ_path, occ_bwd_path;
    bool extra_ok = argc >= 6;
    for (int a = 6; a < argc && extra_ok; ++a) {
        const std::string t = argv[a];
        if (t.compare(0, 4, "bwd=") == 0) bwd_path = t.substr(4);
        else if (t.compare(0, 4, "occ=") == 0) occ_path = t.substr(4);
        else if (t.compare(0, 8, "occ_bwd=") == 0) occ_bwd_path = t.substr(8);
        else extra_ok = false;
    }
    if (!extra_ok) {
        printf("Invalid Input! ");
        usage();
        return 1;
    }
    std::string err;
    arapio::Image rgb, msk;
    if (!arapio::read_png_rgb(argv[1], rgb, err) || !arapio::read_png_rgb(argv[2], msk, err)) { printf("%s\n", err.c_str()); return 1; }
    std::vector<float> flow;
    int fw = 0, fh = 0;
    if (!arapio::read_flo(argv[3], flow, fw, fh)) return 1;
    if (fw != rgb.w || fh != rgb.h || msk.w != rgb.w || msk.h != rgb.h) { printf("image, mask and flow sizes differ\n"); return 1; }
    const int w = rgb.w, h = rgb.h;
    const size_t N = (size_t)w * h;
    std::vector<uint8_t> mred(N);
    for (size_t i = 0; i < N; ++i) mred[i] = msk.rgb[3 * i];
    Opt_InitializationParameters ip = {0, 0, 0, 0};
    Opt_State* state = Opt_NewState(ip);
    if (!state) return 1;
    void *d_rgb, *d_msk, *d_flow, *d_orgb, *d_omsk, *d_scr;
    HCHECK(hipMalloc(&d_rgb, 3 * N)); HCHECK(hipMalloc(&d_msk, N)); HCHECK(hipMalloc(&d_flow, 8 * N));
    HCHECK(hipMalloc(&d_orgb, 3 * N)); HCHECK(hipMalloc(&d_omsk, N));
    const bool ex = !bwd_path.empty() || !occ_path.empty() || !occ_bwd_path.empty();
    void *d_bwd = nullptr, *d_obwd = nullptr, *d_occ = nullptr;
    if (!bwd_path.empty()) HCHECK(hipMalloc(&d_bwd, 8 * N));
    if (!occ_bwd_path.empty()) HCHECK(hipMalloc(&d_obwd, N));
    if (!occ_path.empty()) HCHECK(hipMalloc(&d_occ, N));
    HCHECK(hipMalloc(&d_scr, ex ? ArapFlow_WarpExScratchBytes((unsigned)w, (unsigned)h)
                                : ArapFlow_WarpScratchBytes((unsigned)w, (unsigned)h)));
    HCHECK(hipMemcpy(d_rgb, rgb.rgb.data(), 3 * N, hipMemcpyHostToDevice));
    HCHECK(hipMemcpy(d_msk, mred.data(), N, hipMemcpyHostToDevice));
    HCHECK(hipMemcpy(d_flow, flow.data(), 8 * N, hipMemcpyHostToDevice));
    if (!ex && ArapFlow_Warp(state, (unsigned)w, (unsigned)h, d_rgb, d_msk, d_flow, d_orgb, d_omsk, d_scr) != 0) { printf("ArapFlow_Warp failed\n"); return 1; }
    if (ex && ArapFlow_WarpEx(state, (unsigned)w, (unsigned)h, d_rgb, d_msk, d_flow, d_orgb, d_omsk, d_bwd, d_obwd, d_occ,
                              d_scr) != 0) { printf("ArapFlow_WarpEx failed\n"); return 1; }
    HCHECK(hipDeviceSynchronize());
    std::vector<uint8_t> orgb(3 * N), omsk(N);
    HCHECK(hipMemcpy(orgb.data(), d_orgb, 3 * N, hipMemcpyDeviceToHost));
    HCHECK(hipMemcpy(omsk.data(), d_omsk, N, hipMemcpyDeviceToHost));
    if (!arapio::write_png_rgb(argv[4], w, h, orgb.data(), err) || !arapio::write_png_mask1(argv[5], w, h, omsk.data(), err)) {
        printf("%s\n", err.c_str());
        return 1;
    }
    if (d_bwd) {
        std::vector<float> bwd(2 * N);
        HCHECK(hipMemcpy(bwd.data(), d_bwd, 8 * N, hipMemcpyDeviceToHost));
        if (!arapio::write_flo(bwd_path, bwd.data(), w, h)) return 1;
    }
    for (auto po : {std::make_pair(d_obwd, &occ_bwd_path), std::make_pair(d_occ, &occ_path)}) {
        if (!po.first) continue;
        std::vector<uint8_t> m(N);
        HCHECK(hipMemcpy(m.data(), po.first, N, hipMemcpyDeviceToHost));
        if (!arapio::write_png_gray8(*po.second, w, h, m.data(), err)) { printf("%s\n", err.c_str()); return 1; }
    }
    printf("Saved\n");
    return 0;
}
