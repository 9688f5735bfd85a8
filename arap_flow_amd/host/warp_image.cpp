// warp_image -- C++ host program with the argv contract of ARAP/warping/src/main.cpp:302-336:
//   ./warp_image image mask flow warped_image warped_mask
// The rasterisation runs on the GPU (ArapFlow_Warp); output is bit exact against the reference's executable.
// Optional tokens after the five arguments (addition, DESIGN.md "Backward flow and occlusion"): bwd=PATH.flo,
// occ=PATH.png, occ_bwd=PATH.png; then ArapFlow_WarpEx also writes those maps.  diag=PATH.txt, fold=PATH.png (DESIGN.md
// "Fold diagnostics"): the mesh statistics and the fold map of the flow, through ArapFlow_WarpDiag.
#include <cstdio>
#include <string>
#include <vector>

#include "device_pass.h"
#include "list_line.h"

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
    std::string bwd_path, occ_path, occ_bwd_path, diag_path, fold_path;
    bool extra_ok = argc >= 6;
    for (int a = 6; a < argc && extra_ok; ++a) {
        std::string k, v;
        std::string* dst = split_token(argv[a], k, v)
                               ? field_of({{"bwd", &bwd_path}, {"occ", &occ_path}, {"occ_bwd", &occ_bwd_path},
                                           {"diag", &diag_path}, {"fold", &fold_path}}, k) : nullptr;
        if (dst) *dst = v;
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
    const bool ex = !bwd_path.empty() || !occ_path.empty() || !occ_bwd_path.empty();
    DeviceArena dev;
    const size_t d_rgb = dev.stage(rgb.rgb.data(), 3 * N), d_msk = dev.stage(mred.data(), N), d_flow = dev.stage(flow.data(), 8 * N);
    OutputTable out(dev, w, h);
    const size_t o_rgb = out.add(FileKind::rgb, argv[4]), o_msk = out.add(FileKind::mask1, argv[5]);
    const size_t o_bwd = out.add(FileKind::flo, bwd_path), o_obwd = out.add(FileKind::gray8, occ_bwd_path);
    const size_t o_occ = out.add(FileKind::gray8, occ_path), o_fold = out.add(FileKind::gray8, fold_path);
    const size_t d_stats = diag_path.empty() ? DeviceArena::kNone : dev.take(sizeof(ArapFlow_MeshStats));
    const size_t d_scr = dev.take(ex ? ArapFlow_WarpExScratchBytes((unsigned)w, (unsigned)h)
                                     : ArapFlow_WarpScratchBytes((unsigned)w, (unsigned)h));
    HCHECK(dev.alloc());
    HCHECK(dev.upload());
    if (!ex && ArapFlow_Warp(state, (unsigned)w, (unsigned)h, dev.at(d_rgb), dev.at(d_msk), dev.at(d_flow), out.dev(o_rgb),
                             out.dev(o_msk), dev.at(d_scr)) != 0) { printf("ArapFlow_Warp failed\n"); return 1; }
    if (ex && ArapFlow_WarpEx(state, (unsigned)w, (unsigned)h, dev.at(d_rgb), dev.at(d_msk), dev.at(d_flow), out.dev(o_rgb),
                              out.dev(o_msk), out.dev(o_bwd), out.dev(o_obwd), out.dev(o_occ), dev.at(d_scr)) != 0) {
        printf("ArapFlow_WarpEx failed\n");
        return 1;
    }
    if ((!diag_path.empty() || !fold_path.empty()) &&
        ArapFlow_WarpDiag(state, (unsigned)w, (unsigned)h, dev.at(d_msk), dev.at(d_flow), out.dev(o_fold),
                          (ArapFlow_MeshStats*)dev.at(d_stats)) != 0) { printf("ArapFlow_WarpDiag failed\n"); return 1; }
    HCHECK(hipDeviceSynchronize());
    HCHECK(out.download());
    if (!out.write()) return 1;
    if (!diag_path.empty()) {
        ArapFlow_MeshStats stats;
        HCHECK(hipMemcpy(&stats, dev.at(d_stats), sizeof(stats), hipMemcpyDeviceToHost));
        const std::string text = format_diag(stats);
        if (!save_text(diag_path, text.data(), text.size())) return 1;
    }
    printf("Saved\n");
    return 0;
}
