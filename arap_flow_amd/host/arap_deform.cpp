// arap_deform -- C++ host program over libarapopt.so with the argv contract, schedule and outputs of the
// reference's executable (ARAP/deformation/src/main.cpp:162-241 + CombinedSolver.h + CombinedSolverBase.h):
//   ./arap_deform RGB Mask Constraint Flow warped_RGB warped_Mask        (one frame)
//   ./arap_deform listfile                                               (six paths per line)
//   ./arap_deform --serve                                                (addition: the same lines on stdin, until EOF)
// A list or --serve line may carry optional tokens after its six paths (addition, DESIGN.md "Backward flow and
// occlusion"): bwd=PATH.flo (backward flow), occ=PATH.png (forward occlusion), occ_bwd=PATH.png (backward
// occlusion), 8-bit 0/255, and mid=I1,I2,..:PREFIX (DESIGN.md "In-between frames"): the in-between frames after the
// ramp steps I1 < I2 < .., written as PREFIX_sII.flo, PREFIX_sII.png, PREFIX_sII_mask.png and PREFIX_sII_step.flo (II:
// the step, two digits) in the formats of the line's own flow, warped RGB and warped mask.  All mid= lines of a batch
// must name the same steps.  diag=PATH.txt and fold=PATH.png (DESIGN.md "Fold diagnostics"): the mesh statistics of the
// solve as text (pipeline.format_diag) and its fold map, 8-bit 0/255; a batch computes them iff one of its lines asks.
// Other trailing tokens are ignored, as before.
// A line whose first word is `layers` is no solve but the layered warp of one frame (DESIGN.md "Layered warp"):
//   layers RGB n MASK_1 FLO_1 ... MASK_n FLO_n [occ=P] [bwd=P] [occ_bwd=P] [rgb2=P] [mask2=P] [mid=I1,I2,..:PREFIX]
// (at least one output).  Its mid= token (DESIGN.md "Layered in-between frames") reads every layer's snapshot flows
// STEM_l_sII.flo, STEM_l = FLO_l without `.flo`, and writes per snapshot the composite PREFIX_sII.flo, PREFIX_sII.png,
// PREFIX_sII_mask.png, PREFIX_sII_step.flo and, with occ= on the line, the link occlusions PREFIX_s00_occ.png (frame 1
// -> first snapshot) and PREFIX_sII_occ.png (snapshot -> next state).
// A line whose first word is `bg` is the moving-background pass of one pair (DESIGN.md "Moving background"; with mid= also
// of its in-between frames, "Moving background over in-between frames"):
//   bg BG.png RGB1.png MASK1.png RGB2.png MASK2.png FLOW.flo m=<12 numbers, M1 then M2, comma separated>
//      [occ=IN] [bwd=IN] [occ_bwd=IN] out=RGB1_OUT.png,RGB2_OUT.png,FLOW_OUT.flo [occ_out=P] [bwd_out=P] [occ_bwd_out=P]
// (MASK1: red 0 = object; MASK2: a warped mask, non-zero = object; a place of out= may be empty; at least one output).
// With mid=I1,..,In:PREFIX mm=<6n numbers> mid_out=PREFIX_OUT (all three or none) the line also makes one sequence pass over
// frame 1, the in-between frames PREFIX_sII{.png,_mask.png,_step.flo} (PREFIX_sI1.flo for the first link; with occ= also
// PREFIX_s00_occ.png, PREFIX_sII_occ.png) and frame 2, with the cameras mm= gives the in-between frames, and writes
// PREFIX_OUT_sII.png, PREFIX_OUT_s00_step.flo, PREFIX_OUT_sII_step.flo and, with occ=, PREFIX_OUT_s00_occ.png, _sII_occ.png.
// It answers "Done <first output: the places of out=, then occ_out, bwd_out, occ_bwd_out, then PREFIX_OUT_sI1.png>".
// A line whose first word is `tex` is the random-texture twin of one frame (DESIGN.md "Random textures"):
//   tex RGB n MASK_1 FLO_1 ... MASK_n FLO_n t=<layer 1>;...;<layer n> [rgb1=P] [rgb2=P] [mask2=P]
// (the layers of the frame's layers line; a layer of t= is 19 numbers, comma separated: kind, seed, the six of the map,
// p0, p1, nine palette bytes; at least one output).  rgb1: frame 1 with a procedural texture on every layer's object;
// rgb2 / mask2: its layered warp with the layers' flows, which are read only then.
// A line whose first word is `trk` is the point tracks of one sequence (DESIGN.md "Point tracks"):
//   trk PTS.trk n T  MASK_1 FLO_1,1 .. FLO_1,T  ..  MASK_n FLO_n,1 .. FLO_n,T  out=OUT.trk
// (PTS.trk: a points file, trk_io.h; every state file of every layer is named; OUT.trk has T + 1 frames, the points first).
// A line whose first word is `blur` is the two motion-blurred frames of one pair (DESIGN.md "Motion blur"):
//   blur RGB n MASK_1 FLO_1 ... MASK_n FLO_n BG.png b=<shutter>,<samples> [m=<12 numbers: M1 then M2>]
//        [rgb1=P] [rgb2=P] [alpha1=P] [alpha2=P]
// (the layers of the frame's layers line; BG.png shows behind them through the cameras of m=, the identity without it; at
// least one output).  rgb1 / alpha1: the frame exposed around t = 0; rgb2 / alpha2: around t = 1, the same shutter.
// A line whose first word is `light` is the relit variant of one pair (DESIGN.md "Relit frames"):
//   light RGB1 MASK1 RGB2 COVER2 l=<frame 1>;<frame 2> [rgb1=P] [rgb2=P]
// (the pair's finished frames; MASK1 in the solver's convention, COVER2 a cover; a frame of l= is the 19 numbers of
// ArapFlow_LightFrame; at least one output).
// A line whose first word is `seg` is the segment maps of one pair (DESIGN.md "Segment maps"):
//   seg n MASK_1 FLO_1 ... MASK_n FLO_n s=<tau>,<radius> [m=<12 numbers: M1 then M2>]
//       [idx1=P] [idx2=P] [mb1=P] [mb2=P] [dist1=P] [dist2=P]
// (the layers of the frame's layers line; a static background without m=; 8-bit L PNGs, a distance as its integer square
// root with 255 for "further than the radius"; at least one output).
// A line whose first word is `score` is the error table of one estimated flow (DESIGN.md "Flow scoring"):
//   score GT.flo EST.flo [occ=PNG] [dist=PNG] [skip=PNG] [mask=PNG] out=TXT
// (occ: non-zero = occluded; dist: the 8-bit distance file of a seg line; skip: non-zero = left out; mask: red != 0 is not
// object and left out too; out: the table as text, pipeline.format_score).
// A line whose first word is `tscore` is the TAP-Vid table of one estimated track file (DESIGN.md "Track scoring"):
//   tscore GT.trk EST.trk [s=SX,SY] out=TXT
// (the files agree in W, H, F, P; s: the factors the error is taken under; out: the table as text,
// pipeline.format_track_score), and one whose first word is `chain` the track file of chained flow estimates:
//   chain PTS.trk L FLO_1 .. FLO_L [bwd=B_1,..,B_L] out=OUT.trk
// (the query points are frame 0 of PTS.trk; every flow has its W, H; OUT.trk has L + 1 frames).
// A line whose first word is `fscore` is the PSNR / SSIM table of one estimated frame (DESIGN.md "Frame scoring"):
//   fscore REF.png EST.png [occ=PNG] [dist=PNG] [skip=PNG] [obj=PNG] out=TXT
// (occ: non-zero = occluded; dist: the 8-bit distance file of a seg line; skip: non-zero = left out; obj: red == 0 is
// object, anything else background; out: the table as text, pipeline.format_frame_score).
// A line whose first word is `interp` is the in-between frames of a pair from a flow estimate (DESIGN.md "Frames from flows"):
//   interp A.png B.png FWD.flo s=I1,I2,.. n=N [bwd=BWD.flo] [src=1] out=PREFIX
// (the times are (float)I / (float)N; written: PREFIX_sII.png and, with src=1, the source maps PREFIX_sII_src.png).
// A line whose first word is `lscore` is the DAVIS J / F table of one estimated label map, one whose first word is `mscore`
// the precision / recall table of one estimated occlusion or motion-boundary map (DESIGN.md "Map scoring"):
//   lscore GT.png EST.png l=<L> r=<radius> [skip=PNG] out=TXT
//   mscore GT.png EST.png [t=<thr,...> r=<radius>] [skip=PNG] out=TXT
// (the red channel of every PNG; skip: non-zero = left out; out: the table as text, pipeline.format_label_score /
// format_map_score).
// Any of these runs on the solver's own stream between batches; in a list every earlier line is finished and written first (its
// inputs may be their outputs); --serve answers "Done <path of the first output token on the line>".
// The reference keeps one CombinedSolver (one Opt plan) and feeds it frame after frame (main.cpp:223-238);
// here consecutive frames of equal size are handed to the device-resident batched solver, as many as fit one launch
// (ArapFlow_Solver = CombinedSolver on the GPU: reset, 19-step constraint ramp, 8 GN x 400 PCG, flow, rasteriser).
//
// The GPU never waits for the host: two solver objects alternate.  While one batch is being solved, the next one is
// decoded (worker threads), uploaded into the other object (its own copy stream, pinned staging) and the previous
// batch's results are read back and encoded (worker threads).  --serve is what para_gen.py starts once per GPU: a
// persistent worker that is fed list-file lines over a pipe as the front end produces them and reports
// "Done <flow path>" per finished solve, instead of one child process (HIP start-up, plan, graph capture) per hand-out.
// The grammar of a line is list_line.h; the device layout and the file writer of the synchronous passes are device_pass.h.
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fstream>
#include <future>
#include <iostream>
#include <memory>
#include <mutex>
#include <thread>
#include <unistd.h>

#include "device_pass.h"
#include "list_line.h"
#include "trk_io.h"

// the usage text of the reference's executable (main.cpp:13-24), verbatim: it is part of the CLI contract
static const char kUsage[] =
    "Usage:\n\n"
    "./arap_deform RGB Mask Constraint Flow warped_RGB warped_Mask\n\n"
    "Mask and warp image using the provided optical flow field.\n\n"
    "RGB \t\t [input]  path to an input RGB image (.png only)\n"
    "Mask\t\t [input]  path to an input mask image (.png only) where 0 for object, 1 for background\n"
    "Constraint \t [input]  path to list of constraints, text file\n"
    "Flow \t\t [output] path to optical flow image with (.flo only)\n"
    "warped_RGB \t [output] path to output warped image (.png), all intermediate directories must exist\n"
    "warped_Mask \t [output] path to output warped mask (.png), all intermediate directories must exist\n";

// `return fail(...)`: a step says why it gives up
__attribute__((format(printf, 1, 2))) static bool fail(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vprintf(fmt, ap);
    va_end(ap);
    return false;
}

// constraint file (main.cpp:26-50): a count n, then n rows of four integers x1 y1 x2 y2
static bool read_constraint_file(const std::string& path, std::vector<int32_t>& rows)
{
    FILE* f = fopen(path.c_str(), "r");
    if (!f) return fail("Could not open marker file %s\n", path.c_str());
    unsigned n = 0;
    rows.clear();
    if (fscanf(f, "%u", &n) == 1) {
        rows.reserve(4 * (size_t)n);
        for (size_t k = 0; k < 4 * (size_t)n; ++k) {
            int v = 0;
            if (fscanf(f, "%d", &v) != 1) v = 0;       // the reference's stream extraction leaves 0 on a short file
            rows.push_back(v);
        }
    }
    fclose(f);
    return true;
}

static bool read_png(const std::string& path, arapio::Image& im)       // says why not
{
    std::string err;
    return arapio::read_png_rgb(path, im, err) || fail("%s\n", err.c_str());
}

static std::vector<uint8_t> red_channel(const arapio::Image& im)
{
    std::vector<uint8_t> red(im.rgb.size() / 3);
    for (size_t i = 0; i < red.size(); ++i) red[i] = im.rgb[3 * i];
    return red;
}

struct Frame {                             // a line and, for a solve line, its decoded inputs (ok: they could be read)
    Item item;
    bool ok = true;
    arapio::Image rgb;
    std::vector<uint8_t> mask_red;
    std::vector<int32_t> constraints;      // x1 y1 x2 y2 rows, file order then border pins
};

// loadData of the reference (main.cpp:116-138): constraints file, PNGs, then a pin-to-self constraint for every border pixel
static bool load_frame(Frame& f)
{
    const SolvePaths& paths = f.item.solve;
    if (!read_constraint_file(paths.constraints, f.constraints)) return false;
    arapio::Image msk;
    if (!read_png(paths.rgb, f.rgb) || !read_png(paths.mask, msk)) return false;
    if (msk.w != f.rgb.w || msk.h != f.rgb.h)
        return fail("Mask %s and image %s differ in size\n", paths.mask.c_str(), paths.rgb.c_str());
    const int width = f.rgb.w, height = f.rgb.h;
    f.mask_red = red_channel(msk);
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++)
            if (y == 0 || x == 0 || y == (height - 1) || x == (width - 1)) {
                f.constraints.push_back(x); f.constraints.push_back(y);
                f.constraints.push_back(x); f.constraints.push_back(y);
            }
    return true;
}

// the mid= token of a layers line (pipeline.run_layers_mid): `masks` [n][N] and `flows` [n][N][2] are the line's
// layers, already read.  One ArapFlow_WarpLayersStep per snapshot on the state's stream, synchronously.
static bool run_layers_mid(Opt_State* state, const LayersSpec& q, const arapio::Image& rgb,
                           const std::vector<uint8_t>& masks, const std::vector<float>& flows)
{
    const int w = rgb.w, h = rgb.h;
    const unsigned W = (unsigned)w, H = (unsigned)h, n = (unsigned)q.masks.size();
    const size_t N = (size_t)w * h, ns = q.mid.steps.size(), layer_bytes = n * N * 8;
    // states[k]: the layers' flows after snapshot k; states[ns]: the final flows
    std::vector<std::vector<float>> states(ns);
    for (size_t k = 0; k < ns; ++k) {
        states[k].resize(n * N * 2);
        for (size_t l = 0; l < n; ++l) {
            const std::string& f = q.flows[l];
            if (f.size() < 4 || f.compare(f.size() - 4, 4, ".flo") != 0)
                return fail("layers: mid= needs flows named *.flo, got %s\n", f.c_str());
            const std::string snap = mid_stem(f.substr(0, f.size() - 4), q.mid.steps[k]) + ".flo";
            std::vector<float> fl;
            int fw = 0, fh = 0;
            if (!arapio::read_flo(snap, fl, fw, fh)) return fail("layers: snapshot %s is missing\n", snap.c_str());
            if (fw != w || fh != h) return fail("layers: %s differs in size from %s\n", snap.c_str(), q.rgb.c_str());
            memcpy(states[k].data() + l * N * 2, fl.data(), N * 8);
        }
    }
    DeviceArena dev;
    const size_t d_rgb = dev.stage(rgb.rgb.data(), 3 * N), d_msk = dev.stage(masks.data(), n * N);
    const size_t d_a = dev.take(layer_bytes), d_b = dev.take(layer_bytes);
    OutputTable out(dev, w, h);            // named per call; the link occlusions only with occ= on the line
    const size_t o_step = out.add(FileKind::flo, "", true), o_rgb = out.add(FileKind::rgb, "", true);
    const size_t o_msk = out.add(FileKind::mask1, "", true), o_occ = out.add(FileKind::gray8, "", !q.occ.empty());
    const size_t d_scr = dev.take(std::max(ArapFlow_WarpLayersStepScratchBytes(W, H, n), ArapFlow_WarpLayersScratchBytes(W, H, n)));
    if (dev.alloc() != hipSuccess) return fail("layers: out of device memory\n");
    auto put = [&](size_t part, size_t k) {
        return dev.copy_in(part, k < ns ? states[k].data() : flows.data(), layer_bytes) == hipSuccess;
    };
    // ok: the device work went through; wrote: so did the files (a file that did not has said so itself)
    bool ok = dev.upload() == hipSuccess, wrote = true;
    if (ok && !q.occ.empty()) {               // frame 1 -> first snapshot: the layered warp's occlusion of that state
        out.set_path(o_occ, mid_stem(q.mid.prefix, 0) + "_occ.png");
        ok = put(d_a, 0) &&
             ArapFlow_WarpLayers(state, W, H, n, nullptr, dev.at(d_msk), dev.at(d_a), out.dev(o_rgb), out.dev(o_msk), nullptr,
                                 nullptr, out.dev(o_occ), dev.at(d_scr)) == 0 &&
             hipDeviceSynchronize() == hipSuccess && out.download() == hipSuccess;
        if (ok) wrote = out.write();
    }
    std::vector<float> own(N * 2);
    for (size_t k = 0; ok && wrote && k < ns; ++k) {
        const std::string stem = mid_stem(q.mid.prefix, q.mid.steps[k]);
        out.set_path(o_step, stem + "_step.flo");
        out.set_path(o_rgb, stem + ".png");
        out.set_path(o_msk, stem + "_mask.png");
        out.set_path(o_occ, stem + "_occ.png");
        ok = put(d_a, k) && put(d_b, k + 1) &&
             ArapFlow_WarpLayersStep(state, W, H, n, dev.at(d_rgb), dev.at(d_msk), dev.at(d_a), dev.at(d_b), out.dev(o_rgb),
                                     out.dev(o_msk), out.dev(o_step), out.dev(o_occ), dev.at(d_scr)) == 0 &&
             hipDeviceSynchronize() == hipSuccess && out.download() == hipSuccess;
        if (!ok) break;
        // the composite frame-1 flow: per pixel the snapshot flow of its owner, the largest l with mask_l == 0
        for (size_t i = 0; i < N; ++i) {
            own[2 * i] = own[2 * i + 1] = 0.f;
            for (size_t l = n; l-- > 0;)
                if (masks[l * N + i] == 0) {
                    own[2 * i] = states[k][(l * N + i) * 2];
                    own[2 * i + 1] = states[k][(l * N + i) * 2 + 1];
                    break;
                }
        }
        wrote = save(FileKind::flo, stem + ".flo", w, h, own.data()) && out.write();
    }
    if (!ok) printf("ArapFlow_WarpLayersStep failed\n");
    return ok && wrote;
}

// the files of a frame's layers, read once: the RGB, every layer's mask (red channel, [n][N]) and -- `with_flows` -- flow
// ([n][N][2]); `form`: the line's first word, for the messages
static bool read_layer_files(const char* form, const std::string& rgb_path, const std::vector<std::string>& mask_paths,
                             const std::vector<std::string>& flow_paths, bool with_flows, arapio::Image& rgb,
                             std::vector<uint8_t>& masks, std::vector<float>& flows)
{
    if (!read_png(rgb_path, rgb)) return false;
    const int w = rgb.w, h = rgb.h;
    const size_t N = (size_t)w * h, n = mask_paths.size();
    masks.resize(n * N);
    if (with_flows) flows.resize(n * N * 2);
    for (size_t l = 0; l < n; ++l) {
        arapio::Image msk;
        if (!read_png(mask_paths[l], msk)) return false;
        std::vector<float> fl;
        int fw = w, fh = h;
        if (with_flows && !arapio::read_flo(flow_paths[l], fl, fw, fh)) return fail("Could not read %s\n", flow_paths[l].c_str());
        if (msk.w != w || msk.h != h || fw != w || fh != h)
            return fail("%s: %s / %s differ in size from %s\n", form, mask_paths[l].c_str(), flow_paths[l].c_str(), rgb_path.c_str());
        for (size_t i = 0; i < N; ++i) masks[l * N + i] = msk.rgb[3 * i];      // red channel
        if (with_flows) memcpy(flows.data() + l * N * 2, fl.data(), N * 8);
    }
    return true;
}

// the random-texture twin of one frame, synchronously (pipeline.run_texture): read the layers' files once, one
// ArapFlow_Texture on the state's stream and, if rgb2 or mask2 is wanted, one ArapFlow_WarpLayers on its result (the
// retextured frame stays on the device), write the outputs asked for
static bool run_texture(Opt_State* state, const TexSpec& q)
{
    const bool warp = !q.rgb2.empty() || !q.mask2.empty();
    arapio::Image rgb;
    std::vector<uint8_t> masks;
    std::vector<float> flows;
    if (!read_layer_files("tex", q.rgb, q.masks, q.flows, warp, rgb, masks, flows)) return false;
    const int w = rgb.w, h = rgb.h;
    const unsigned W = (unsigned)w, H = (unsigned)h, n = (unsigned)q.masks.size();
    const size_t N = (size_t)w * h;
    DeviceArena dev;
    const size_t d_rgb = dev.stage(rgb.rgb.data(), 3 * N), d_msk = dev.stage(masks.data(), n * N);
    const size_t d_flow = warp ? dev.stage(flows.data(), n * N * 8) : DeviceArena::kNone;
    OutputTable out(dev, w, h);
    const size_t o_rgb1 = out.add(FileKind::rgb, q.rgb1, true);            // the warp's input, written or not
    const size_t o_rgb2 = out.add(FileKind::rgb, q.rgb2), o_msk2 = out.add(FileKind::mask1, q.mask2);
    const size_t d_scr = warp ? dev.take(ArapFlow_WarpLayersScratchBytes(W, H, n)) : DeviceArena::kNone;
    if (dev.alloc() != hipSuccess) return fail("tex: out of device memory\n");
    void* const rgb1 = out.part(o_rgb1);
    bool ok = dev.upload() == hipSuccess &&
              ArapFlow_Texture(state, W, H, n, dev.at(d_rgb), dev.at(d_msk), q.tex.data(), rgb1) == 0;
    if (ok && warp)
        ok = ArapFlow_WarpLayers(state, W, H, n, rgb1, dev.at(d_msk), dev.at(d_flow), out.dev(o_rgb2), out.dev(o_msk2), nullptr,
                                 nullptr, nullptr, dev.at(d_scr)) == 0;
    ok = ok && hipDeviceSynchronize() == hipSuccess && out.download() == hipSuccess;
    return ok ? out.write() : fail("ArapFlow_Texture failed\n");
}

// the motion-blurred frames of one pair, synchronously (pipeline.run_blur): read the layers' files and the background
// picture once, one ArapFlow_BlurLayers on the state's stream per frame the line asks for (centre 0, centre 1) with one
// scratch buffer, write the outputs asked for
static bool run_blur(Opt_State* state, const BlurSpec& q)
{
    arapio::Image rgb, bg;
    std::vector<uint8_t> masks;
    std::vector<float> flows;
    if (!read_layer_files("blur", q.rgb, q.masks, q.flows, true, rgb, masks, flows) || !read_png(q.bg, bg)) return false;
    const int w = rgb.w, h = rgb.h;
    const unsigned W = (unsigned)w, H = (unsigned)h, n = (unsigned)q.masks.size();
    const size_t N = (size_t)w * h;
    const uint64_t scratch = ArapFlow_BlurLayersScratchBytes(W, H, n, q.samples);
    if (scratch == 0) return fail("blur: %u samples of %u layers on %d x %d: beyond the limits\n", q.samples, n, w, h);
    DeviceArena dev;
    const size_t d_rgb = dev.stage(rgb.rgb.data(), 3 * N), d_msk = dev.stage(masks.data(), n * N);
    const size_t d_flow = dev.stage(flows.data(), n * N * 8), d_bg = dev.stage(bg.rgb.data(), bg.rgb.size());
    OutputTable out(dev, w, h);
    const size_t o_rgb[2] = {out.add(FileKind::rgb, q.rgb1), out.add(FileKind::rgb, q.rgb2)};
    const size_t o_alpha[2] = {out.add(FileKind::gray8, q.alpha1), out.add(FileKind::gray8, q.alpha2)};
    const size_t d_scr = dev.take(scratch);
    if (dev.alloc() != hipSuccess) return fail("blur: out of device memory\n");
    bool ok = dev.upload() == hipSuccess;
    for (int f = 0; ok && f < 2; ++f)
        if (out.dev(o_rgb[f]) || out.dev(o_alpha[f]))
            ok = ArapFlow_BlurLayers(state, W, H, n, dev.at(d_rgb), dev.at(d_msk), nullptr, dev.at(d_flow), (float)f, q.shutter,
                                     q.samples, dev.at(d_bg), (unsigned)bg.w, (unsigned)bg.h, q.m, q.m + 6, out.dev(o_rgb[f]),
                                     out.dev(o_alpha[f]), dev.at(d_scr)) == 0;
    ok = ok && hipDeviceSynchronize() == hipSuccess && out.download() == hipSuccess;
    return ok ? out.write() : fail("ArapFlow_BlurLayers failed\n");
}

// the relit frames of one pair, synchronously (pipeline.run_light): per frame the line asks for, read the frame and its
// mask (red channel), one ArapFlow_Relight on the state's stream -- frame 1 with MASK1 in the solver's convention, frame 2
// with COVER2 as a cover --, write the output
static bool run_light(Opt_State* state, const LightSpec& q)
{
    for (int f = 0; f < 2; ++f) {
        const std::string& out_path = f ? q.out2 : q.out1;
        if (out_path.empty()) continue;
        const std::string &rgb_path = f ? q.rgb2 : q.rgb1, &mask_path = f ? q.cover2 : q.mask1;
        arapio::Image rgb, msk;
        if (!read_png(rgb_path, rgb) || !read_png(mask_path, msk)) return false;
        if (msk.w != rgb.w || msk.h != rgb.h)
            return fail("light: %s differs in size from %s\n", mask_path.c_str(), rgb_path.c_str());
        const size_t N = (size_t)rgb.w * rgb.h;
        std::vector<uint8_t> cover(N);
        for (size_t i = 0; i < N; ++i) cover[i] = msk.rgb[3 * i];             // red channel
        DeviceArena dev;
        const size_t d_rgb = dev.stage(rgb.rgb.data(), 3 * N), d_cov = dev.stage(cover.data(), N);
        OutputTable out(dev, rgb.w, rgb.h);
        const size_t o_rgb = out.add(FileKind::rgb, out_path);
        if (dev.alloc() != hipSuccess) return fail("light: out of device memory\n");
        const bool ok = dev.upload() == hipSuccess &&
                        ArapFlow_Relight(state, (unsigned)rgb.w, (unsigned)rgb.h, dev.at(d_rgb), dev.at(d_cov), f == 0, &q.frames[f],
                                         out.dev(o_rgb)) == 0 &&
                        hipDeviceSynchronize() == hipSuccess && out.download() == hipSuccess;
        if (!ok) return fail("ArapFlow_Relight failed\n");
        if (!out.write()) return false;
    }
    return true;
}

// the segment maps of one pair, synchronously (pipeline.run_seg): read every layer's mask (red channel) and flow, one
// ArapFlow_SegMaps on the state's stream, write the outputs asked for as 8-bit L PNGs: the labels and the 0 / 255 maps as
// they are, a distance as the integer square root of the device's squared value, 255 for its sentinel
static bool run_seg(Opt_State* state, const SegSpec& q)
{
    const unsigned n = (unsigned)q.masks.size();
    std::vector<uint8_t> masks;
    std::vector<float> flows;
    int w = 0, h = 0;
    size_t N = 0;
    for (unsigned l = 0; l < n; ++l) {
        arapio::Image msk;
        std::vector<float> fl;
        int fw = 0, fh = 0;
        if (!read_png(q.masks[l], msk)) return false;
        if (!arapio::read_flo(q.flows[l], fl, fw, fh)) return fail("Could not read %s\n", q.flows[l].c_str());
        if (l == 0) {
            w = msk.w; h = msk.h; N = (size_t)w * h;
            masks.resize(n * N);
            flows.resize(n * N * 2);
        }
        if (msk.w != w || msk.h != h || fw != w || fh != h)
            return fail("seg: %s / %s differ in size from %s\n", q.masks[l].c_str(), q.flows[l].c_str(), q.masks[0].c_str());
        for (size_t i = 0; i < N; ++i) masks[l * N + i] = msk.rgb[3 * i];      // red channel
        memcpy(flows.data() + l * N * 2, fl.data(), N * 8);
    }
    const unsigned W = (unsigned)w, H = (unsigned)h;
    const uint64_t scratch = ArapFlow_SegMapsScratchBytes(W, H, n);
    if (scratch == 0) return fail("seg: %u layers on %d x %d: beyond the limits\n", n, w, h);
    DeviceArena dev;
    const size_t d_msk = dev.stage(masks.data(), n * N), d_flow = dev.stage(flows.data(), n * N * 8);
    OutputTable out(dev, w, h);
    const size_t o_idx1 = out.add(FileKind::gray8, q.idx1), o_idx2 = out.add(FileKind::gray8, q.idx2);
    const size_t o_mb1 = out.add(FileKind::gray8, q.mb1), o_mb2 = out.add(FileKind::gray8, q.mb2);
    const std::string* const dist_path[2] = {&q.dist1, &q.dist2};
    size_t d_dist[2];
    for (int f = 0; f < 2; ++f) d_dist[f] = dist_path[f]->empty() ? DeviceArena::kNone : dev.take(2 * N);
    const size_t d_scr = dev.take(scratch);
    if (dev.alloc() != hipSuccess) return fail("seg: out of device memory\n");
    bool ok = dev.upload() == hipSuccess &&
              ArapFlow_SegMaps(state, W, H, n, dev.at(d_msk), dev.at(d_flow), q.have_m ? q.m : nullptr, q.have_m ? q.m + 6 : nullptr,
                               q.tau, q.radius, out.dev(o_idx1), out.dev(o_idx2), out.dev(o_mb1), out.dev(o_mb2),
                               dev.at(d_dist[0]), dev.at(d_dist[1]), dev.at(d_scr)) == 0 &&
              hipDeviceSynchronize() == hipSuccess && out.download() == hipSuccess;
    std::vector<uint16_t> d2(N);
    std::vector<uint8_t> root[2];
    for (int f = 0; ok && f < 2; ++f) {
        if (d_dist[f] == DeviceArena::kNone) continue;
        ok = hipMemcpy(d2.data(), dev.at(d_dist[f]), 2 * N, hipMemcpyDeviceToHost) == hipSuccess;
        root[f].resize(N);
        for (size_t i = 0; i < N; ++i) {
            unsigned r = 0;
            while ((r + 1) * (r + 1) <= (unsigned)d2[i]) ++r;                 // (at most 255 steps; the sentinel gives 255)
            root[f][i] = (uint8_t)r;
        }
    }
    if (!ok) return fail("ArapFlow_SegMaps failed\n");
    if (!out.write()) return false;
    for (int f = 0; f < 2; ++f)
        if (!root[f].empty() && !save(FileKind::gray8, *dist_path[f], w, h, root[f].data())) return false;
    return true;
}

// the error table of one estimate, synchronously (pipeline.run_score): read the two flows and the planes the line names
// (red channels), the distance file back to squared distances (pipeline.dist_from_png), skip= and mask= OR-ed into the one
// skip plane, one ArapFlow_FlowScore on the state's stream, write the table as text
static bool run_score(Opt_State* state, const ScoreSpec& q)
{
    std::vector<float> gt, est;
    int w = 0, h = 0, ew = 0, eh = 0;
    if (!arapio::read_flo(q.gt, gt, w, h)) return fail("Could not read %s\n", q.gt.c_str());
    if (!arapio::read_flo(q.est, est, ew, eh)) return fail("Could not read %s\n", q.est.c_str());
    if (ew != w || eh != h) return fail("score: %s differs in size from %s\n", q.est.c_str(), q.gt.c_str());
    const size_t N = (size_t)w * h;
    std::vector<uint8_t> occ, skip;
    std::vector<uint16_t> dist;
    const std::string* const paths[4] = {&q.occ, &q.dist, &q.skip, &q.mask};
    for (int k = 0; k < 4; ++k) {
        if (paths[k]->empty()) continue;
        arapio::Image im;
        if (!read_png(*paths[k], im)) return false;
        if (im.w != w || im.h != h) return fail("score: %s differs in size from %s\n", paths[k]->c_str(), q.gt.c_str());
        if (k == 0) occ.resize(N);
        if (k == 1) dist.resize(N);
        if (k >= 2) skip.resize(N, 0);
        for (size_t i = 0; i < N; ++i) {
            const unsigned v = im.rgb[3 * i];                                   // red channel
            if (k == 0) occ[i] = (uint8_t)v;
            else if (k == 1) dist[i] = (uint16_t)(v == 255 ? 65535u : v * v);
            else skip[i] |= v != 0 ? 1 : 0;
        }
    }
    DeviceArena dev;
    auto input = [&](const void* src, size_t bytes) { return bytes ? dev.stage(src, bytes) : DeviceArena::kNone; };
    const size_t d_gt = dev.stage(gt.data(), N * 8), d_est = dev.stage(est.data(), N * 8);
    const size_t d_occ = input(occ.data(), occ.size()), d_dist = input(dist.data(), dist.size() * 2), d_skip = input(skip.data(), skip.size());
    uint64_t table[ARAPFLOW_SCORE_ROWS * ARAPFLOW_SCORE_FIELDS];
    const size_t d_table = dev.take(sizeof(table));
    if (dev.alloc() != hipSuccess) return fail("score: out of device memory\n");
    const bool ok = dev.upload() == hipSuccess &&
                    ArapFlow_FlowScore(state, (unsigned)w, (unsigned)h, 1, dev.at(d_gt), dev.at(d_est), dev.at(d_occ), dev.at(d_dist),
                                       dev.at(d_skip), dev.at(d_table), nullptr) == 0 &&
                    hipDeviceSynchronize() == hipSuccess &&
                    hipMemcpy(table, dev.at(d_table), sizeof(table), hipMemcpyDeviceToHost) == hipSuccess;
    if (!ok) return fail("ArapFlow_FlowScore failed\n");
    const std::string text = format_score(table);
    return save_text(q.out, text.data(), text.size());
}

// the PSNR / SSIM table of one estimated frame, synchronously (pipeline.run_fscore): read the two frames and the planes
// the line names (red channels), the distance file back to squared distances (pipeline.dist_from_png), one
// ArapFlow_FrameScore on the state's stream, write the table as text
static bool run_fscore(Opt_State* state, const FScoreSpec& q)
{
    arapio::Image ref, est;
    if (!read_png(q.ref, ref) || !read_png(q.est, est)) return false;
    if (est.w != ref.w || est.h != ref.h) return fail("fscore: %s differs in size from %s\n", q.est.c_str(), q.ref.c_str());
    const int w = ref.w, h = ref.h;
    const size_t N = (size_t)w * h;
    std::vector<uint8_t> plane[4];
    std::vector<uint16_t> dist;
    const std::string* const paths[4] = {&q.occ, &q.dist, &q.skip, &q.obj};
    for (int k = 0; k < 4; ++k) {
        if (paths[k]->empty()) continue;
        arapio::Image im;
        if (!read_png(*paths[k], im)) return false;
        if (im.w != w || im.h != h) return fail("fscore: %s differs in size from %s\n", paths[k]->c_str(), q.ref.c_str());
        if (k == 1) dist.resize(N);
        else plane[k].resize(N);
        for (size_t i = 0; i < N; ++i) {
            const unsigned v = im.rgb[3 * i];                                   // red channel
            if (k == 1) dist[i] = (uint16_t)(v == 255 ? 65535u : v * v);
            else plane[k][i] = (uint8_t)v;
        }
    }
    DeviceArena dev;
    auto input = [&](const void* src, size_t bytes) { return bytes ? dev.stage(src, bytes) : DeviceArena::kNone; };
    const size_t d_ref = dev.stage(ref.rgb.data(), N * 3), d_est = dev.stage(est.rgb.data(), N * 3);
    const size_t d_occ = input(plane[0].data(), plane[0].size()), d_dist = input(dist.data(), dist.size() * 2);
    const size_t d_skip = input(plane[2].data(), plane[2].size()), d_obj = input(plane[3].data(), plane[3].size());
    uint64_t table[ARAPFLOW_FSCORE_ROWS * ARAPFLOW_FSCORE_FIELDS];
    const size_t d_table = dev.take(sizeof(table));
    if (dev.alloc() != hipSuccess) return fail("fscore: out of device memory\n");
    const bool ok = dev.upload() == hipSuccess &&
                    ArapFlow_FrameScore(state, (unsigned)w, (unsigned)h, 1, dev.at(d_ref), dev.at(d_est), dev.at(d_occ), dev.at(d_dist),
                                        dev.at(d_skip), dev.at(d_obj), dev.at(d_table), nullptr) == 0 &&
                    hipDeviceSynchronize() == hipSuccess &&
                    hipMemcpy(table, dev.at(d_table), sizeof(table), hipMemcpyDeviceToHost) == hipSuccess;
    if (!ok) return fail("ArapFlow_FrameScore failed\n");
    const std::string text = format_frame_score(table);
    return save_text(q.out, text.data(), text.size());
}

// the maps of an lscore / mscore line, red channels: gt, est and, when the line names one, skip, of one size
static bool read_score_maps(const char* word, const std::string& gt_path, const std::string& est_path, const std::string& skip_path,
                            int& w, int& h, std::vector<uint8_t> (&plane)[3])
{
    const std::string* const paths[3] = {&gt_path, &est_path, &skip_path};
    for (int k = 0; k < 3; ++k) {
        if (paths[k]->empty()) continue;
        arapio::Image im;
        if (!read_png(*paths[k], im)) return false;
        if (k == 0) { w = im.w; h = im.h; }
        if (im.w != w || im.h != h) return fail("%s: %s differs in size from %s\n", word, paths[k]->c_str(), gt_path.c_str());
        plane[k].resize((size_t)w * h);
        for (size_t i = 0; i < plane[k].size(); ++i) plane[k][i] = im.rgb[3 * i];
    }
    return true;
}

// the DAVIS J / F table of one estimated label map, synchronously (pipeline.run_lscore): read the maps, one
// ArapFlow_LabelScore on the state's stream, write the table as text
static bool run_lscore(Opt_State* state, const LScoreSpec& q)
{
    int w = 0, h = 0;
    std::vector<uint8_t> plane[3];
    if (!read_score_maps("lscore", q.gt, q.est, q.skip, w, h, plane)) return false;
    const uint64_t scratch = ArapFlow_MapScoreScratchBytes((unsigned)w, (unsigned)h);
    if (!scratch) return fail("lscore: maps of %d x %d: beyond the limits\n", w, h);
    DeviceArena dev;
    const size_t d_gt = dev.stage(plane[0].data(), plane[0].size()), d_est = dev.stage(plane[1].data(), plane[1].size());
    const size_t d_skip = plane[2].empty() ? DeviceArena::kNone : dev.stage(plane[2].data(), plane[2].size());
    std::vector<uint64_t> table((size_t)(q.L + 1) * ARAPFLOW_LSCORE_FIELDS);
    const size_t d_table = dev.take(table.size() * 8), d_scr = dev.take(scratch);
    if (dev.alloc() != hipSuccess) return fail("lscore: out of device memory\n");
    const bool ok = dev.upload() == hipSuccess &&
                    ArapFlow_LabelScore(state, (unsigned)w, (unsigned)h, 1, q.L, q.radius, dev.at(d_gt), dev.at(d_est), dev.at(d_skip),
                                        dev.at(d_table), dev.at(d_scr)) == 0 &&
                    hipDeviceSynchronize() == hipSuccess &&
                    hipMemcpy(table.data(), dev.at(d_table), table.size() * 8, hipMemcpyDeviceToHost) == hipSuccess;
    if (!ok) return fail("ArapFlow_LabelScore failed\n");
    const std::string text = format_label_score(table.data(), q.L);
    return save_text(q.out, text.data(), text.size());
}

// the precision / recall table of one estimated occlusion or motion-boundary map, synchronously (pipeline.run_mscore)
static bool run_mscore(Opt_State* state, const MScoreSpec& q)
{
    int w = 0, h = 0;
    std::vector<uint8_t> plane[3];
    if (!read_score_maps("mscore", q.gt, q.est, q.skip, w, h, plane)) return false;
    const unsigned m = (unsigned)q.thr.size();
    const uint64_t scratch = ArapFlow_MapScoreScratchBytes((unsigned)w, (unsigned)h);
    if (!scratch) return fail("mscore: maps of %d x %d: beyond the limits\n", w, h);
    DeviceArena dev;
    const size_t d_gt = dev.stage(plane[0].data(), plane[0].size()), d_est = dev.stage(plane[1].data(), plane[1].size());
    const size_t d_skip = plane[2].empty() ? DeviceArena::kNone : dev.stage(plane[2].data(), plane[2].size());
    std::vector<uint64_t> hist(512), match((size_t)m * 4);
    const size_t d_hist = dev.take(hist.size() * 8);
    const size_t d_match = m ? dev.take(match.size() * 8) : DeviceArena::kNone, d_scr = m ? dev.take(scratch) : DeviceArena::kNone;
    if (dev.alloc() != hipSuccess) return fail("mscore: out of device memory\n");
    const bool ok = dev.upload() == hipSuccess &&
                    ArapFlow_MapScore(state, (unsigned)w, (unsigned)h, 1, dev.at(d_gt), dev.at(d_est), dev.at(d_skip), m,
                                      m ? q.thr.data() : nullptr, q.radius, dev.at(d_hist), dev.at(d_match), dev.at(d_scr)) == 0 &&
                    hipDeviceSynchronize() == hipSuccess &&
                    hipMemcpy(hist.data(), dev.at(d_hist), hist.size() * 8, hipMemcpyDeviceToHost) == hipSuccess &&
                    (!m || hipMemcpy(match.data(), dev.at(d_match), match.size() * 8, hipMemcpyDeviceToHost) == hipSuccess);
    if (!ok) return fail("ArapFlow_MapScore failed\n");
    const std::string text = format_map_score(hist.data(), q.thr.data(), m, match.data());
    return save_text(q.out, text.data(), text.size());
}

// the in-between frames of one pair from a flow estimate, synchronously (pipeline.run_interp): read the two frames and the
// flows, one ArapFlow_InterpFrames on the state's stream, write a frame (and with src=1 a source map) per step
static bool run_interp(Opt_State* state, const InterpSpec& q)
{
    arapio::Image a, b;
    if (!read_png(q.a, a) || !read_png(q.b, b)) return false;
    if (b.w != a.w || b.h != a.h) return fail("interp: %s differs in size from %s\n", q.b.c_str(), q.a.c_str());
    const int w = a.w, h = a.h;
    const size_t N = (size_t)w * h;
    const unsigned K = (unsigned)q.steps.size();
    std::vector<float> flow[2];
    const std::string* const paths[2] = {&q.fwd, &q.bwd};
    for (int k = 0; k < 2; ++k) {
        if (paths[k]->empty()) continue;
        int fw = 0, fh = 0;
        if (!arapio::read_flo(*paths[k], flow[k], fw, fh)) return fail("Could not read %s\n", paths[k]->c_str());
        if (fw != w || fh != h) return fail("interp: %s differs in size from %s\n", paths[k]->c_str(), q.a.c_str());
    }
    const uint64_t scratch = ArapFlow_InterpScratchBytes((unsigned)w, (unsigned)h, K);
    if (!scratch) return fail("interp: %u frames of %d x %d: beyond the limits\n", K, w, h);
    float times[ARAPFLOW_INTERP_MAX_TIMES];
    for (unsigned k = 0; k < K; ++k) times[k] = (float)q.steps[k] / (float)q.n;
    DeviceArena dev;
    const size_t d_a = dev.stage(a.rgb.data(), N * 3), d_b = dev.stage(b.rgb.data(), N * 3);
    const size_t d_fwd = dev.stage(flow[0].data(), N * 8);
    const size_t d_bwd = flow[1].empty() ? DeviceArena::kNone : dev.stage(flow[1].data(), N * 8);
    const size_t d_out = dev.take((size_t)K * N * 3), d_src = q.src ? dev.take((size_t)K * N) : DeviceArena::kNone;
    const size_t d_scratch = dev.take((size_t)scratch);
    if (dev.alloc() != hipSuccess) return fail("interp: out of device memory\n");
    std::vector<uint8_t> out((size_t)K * N * 3), src(q.src ? (size_t)K * N : 0);
    const bool ok = dev.upload() == hipSuccess &&
                    ArapFlow_InterpFrames(state, (unsigned)w, (unsigned)h, dev.at(d_a), dev.at(d_b), dev.at(d_fwd), dev.at(d_bwd), K,
                                          times, dev.at(d_out), dev.at(d_src), dev.at(d_scratch)) == 0 &&
                    hipDeviceSynchronize() == hipSuccess &&
                    hipMemcpy(out.data(), dev.at(d_out), out.size(), hipMemcpyDeviceToHost) == hipSuccess &&
                    (!q.src || hipMemcpy(src.data(), dev.at(d_src), src.size(), hipMemcpyDeviceToHost) == hipSuccess);
    if (!ok) return fail("ArapFlow_InterpFrames failed\n");
    for (unsigned k = 0; k < K; ++k) {
        const std::string stem = mid_stem(q.out, q.steps[k]);
        if (!save(FileKind::rgb, stem + ".png", w, h, out.data() + k * N * 3)) return false;
        if (q.src && !save(FileKind::gray8, stem + "_src.png", w, h, src.data() + k * N)) return false;
    }
    return true;
}

// the TAP-Vid table of one estimated track file, synchronously (pipeline.run_tscore): read the two track files, one
// ArapFlow_TrackScore on the state's stream, write the table as text
static bool run_tscore(Opt_State* state, const TScoreSpec& q)
{
    arapio::Tracks gt, est;
    if (!arapio::read_trk(q.gt, gt) || !arapio::read_trk(q.est, est)) return false;
    if (gt.w != est.w || gt.h != est.h || gt.frames != est.frames || gt.points != est.points)
        return fail("tscore: %s and %s differ in W, H, F or P\n", q.gt.c_str(), q.est.c_str());
    const unsigned F = (unsigned)gt.frames, P = (unsigned)gt.points;
    if (F < 2 || F > ARAPFLOW_TSCORE_MAX_FRAMES || P > (1u << 24))
        return fail("tscore: %u frames of %u points: beyond the limits\n", F, P);
    const size_t n = (size_t)F * P;
    DeviceArena dev;
    const size_t d_gp = dev.stage(gt.pos.data(), n * 8), d_go = dev.stage(gt.occ.data(), n);
    const size_t d_ep = dev.stage(est.pos.data(), n * 8), d_eo = dev.stage(est.occ.data(), n);
    std::vector<uint64_t> table((size_t)F * ARAPFLOW_TSCORE_CLASSES * ARAPFLOW_TSCORE_FIELDS);
    const size_t d_table = dev.take(table.size() * 8);
    if (dev.alloc() != hipSuccess) return fail("tscore: out of device memory\n");
    const bool ok = dev.upload() == hipSuccess &&
                    ArapFlow_TrackScore(state, F, P, dev.at(d_gp), dev.at(d_go), dev.at(d_ep), dev.at(d_eo), q.sx, q.sy,
                                        dev.at(d_table)) == 0 &&
                    hipDeviceSynchronize() == hipSuccess &&
                    hipMemcpy(table.data(), dev.at(d_table), table.size() * 8, hipMemcpyDeviceToHost) == hipSuccess;
    if (!ok) return fail("ArapFlow_TrackScore failed\n");
    const std::string text = format_track_score(table.data(), F);
    return save_text(q.out, text.data(), text.size());
}

// the track file of chained flow estimates, synchronously (pipeline.run_chain): read the points and the flows, one
// ArapFlow_ChainFlows on the state's stream, write the track file
static bool run_chain(Opt_State* state, const ChainSpec& q)
{
    arapio::Tracks pts;
    if (!arapio::read_trk(q.points, pts)) return false;
    const int w = pts.w, h = pts.h;
    const unsigned L = (unsigned)q.flows.size(), P = (unsigned)pts.points;
    const size_t N = (size_t)w * h;
    if (P > (1u << 24) || N >= ((size_t)1 << 31)) return fail("chain: %u points on %d x %d: beyond the limits\n", P, w, h);
    std::vector<float> flows((size_t)L * N * 2), bwd(q.bwd.size() * N * 2);
    for (int b = 0; b < 2; ++b) {
        const std::vector<std::string>& paths = b ? q.bwd : q.flows;
        for (size_t j = 0; j < paths.size(); ++j) {
            std::vector<float> fl;
            int fw = 0, fh = 0;
            if (!arapio::read_flo(paths[j], fl, fw, fh)) return fail("Could not read %s\n", paths[j].c_str());
            if (fw != w || fh != h) return fail("chain: %s differs in size from %s\n", paths[j].c_str(), q.points.c_str());
            memcpy((b ? bwd : flows).data() + j * N * 2, fl.data(), N * 8);
        }
    }
    DeviceArena dev;
    const size_t d_flow = dev.stage(flows.data(), flows.size() * 4);
    const size_t d_bwd = bwd.empty() ? DeviceArena::kNone : dev.stage(bwd.data(), bwd.size() * 4);
    const size_t d_pts = dev.stage(pts.pos.data(), (size_t)P * 8);              // frame 0
    const size_t d_pos = dev.take((size_t)(L + 1) * P * 8), d_occ = dev.take((size_t)(L + 1) * P);
    if (dev.alloc() != hipSuccess) return fail("chain: out of device memory\n");
    arapio::Tracks out;
    out.w = w; out.h = h; out.frames = (int32_t)L + 1; out.points = (int32_t)P;
    out.pos.resize((size_t)(L + 1) * P * 2);
    out.occ.resize((size_t)(L + 1) * P);
    const bool ok = dev.upload() == hipSuccess &&
                    ArapFlow_ChainFlows(state, (unsigned)w, (unsigned)h, L, dev.at(d_flow), dev.at(d_bwd), P, dev.at(d_pts),
                                        dev.at(d_pos), dev.at(d_occ)) == 0 &&
                    hipDeviceSynchronize() == hipSuccess &&
                    hipMemcpy(out.pos.data(), dev.at(d_pos), out.pos.size() * 4, hipMemcpyDeviceToHost) == hipSuccess &&
                    hipMemcpy(out.occ.data(), dev.at(d_occ), out.occ.size(), hipMemcpyDeviceToHost) == hipSuccess;
    if (!ok) return fail("ArapFlow_ChainFlows failed\n");
    return arapio::write_trk(q.out, out);
}

// the point tracks of one sequence, synchronously (pipeline.run_tracks): read the points, every layer's mask and its T
// state flows, one ArapFlow_TrackPoints on the state's stream, write the track file: the points themselves as frame 0
// (occ by the frame test), then the T states
static bool run_tracks(Opt_State* state, const TrkSpec& q)
{
    arapio::Tracks trk;
    if (!arapio::read_trk(q.points, trk)) return false;
    if (trk.frames != 1) return fail("trk: %s is no points file (%d frames)\n", q.points.c_str(), trk.frames);
    const int w = trk.w, h = trk.h;
    const unsigned W = (unsigned)w, H = (unsigned)h, n = (unsigned)q.masks.size(), T = q.states, P = (unsigned)trk.points;
    const size_t N = (size_t)w * h;
    std::vector<uint8_t> masks(n * N);
    std::vector<float> flows((size_t)T * n * N * 2);           // [T][n][N][2]
    for (size_t l = 0; l < n; ++l) {
        arapio::Image msk;
        if (!read_png(q.masks[l], msk)) return false;
        if (msk.w != w || msk.h != h) return fail("trk: %s differs in size from %s\n", q.masks[l].c_str(), q.points.c_str());
        for (size_t i = 0; i < N; ++i) masks[l * N + i] = msk.rgb[3 * i];          // red channel
        for (size_t s = 0; s < T; ++s) {
            const std::string& path = q.flows[l * T + s];
            std::vector<float> fl;
            int fw = 0, fh = 0;
            if (!arapio::read_flo(path, fl, fw, fh)) return fail("Could not read %s\n", path.c_str());
            if (fw != w || fh != h) return fail("trk: %s differs in size from %s\n", path.c_str(), q.points.c_str());
            memcpy(flows.data() + (s * n + l) * N * 2, fl.data(), N * 8);
        }
    }
    const uint64_t scratch = ArapFlow_TrackPointsScratchBytes(W, H, T, P);
    if (scratch == 0) return fail("trk: %u points, %u states on %d x %d: beyond the limits\n", P, T, w, h);
    DeviceArena dev;
    const size_t d_msk = dev.stage(masks.data(), masks.size()), d_flow = dev.stage(flows.data(), flows.size() * 4);
    const size_t d_pts = dev.stage(trk.pos.data(), (size_t)P * 8);
    const size_t d_pos = dev.take((size_t)T * P * 8), d_occ = dev.take((size_t)T * P), d_scr = dev.take(scratch);
    if (dev.alloc() != hipSuccess) return fail("trk: out of device memory\n");
    arapio::Tracks out;
    out.w = w; out.h = h; out.frames = (int32_t)T + 1; out.points = (int32_t)P;
    out.pos.resize((size_t)(T + 1) * P * 2);
    out.occ.resize((size_t)(T + 1) * P);
    const bool ok = dev.upload() == hipSuccess &&
                    ArapFlow_TrackPoints(state, W, H, n, dev.at(d_msk), T, dev.at(d_flow), P, dev.at(d_pts), dev.at(d_pos),
                                         dev.at(d_occ), dev.at(d_scr)) == 0 &&
                    hipDeviceSynchronize() == hipSuccess &&
                    hipMemcpy(out.pos.data() + (size_t)P * 2, dev.at(d_pos), (size_t)T * P * 8, hipMemcpyDeviceToHost) == hipSuccess &&
                    hipMemcpy(out.occ.data() + P, dev.at(d_occ), (size_t)T * P, hipMemcpyDeviceToHost) == hipSuccess;
    if (!ok) return fail("ArapFlow_TrackPoints failed\n");
    memcpy(out.pos.data(), trk.pos.data(), (size_t)P * 8);
    for (size_t k = 0; k < P; ++k) {
        const float x = trk.pos[2 * k], y = trk.pos[2 * k + 1];
        out.occ[k] = x >= 0.f && x <= (float)(w - 1) && y >= 0.f && y <= (float)(h - 1) ? 0 : 255;     // false on NaN
    }
    return arapio::write_trk(q.out, out);
}

// the layered warp of one frame, synchronously: read the layers' files, one ArapFlow_WarpLayers on the state's stream
// (behind whatever solve is in flight there, never beside it), write the outputs asked for
static bool run_layers(Opt_State* state, const LayersSpec& q)
{
    arapio::Image rgb;
    std::vector<uint8_t> masks;
    std::vector<float> flows;
    if (!read_layer_files("layers", q.rgb, q.masks, q.flows, true, rgb, masks, flows)) return false;
    const int w = rgb.w, h = rgb.h;
    const unsigned W = (unsigned)w, H = (unsigned)h, n = (unsigned)q.masks.size();
    const size_t N = (size_t)w * h;
    if (!q.mid.steps.empty() && !run_layers_mid(state, q, rgb, masks, flows)) return false;
    if (q.occ.empty() && q.bwd.empty() && q.occ_bwd.empty() && q.rgb2.empty() && q.mask2.empty()) return true;
    DeviceArena dev;
    const size_t d_rgb = dev.stage(rgb.rgb.data(), 3 * N), d_msk = dev.stage(masks.data(), n * N);
    const size_t d_flow = dev.stage(flows.data(), n * N * 8);
    OutputTable out(dev, w, h);
    const size_t o_rgb = out.add(FileKind::rgb, q.rgb2), o_msk = out.add(FileKind::mask1, q.mask2);
    const size_t o_bwd = out.add(FileKind::flo, q.bwd), o_obwd = out.add(FileKind::gray8, q.occ_bwd);
    const size_t o_occ = out.add(FileKind::gray8, q.occ);
    const size_t d_scr = dev.take(ArapFlow_WarpLayersScratchBytes(W, H, n));
    if (dev.alloc() != hipSuccess) return fail("layers: out of device memory\n");
    const bool ok = dev.upload() == hipSuccess &&
                    ArapFlow_WarpLayers(state, W, H, n, dev.at(d_rgb), dev.at(d_msk), dev.at(d_flow), out.dev(o_rgb),
                                        out.dev(o_msk), out.dev(o_bwd), out.dev(o_obwd), out.dev(o_occ), dev.at(d_scr)) == 0 &&
                    hipDeviceSynchronize() == hipSuccess && out.download() == hipSuccess;
    return ok ? out.write() : fail("ArapFlow_WarpLayers failed\n");
}

// the mid= / mm= / mid_out= tokens of a bg line (pipeline.run_background_seq): frame 1, the snapshots mid= names and
// frame 2 are the frames of one ArapFlow_BackgroundSeq, which writes every in-between frame, every link's flow and, with
// occ= on the line, every link's occlusion.  The composites of frame 1 and frame 2 stay with out=.
static bool run_background_seq(Opt_State* state, const BgSpec& q, const arapio::Image& bg, const std::vector<uint8_t>& mask_red,
                               const std::vector<uint8_t>& cover2, int w, int h)
{
    const size_t N = (size_t)w * h, n = q.mid.steps.size(), m = n + 2;
    const bool with_occ = !q.occ.empty();
    std::vector<arapio::Image> rgbs(n);
    std::vector<std::vector<uint8_t>> covers(n), occs(with_occ ? n + 1 : 0);
    std::vector<std::vector<float>> flows(n + 1);
    auto missing = [](const std::string& path) { return fail("bg: snapshot %s is missing\n", path.c_str()); };
    auto differs = [&](const std::string& path) { return fail("bg: %s differs in size from %s\n", path.c_str(), q.mask1.c_str()); };
    auto flo = [&](const std::string& path, std::vector<float>& fl) {
        int fw = 0, fh = 0;
        if (!arapio::read_flo(path, fl, fw, fh)) return missing(path);
        return (fw == w && fh == h) || differs(path);
    };
    auto png = [&](const std::string& path, arapio::Image& im) {
        std::string err;
        if (!arapio::read_png_rgb(path, im, err)) return missing(path);
        return (im.w == w && im.h == h) || differs(path);
    };
    if (!flo(mid_stem(q.mid.prefix, q.mid.steps[0]) + ".flo", flows[0])) return false;
    for (size_t k = 0; k <= n; ++k) {
        const std::string stem = mid_stem(q.mid.prefix, k ? q.mid.steps[k - 1] : 0);
        arapio::Image im;
        if (with_occ) {
            if (!png(stem + "_occ.png", im)) return false;
            occs[k] = red_channel(im);
        }
        if (k == 0) continue;
        if (!png(stem + ".png", rgbs[k - 1]) || !png(stem + "_mask.png", im) || !flo(stem + "_step.flo", flows[k])) return false;
        covers[k - 1] = red_channel(im);
        for (uint8_t& c : covers[k - 1]) c = c ? 255 : 0;
    }
    DeviceArena dev;
    const size_t d_bg = dev.stage(bg.rgb.data(), bg.rgb.size()), d_m1 = dev.stage(mask_red.data(), N);
    std::vector<size_t> d_cover(m, DeviceArena::kNone), d_rgb(m, DeviceArena::kNone), d_flow(m - 1), d_occ(m - 1, DeviceArena::kNone);
    d_cover[m - 1] = dev.stage(cover2.data(), N);
    for (size_t k = 0; k < n; ++k) {
        d_cover[k + 1] = dev.stage(covers[k].data(), N);
        d_rgb[k + 1] = dev.stage(rgbs[k].rgb.data(), 3 * N);
    }
    for (size_t k = 0; k <= n; ++k) {
        d_flow[k] = dev.stage(flows[k].data(), 8 * N);
        if (with_occ) d_occ[k] = dev.stage(occs[k].data(), N);
    }
    OutputTable out(dev, w, h);            // in the order of pipeline.bg_outputs
    std::vector<size_t> o_rgb(m, DeviceArena::kNone), o_flow(m - 1), o_occ(m - 1, DeviceArena::kNone);
    for (size_t k = 1; k <= n; ++k) o_rgb[k] = out.add(FileKind::rgb, mid_stem(q.mid_out, q.mid.steps[k - 1]) + ".png");
    for (size_t k = 0; k <= n; ++k) o_flow[k] = out.add(FileKind::flo, mid_stem(q.mid_out, k ? q.mid.steps[k - 1] : 0) + "_step.flo");
    for (size_t k = 0; with_occ && k <= n; ++k)
        o_occ[k] = out.add(FileKind::gray8, mid_stem(q.mid_out, k ? q.mid.steps[k - 1] : 0) + "_occ.png");
    if (dev.alloc() != hipSuccess) return fail("bg: out of device memory\n");
    std::vector<float> maps(q.m, q.m + 6);
    maps.insert(maps.end(), q.mm.begin(), q.mm.end());
    maps.insert(maps.end(), q.m + 6, q.m + 12);
    std::vector<const void*> p_cover(m), p_rgb(m), p_flow(m - 1), p_occ(m - 1);
    std::vector<void*> p_orgb(m), p_oflow(m - 1), p_oocc(m - 1);
    auto row = [&](size_t r) { return r == DeviceArena::kNone ? nullptr : out.dev(r); };
    for (size_t f = 0; f < m; ++f) {
        p_cover[f] = dev.at(d_cover[f]); p_rgb[f] = dev.at(d_rgb[f]); p_orgb[f] = row(o_rgb[f]);
        if (f + 1 < m) { p_flow[f] = dev.at(d_flow[f]); p_occ[f] = dev.at(d_occ[f]); p_oflow[f] = row(o_flow[f]); p_oocc[f] = row(o_occ[f]); }
    }
    const bool ok = dev.upload() == hipSuccess &&
                    ArapFlow_BackgroundSeq(state, (unsigned)w, (unsigned)h, dev.at(d_bg), (unsigned)bg.w, (unsigned)bg.h, (unsigned)m,
                                           maps.data(), dev.at(d_m1), p_cover.data(), p_rgb.data(), p_flow.data(), p_occ.data(),
                                           p_orgb.data(), p_oflow.data(), p_oocc.data()) == 0 &&
                    hipDeviceSynchronize() == hipSuccess && out.download() == hipSuccess;
    return ok ? out.write() : fail("ArapFlow_BackgroundSeq failed\n");
}

// the moving-background pass of one pair, synchronously (pipeline.run_background): read the line's files, one
// ArapFlow_Background on the state's stream, write the outputs asked for; then, with mid=, the sequence pass
static bool run_background(Opt_State* state, const BgSpec& q)
{
    arapio::Image bg, rgb1, rgb2, m1, m2, occ, occ_bwd;
    if (!read_png(q.bg, bg) || !read_png(q.rgb1, rgb1) || !read_png(q.mask1, m1) || !read_png(q.rgb2, rgb2) ||
        !read_png(q.mask2, m2))
        return false;
    if (!q.occ.empty() && !read_png(q.occ, occ)) return false;
    if (!q.occ_bwd.empty() && !read_png(q.occ_bwd, occ_bwd)) return false;
    const int w = rgb1.w, h = rgb1.h;
    std::vector<float> flow, bwd;
    int fw = 0, fh = 0, bw = w, bh = h;
    if (!arapio::read_flo(q.flow, flow, fw, fh)) return false;
    if (!q.bwd.empty() && !arapio::read_flo(q.bwd, bwd, bw, bh)) return false;
    auto same = [&](const arapio::Image& im) { return im.w == w && im.h == h; };
    if (!same(m1) || !same(rgb2) || !same(m2) || fw != w || fh != h || bw != w || bh != h ||
        (!q.occ.empty() && !same(occ)) || (!q.occ_bwd.empty() && !same(occ_bwd)))
        return fail("bg: image, mask and flow sizes differ: %s\n", q.rgb1.c_str());
    const size_t N = (size_t)w * h;
    // the red channels of the masks (cover2 as it is read: non-zero = object) and of the occlusion maps the line names
    const std::vector<uint8_t> mask_red = red_channel(m1), occ_red = red_channel(occ), occ_bwd_red = red_channel(occ_bwd);
    std::vector<uint8_t> cover2 = red_channel(m2);
    for (uint8_t& c : cover2) c = c ? 255 : 0;
    DeviceArena dev;
    auto input = [&](const void* src, size_t bytes) { return bytes ? dev.stage(src, bytes) : DeviceArena::kNone; };
    const size_t d_bg = dev.stage(bg.rgb.data(), bg.rgb.size()), d_rgb1 = dev.stage(rgb1.rgb.data(), 3 * N);
    const size_t d_rgb2 = dev.stage(rgb2.rgb.data(), 3 * N), d_m1 = dev.stage(mask_red.data(), N);
    const size_t d_cover2 = dev.stage(cover2.data(), N), d_flow = dev.stage(flow.data(), 8 * N);
    const size_t d_occ = input(occ_red.data(), occ_red.size()), d_bwd = input(bwd.data(), 4 * bwd.size());
    const size_t d_occ_bwd = input(occ_bwd_red.data(), occ_bwd_red.size());
    OutputTable out(dev, w, h);
    const size_t o_rgb1 = out.add(FileKind::rgb, q.out_rgb1), o_rgb2 = out.add(FileKind::rgb, q.out_rgb2);
    const size_t o_flow = out.add(FileKind::flo, q.out_flow), o_bwd = out.add(FileKind::flo, q.out_bwd);
    const size_t o_occ = out.add(FileKind::gray8, q.out_occ), o_occ_bwd = out.add(FileKind::gray8, q.out_occ_bwd);
    const bool pair = !(q.out_rgb1 + q.out_rgb2 + q.out_flow + q.out_occ + q.out_bwd + q.out_occ_bwd).empty();
    if (dev.alloc() != hipSuccess) return fail("bg: out of device memory\n");
    const bool ok = !pair || (dev.upload() == hipSuccess &&
                    ArapFlow_Background(state, (unsigned)w, (unsigned)h, dev.at(d_bg), (unsigned)bg.w, (unsigned)bg.h, q.m, q.m + 6,
                                        dev.at(d_rgb1), dev.at(d_m1), dev.at(d_rgb2), dev.at(d_cover2), dev.at(d_flow),
                                        dev.at(d_occ), dev.at(d_bwd), dev.at(d_occ_bwd), out.dev(o_rgb1), out.dev(o_rgb2),
                                        out.dev(o_flow), out.dev(o_occ), out.dev(o_bwd), out.dev(o_occ_bwd)) == 0 &&
                    hipDeviceSynchronize() == hipSuccess && out.download() == hipSuccess);
    if (!ok) return fail("ArapFlow_Background failed\n");
    if (!out.write()) return false;
    return q.mid_out.empty() || run_background_seq(state, q, bg, mask_red, cover2, w, h);
}

// ---- where the lines come from: a finished list, or stdin as it arrives (--serve) ------------------------------------
class FrameSource {
  public:
    explicit FrameSource(const std::vector<Item>& fixed) : lines_(fixed.begin(), fixed.end()), eof_(true) {}
    FrameSource() : eof_(false)                                         // --serve: a thread reads stdin
    {
        reader_ = std::thread([this]() {
            for (std::string line; std::getline(std::cin, line);) {
                Item q;
                if (parse_item(line, q) != Parsed::Good) continue;
                { std::lock_guard<std::mutex> g(m_); lines_.push_back(std::move(q)); }
                cv_.notify_all();
            }
            { std::lock_guard<std::mutex> g(m_); eof_ = true; }
            cv_.notify_all();
        });
    }
    ~FrameSource() { if (reader_.joinable()) reader_.join(); }

    // Next decoded frame in line order.  wait_ms < 0: block until one is there or the source is exhausted;
    // otherwise give up after wait_ms.  Returns 1 (frame in *out), 0 (nothing within the time), -1 (exhausted).
    int next(std::unique_ptr<Frame>* out, int wait_ms)
    {
        using clock = std::chrono::steady_clock;
        const auto deadline = clock::now() + std::chrono::milliseconds(wait_ms < 0 ? 0 : wait_ms);
        for (;;) {
            start_loads();
            if (!loading_.empty()) {
                std::future<Frame>& f = loading_.front();
                if (wait_ms < 0) f.wait();
                else if (f.wait_until(deadline) == std::future_status::timeout) return 0;
                out->reset(new Frame(f.get()));
                loading_.pop_front();
                return 1;
            }
            std::unique_lock<std::mutex> g(m_);
            if (!lines_.empty()) continue;
            if (eof_) return -1;
            if (wait_ms < 0) cv_.wait(g, [this]() { return !lines_.empty() || eof_; });
            else if (!cv_.wait_until(g, deadline, [this]() { return !lines_.empty() || eof_; })) return 0;
        }
    }

  private:
    void start_loads()                                                  // decode ahead: loadData on worker threads
    {
        std::lock_guard<std::mutex> g(m_);
        while (!lines_.empty() && loading_.size() < kAhead) {
            auto q = std::make_shared<Item>(std::move(lines_.front()));
            lines_.pop_front();
            // a layers / bg / tex / trk / blur / light / seg / score / tscore / chain / fscore / interp / lscore / mscore line is read when its turn comes: in a list its inputs may not exist yet
            const bool solve = q->kind == Item::Kind::Solve;
            loading_.push_back(std::async(solve ? std::launch::async : std::launch::deferred, [q, solve]() {
                Frame f;
                f.item = std::move(*q);
                f.ok = !solve || load_frame(f);
                return f;
            }));
        }
    }
    static constexpr size_t kAhead = 48;
    std::mutex m_;
    std::condition_variable cv_;
    std::deque<Item> lines_;
    std::deque<std::future<Frame>> loading_;
    bool eof_;
    std::thread reader_;
};

// ---- results: read back from the solver's pinned buffers, encoded and written by worker threads ---------------------
struct OutFile { FileKind kind; std::string path; std::vector<uint8_t> data; bool text = false; };   // text: written as it is
struct Result { std::string flow; std::vector<OutFile> files; };       // a line's flow path and its files in writing order

class Writer {
  public:
    explicit Writer(bool report) : report_(report) {}
    void submit(std::shared_ptr<Result> r, int w, int h)
    {
        while (tasks_.size() >= 24) { tasks_.front().get(); tasks_.pop_front(); }
        tasks_.push_back(std::async(std::launch::async, [this, r, w, h]() {
            for (const OutFile& f : r->files) {
                if (f.text) save_text(f.path, f.data.data(), f.data.size());
                else save(f.kind, f.path, w, h, f.data.data());
            }
            say(report_ ? "Done " + r->flow : std::string("Saved"));    // --serve: one line per finished solve
        }));
    }
    void finish() { for (auto& t : tasks_) t.get(); tasks_.clear(); }
    void say(const std::string& line)
    {
        std::lock_guard<std::mutex> g(print_);
        printf("%s\n", line.c_str());
        fflush(stdout);
    }

  private:
    const bool report_;
    std::mutex print_;
    std::deque<std::future<void>> tasks_;  // (declared last: destroyed, that is waited for, first)
};

// ---- the schedule: two solver objects of one frame size alternate (see the header comment) --------------------------
static const unsigned numIter = 19, nonLinearIter = 8, linearIter = 400;    // main.cpp:215-221

struct Lane {
    ArapFlow_Solver* solver = nullptr;
    std::vector<SolvePaths> batch;         // frames set into the slots, in slot order
    bool inflight = false;
    bool diag = false;                     // fold diagnostics in effect in `solver`
};

struct Lanes {
    Writer& writer;
    const bool serve;
    Lane lane[2];
    int w = 0, h = 0;                      // the frame size the solvers are built for
    // Frames per solve call: the library gives every solve a group of the resident launch's workgroups sized by its
    // active tiles and a launch costs the same however full it is, so frames join a batch while they still fit ONE
    // launch (ArapFlow_SolverLaunchesFor); kMinFill frames per call when the resident kernel does not apply.
    // Both bounds follow the frame size: a solver object pins 24 bytes x vertices x maxBatch of host staging (two objects:
    // 0.6 GB at 854x480 x 32 -- but 3.2 GB at 1920x1080 x 32, where a launch holds four segment solves anyway).
    unsigned maxBatch = 32;
    static constexpr unsigned kMinFill = 8;

    // solvers for another frame size; everything of the old size is finished (CombinedSolver.h:149-160)
    bool rebuild(Opt_State* state, int nw, int nh)
    {
        if (lane[0].solver) {
            printf("Warning: Input image has different size to one in the prebuilt plan.\n"
                   "To avoid re-building the plan and to save time, put images of the same size in the same list.\n"
                   "Starting to re-build plan...\n");            // CombinedSolver.h:151-153
            release();
        }
        const double rel = (double)nw * nh / (854.0 * 480.0);
        const int m = (int)(32.0 / (rel < 1.0 ? 1.0 : rel));
        maxBatch = (unsigned)(m < 8 ? 8 : m);
        for (Lane& L : lane) { L.solver = ArapFlow_SolverCreate(state, (unsigned)nw, (unsigned)nh, maxBatch); L.diag = false; }
        w = nw; h = nh;
        return lane[0].solver && lane[1].solver;
    }
    void release()
    {
        for (Lane& L : lane)
            if (L.solver) { ArapFlow_SolverFree(L.solver); L.solver = nullptr; }
    }
    // does the frame just set into slot batch.size() of L still belong to its batch?
    bool fits(const Lane& L) const
    {
        const unsigned b = (unsigned)L.batch.size();
        if (b == 0) return true;
        const int launches = ArapFlow_SolverLaunchesFor(L.solver, b + 1);
        return !(launches > 1 || (launches == 0 && b >= kMinFill));
    }
    // start L's batch, then finish both lanes
    bool flush(Lane& L, Lane& other) { return launch(L) && drain(other) && drain(L); }

    bool drain(Lane& L)                    // wait for the lane's solve, hand its results to the writer threads
    {
        if (!L.inflight) return true;
        if (ArapFlow_SolverWait(L.solver) != 0) return fail("ARAP solve failed\n");
        const size_t n = (size_t)w * h;
        for (size_t b = 0; b < L.batch.size(); ++b) {                    // copyResultToCPU
            const SolvePaths& q = L.batch[b];
            auto r = std::make_shared<Result>(Result{q.flow, {}});
            auto keep = [&](FileKind kind, const std::string& path, const void* src) {
                const uint8_t* p = (const uint8_t*)src;
                if (p && !path.empty()) r->files.push_back(OutFile{kind, path, std::vector<uint8_t>(p, p + bytes_per_pixel(kind) * n)});
            };
            const float* flow; const uint8_t *wrgb, *wmsk;
            if (ArapFlow_SolverHostResults(L.solver, (unsigned)b, &flow, &wrgb, &wmsk) != 0 || !wrgb)
                return fail("ARAP results unavailable\n");
            keep(FileKind::rgb, q.warped_rgb, wrgb);
            keep(FileKind::mask1, q.warped_mask, wmsk);
            keep(FileKind::flo, q.flow, flow);
            if (q.outputs()) {
                const float* bwd; const uint8_t *obwd, *occ;
                if (ArapFlow_SolverHostExtraResults(L.solver, (unsigned)b, &bwd, &obwd, &occ) != 0)
                    return fail("ARAP extra results unavailable\n");
                keep(FileKind::flo, q.bwd, bwd);
                keep(FileKind::gray8, q.occ_bwd, bwd ? obwd : nullptr);
                keep(FileKind::gray8, q.occ, occ);
            }
            if (q.wants_diag()) {
                const ArapFlow_MeshStats* stats; const uint8_t* fold;
                if (ArapFlow_SolverHostDiag(L.solver, (unsigned)b, &stats, &fold) != 0)
                    return fail("ARAP diagnostics unavailable\n");
                if (!q.diag.empty()) {
                    const std::string text = format_diag(*stats);
                    r->files.push_back(OutFile{FileKind::gray8, q.diag, std::vector<uint8_t>(text.begin(), text.end()), true});
                }
                keep(FileKind::gray8, q.fold, fold);
            }
            for (unsigned k = 0; k < q.mid.steps.size(); ++k) {
                const float *mf, *ms; const uint8_t *mr, *mm;
                if (ArapFlow_SolverHostSnapshot(L.solver, (unsigned)b, k, &mf, &mr, &mm, &ms) != 0 || !mr)
                    return fail("ARAP snapshots unavailable\n");
                const std::string stem = mid_stem(q.mid.prefix, q.mid.steps[k]);
                keep(FileKind::flo, stem + ".flo", mf);
                keep(FileKind::rgb, stem + ".png", mr);
                keep(FileKind::mask1, stem + "_mask.png", mm);
                keep(FileKind::flo, stem + "_step.flo", ms);
            }
            writer.submit(r, w, h);
        }
        L.batch.clear();
        L.inflight = false;
        return true;
    }

    bool launch(Lane& L)
    {
        if (L.batch.empty()) return true;
        int outputs = 0;                     // what any line of the batch asks for (off for plain lines: no extra kernel)
        for (const SolvePaths& q : L.batch) outputs |= q.outputs();
        if (ArapFlow_SolverSetOutputs(L.solver, outputs) != 0) return fail("ARAP outputs could not be set\n");
        // snapshots are on iff a line of the batch asks (plain batches run nothing new); its mid= lines name the same steps
        const std::vector<unsigned>* steps = nullptr;
        for (const SolvePaths& q : L.batch) {
            if (q.mid.steps.empty()) continue;
            if (steps && *steps != q.mid.steps) return fail("mid= steps differ from those of the batch: %s\n", q.flow.c_str());
            steps = &q.mid.steps;
        }
        if (ArapFlow_SolverSetSnapshots(L.solver, steps ? steps->data() : nullptr, steps ? (unsigned)steps->size() : 0) != 0)
            return fail("ARAP snapshots could not be set\n");
        bool diag = false;                   // likewise: set only to turn the diagnostics on, or off again
        for (const SolvePaths& q : L.batch) diag = diag || q.wants_diag();
        if (diag != L.diag) {
            if (ArapFlow_SolverSetDiag(L.solver, diag) != 0) return fail("ARAP diagnostics could not be set\n");
            L.diag = diag;
        }
        if (ArapFlow_SolverSolveAsync(L.solver, (unsigned)L.batch.size(), numIter, nonLinearIter, linearIter, 1, 1) != 0)
            return fail("ARAP solve could not be started\n");
        if (serve) { printf("Batch %zu\n", L.batch.size()); fflush(stdout); }    // (para_gen.py keeps statistics)
        L.inflight = true;
        return true;
    }
};

int main(int argc, const char* argv[])
{
    std::unique_ptr<FrameSource> source;
    bool serve = false;
    if (argc == 7) {                                                     // one frame on the command line
        Item one;
        one.solve = SolvePaths{argv[1], argv[2], argv[3], argv[4], argv[5], argv[6]};
        source.reset(new FrameSource(std::vector<Item>{one}));
    } else if (argc == 2 && strcmp(argv[1], "--serve") == 0) {
        serve = true;
    } else if (argc == 2) {                                              // list file
        std::ifstream list(argv[1]);
        std::vector<Item> lines;
        for (std::string line; std::getline(list, line);) {
            Item q;
            const Parsed p = parse_item(line, q);
            if (p == Parsed::Bad) return 1;
            if (p == Parsed::Good) lines.push_back(q);
        }
        if (lines.empty()) { printf("No file to be processed"); return 1; }
        source.reset(new FrameSource(lines));
    } else {
        printf("Invalid Input!\n");
        fputs(kUsage, stdout);
        return 1;
    }
    Opt_InitializationParameters ip = {0, 0, 0, 0};
    Opt_State* state = Opt_NewState(ip);
    if (!state) return 1;
    ArapFlow_UseOwnStream(state);            // uploads / downloads overlap the solves (see the header comment)
    const char* planPath = getenv("ARAP_PLAN");                          // main.cpp:206-213
    if (planPath) {
        printf("Optimization plan at %s\n", planPath);
        std::ifstream f(planPath);
        if (!f.good()) {
            printf(" Not found! Please run export ARAP_PLAN=/path/to/plan.t or copy the file to the running folder "
                   "with name arap_plan.t");
            return 1;
        }
        Opt_Problem* pr = Opt_ProblemDefine(state, planPath, "gaussNewtonGPU");
        if (!pr) return 1;
        Opt_ProblemDelete(state, pr);
    }
    if (serve) {
        printf("Ready\n");                   // HIP is up: the parent may start its clock / feed lines
        fflush(stdout);
        source.reset(new FrameSource());
    }
    // --serve: how long a partly filled batch waits for another line when the GPU is idle
    int linger_ms = 30;
    if (const char* e = getenv("ARAP_DEFORM_LINGER_MS")) linger_ms = atoi(e);

    Writer writer(serve);
    Lanes lanes{writer, serve};
    int cur = 0;
    std::unique_ptr<Frame> carry;           // decoded frame that did not fit the batch it was offered to
    bool exhausted = false;
    int rc = 0;
    while (rc == 0) {
        Lane& L = lanes.lane[cur];
        Lane& other = lanes.lane[cur ^ 1];
        // ---- next frame: the carried one, or whatever the source has.  An empty batch with nothing in flight blocks;
        //      a partly filled one waits `linger_ms` (while the other lane is solving, waiting costs nothing: drain it
        //      first, new lines may arrive meanwhile)
        std::unique_ptr<Frame> fr;
        bool full = false;
        if (carry) fr = std::move(carry);
        else if (!exhausted) {
            int got;
            if (L.batch.empty() && !other.inflight) got = source->next(&fr, -1);
            else {
                got = source->next(&fr, 0);
                if (got == 0 && other.inflight) {
                    if (!lanes.drain(other)) { rc = 1; break; }
                    got = source->next(&fr, 0);
                }
                if (got == 0) got = source->next(&fr, L.batch.empty() ? -1 : linger_ms);
            }
            if (got < 0) exhausted = true;
        }
        if (fr && fr->item.kind != Item::Kind::Solve) {
            // A list: every earlier line is solved and written first (this line's inputs may be their outputs).  --serve:
            // the sender names only files that exist, so nothing is flushed; the call queues behind the solve in flight.
            if (!serve) {
                if (!lanes.flush(L, other)) { rc = 1; break; }
                writer.finish();
            }
            const Item::Kind kind = fr->item.kind;
            if (!(kind == Item::Kind::Bg    ? run_background(state, fr->item.bg)
                  : kind == Item::Kind::Tex ? run_texture(state, fr->item.tex)
                  : kind == Item::Kind::Trk ? run_tracks(state, fr->item.trk)
                  : kind == Item::Kind::Blur ? run_blur(state, fr->item.blur)
                  : kind == Item::Kind::Light ? run_light(state, fr->item.light)
                  : kind == Item::Kind::Seg ? run_seg(state, fr->item.seg)
                  : kind == Item::Kind::Score ? run_score(state, fr->item.score)
                  : kind == Item::Kind::TScore ? run_tscore(state, fr->item.tscore)
                  : kind == Item::Kind::Chain ? run_chain(state, fr->item.chain)
                  : kind == Item::Kind::FScore ? run_fscore(state, fr->item.fscore)
                  : kind == Item::Kind::Interp ? run_interp(state, fr->item.interp)
                  : kind == Item::Kind::LScore ? run_lscore(state, fr->item.lscore)
                  : kind == Item::Kind::MScore ? run_mscore(state, fr->item.mscore)
                                            : run_layers(state, fr->item.layers))) { rc = 1; break; }
            writer.say(serve ? "Done " + done_path(fr->item) : std::string("Saved"));
            continue;
        }
        if (fr) {
            if (!fr->ok) { rc = 1; break; }
            const int w = fr->rgb.w, h = fr->rgb.h;
            // another frame size: finish everything of the old size, then re-build
            if ((w != lanes.w || h != lanes.h) && !(lanes.flush(L, other) && lanes.rebuild(state, w, h))) { rc = 1; break; }
            if (ArapFlow_SolverSetFrame(L.solver, (unsigned)L.batch.size(), fr->rgb.rgb.data(), fr->mask_red.data(),
                                        fr->constraints.data(), (unsigned)(fr->constraints.size() / 4), 0) != 0) { rc = 1; break; }
            if (lanes.fits(L)) {
                L.batch.push_back(fr->item.solve);
                full = L.batch.size() >= lanes.maxBatch;
            } else {
                carry = std::move(fr);                                   // opens the next batch (set again there)
                full = true;
            }
            if (!full) continue;
        }
        // ---- nothing more joins this batch: start it, then turn to the other lane (its results, then its next batch)
        if (!L.batch.empty()) {
            if (!lanes.launch(L) || !lanes.drain(other)) { rc = 1; break; }
            cur ^= 1;
        } else if (exhausted && !carry) {
            break;
        }
    }
    if (rc == 0 && (!lanes.drain(lanes.lane[cur ^ 1]) || !lanes.drain(lanes.lane[cur]))) rc = 1;
    writer.finish();
    lanes.release();
    ArapFlow_FreeState(state);
    fflush(stdout);
    if (rc != 0) _exit(rc);                  // (--serve: the stdin reader may still be blocked in getline)
    return rc;
}
