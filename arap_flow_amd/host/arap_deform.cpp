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
// must name the same steps.  Other trailing tokens are ignored, as before.
// A line whose first word is `layers` is no solve but the layered warp of one frame (DESIGN.md "Layered warp"):
//   layers RGB n MASK_1 FLO_1 ... MASK_n FLO_n [occ=P] [bwd=P] [occ_bwd=P] [rgb2=P] [mask2=P] [mid=I1,I2,..:PREFIX]
// (at least one output).  Its mid= token (DESIGN.md "Layered in-between frames") reads every layer's snapshot flows
// STEM_l_sII.flo, STEM_l = FLO_l without `.flo`, and writes per snapshot the composite PREFIX_sII.flo, PREFIX_sII.png,
// PREFIX_sII_mask.png, PREFIX_sII_step.flo and, with occ= on the line, the link occlusions PREFIX_s00_occ.png (frame 1
// -> first snapshot) and PREFIX_sII_occ.png (snapshot -> next state).
// A line whose first word is `bg` is the moving-background pass of one pair (DESIGN.md "Moving background"):
//   bg BG.png RGB1.png MASK1.png RGB2.png MASK2.png FLOW.flo m=<12 numbers, M1 then M2, comma separated>
//      [occ=IN] [bwd=IN] [occ_bwd=IN] out=RGB1_OUT.png,RGB2_OUT.png,FLOW_OUT.flo [occ_out=P] [bwd_out=P] [occ_bwd_out=P]
// (MASK1: red 0 = object; MASK2: a warped mask, non-zero = object; a place of out= may be empty; at least one output).
// It answers "Done <first output: the places of out=, then occ_out, bwd_out, occ_bwd_out>".
// Either runs on the solver's own stream between batches; in a list every earlier line is finished and written first (its
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
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fstream>
#include <future>
#include <iostream>
#include <memory>
#include <mutex>
#include <sstream>
#include <string>
#include <thread>
#include <unistd.h>
#include <vector>

#include <hip/hip_runtime_api.h>

extern "C" {
#include "../../include/arap_opt.h"
}
#include "flo_io.h"
#include "png_io.h"

// one solve = one list-file line (ARAP/deformation/src/main.cpp:4-11,183-191)
struct SolvePaths {
    std::string rgb, mask, constraints, flow, warped_rgb, warped_mask;
    std::string bwd, occ, occ_bwd;         // optional outputs (empty: not wanted)
    std::vector<unsigned> mid_steps;       // mid= token: snapshot steps (empty: not wanted) and the files' path prefix
    std::string mid_prefix;
    int outputs() const
    {
        return (bwd.empty() && occ_bwd.empty() ? 0 : ARAPFLOW_OUT_BACKWARD) | (occ.empty() ? 0 : ARAPFLOW_OUT_OCCLUSION);
    }
};

// one `layers` line
struct LayersSpec {
    std::string rgb;
    std::vector<std::string> masks, flows;
    std::string occ, bwd, occ_bwd, rgb2, mask2;
    std::vector<unsigned> mid_steps;       // mid= token (empty: not wanted) and the composite files' path prefix
    std::string mid_prefix;
    std::string first_out;                 // the first output token's path: what --serve reports
};

// one `bg` line (pipeline.BgLine)
struct BgSpec {
    std::string bg, rgb1, mask1, rgb2, mask2, flow;
    float m[12];                           // M1, M2
    std::string occ, bwd, occ_bwd;         // optional object-side inputs
    std::string out_rgb1, out_rgb2, out_flow, out_occ, out_bwd, out_occ_bwd;      // outputs (empty: not wanted)
    std::string first_out() const
    {
        for (const std::string* q : {&out_rgb1, &out_rgb2, &out_flow, &out_occ, &out_bwd, &out_occ_bwd})
            if (!q->empty()) return *q;
        return std::string();
    }
};

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

// constraint file (main.cpp:26-50): a count n, then n rows of four integers x1 y1 x2 y2
static bool read_constraint_file(const std::string& path, std::vector<int32_t>& rows)
{
    FILE* f = fopen(path.c_str(), "r");
    if (!f) {
        std::cout << "Could not open marker file " << path << std::endl;
        return false;
    }
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

struct Frame {
    SolvePaths paths;
    arapio::Image rgb;
    std::vector<uint8_t> mask_red;
    std::vector<int32_t> constraints;      // x1 y1 x2 y2 rows, file order then border pins
};

// loadData of the reference (main.cpp:116-138): constraints file, PNGs, then a pin-to-self constraint for every border pixel
static bool load_frame(const SolvePaths& paths, Frame& f)
{
    f.paths = paths;
    if (!read_constraint_file(paths.constraints, f.constraints)) return false;
    std::string err;
    if (!arapio::read_png_rgb(paths.rgb, f.rgb, err)) { printf("%s\n", err.c_str()); return false; }
    arapio::Image msk;
    if (!arapio::read_png_rgb(paths.mask, msk, err)) { printf("%s\n", err.c_str()); return false; }
    if (msk.w != f.rgb.w || msk.h != f.rgb.h) {
        printf("Mask %s and image %s differ in size\n", paths.mask.c_str(), paths.rgb.c_str());
        return false;
    }
    const int width = f.rgb.w, height = f.rgb.h;
    f.mask_red.resize((size_t)width * height);
    for (size_t i = 0; i < f.mask_red.size(); ++i) f.mask_red[i] = msk.rgb[3 * i];      // red channel
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++)
            if (y == 0 || x == 0 || y == (height - 1) || x == (width - 1)) {
                f.constraints.push_back(x); f.constraints.push_back(y);
                f.constraints.push_back(x); f.constraints.push_back(y);
            }
    return true;
}

// the value of a mid= token: I1,I2,..:PREFIX with 1 <= I1 < I2 < .., at most ARAPFLOW_MAX_SNAPSHOTS indices
static bool parse_mid(const std::string& v, std::vector<unsigned>& steps, std::string& prefix)
{
    const size_t colon = v.find(':');
    if (colon == std::string::npos || colon == 0 || colon + 1 >= v.size()) return false;
    steps.clear();
    size_t a = 0;
    while (a < colon) {
        size_t b = v.find(',', a);
        if (b == std::string::npos || b > colon) b = colon;
        if (b == a || b - a > 6) return false;
        unsigned x = 0;
        for (size_t k = a; k < b; ++k) {
            if (v[k] < '0' || v[k] > '9') return false;
            x = 10 * x + (unsigned)(v[k] - '0');
        }
        if (x < 1 || (!steps.empty() && x <= steps.back())) return false;
        steps.push_back(x);
        if (b == colon && v[b - 1] == ',') return false;
        a = b + 1;
    }
    if (v[colon - 1] == ',' || steps.empty() || steps.size() > ARAPFLOW_MAX_SNAPSHOTS) return false;
    prefix = v.substr(colon + 1);
    return true;
}

// -1: not a solve line (too few paths), 0: a solve line with a malformed mid= token, 1: good
static int parse_line(const std::string& line, SolvePaths& q)
{
    std::istringstream tok(line);
    if (!(tok >> q.rgb >> q.mask >> q.constraints >> q.flow >> q.warped_rgb >> q.warped_mask)) return -1;
    for (std::string t; tok >> t;) {
        if (t.compare(0, 4, "bwd=") == 0) q.bwd = t.substr(4);
        else if (t.compare(0, 4, "occ=") == 0) q.occ = t.substr(4);
        else if (t.compare(0, 8, "occ_bwd=") == 0) q.occ_bwd = t.substr(8);
        else if (t.compare(0, 4, "mid=") == 0 && t.size() > 4 && !parse_mid(t.substr(4), q.mid_steps, q.mid_prefix)) return 0;
    }
    return 1;
}

static bool is_layers_line(const std::string& line)
{
    std::istringstream tok(line);
    std::string w;
    return (tok >> w) && w == "layers";
}

static bool parse_layers(const std::string& line, LayersSpec& q)
{
    std::istringstream tok(line);
    std::string w;
    long n = 0;
    if (!(tok >> w >> q.rgb >> n) || w != "layers" || n < 1 || n > 255) return false;
    for (long l = 0; l < n; ++l) {
        std::string m, f;
        if (!(tok >> m >> f)) return false;
        q.masks.push_back(m);
        q.flows.push_back(f);
    }
    for (std::string t; tok >> t;) {
        const size_t eq = t.find('=');
        if (eq == std::string::npos || eq + 1 >= t.size()) return false;
        const std::string k = t.substr(0, eq), v = t.substr(eq + 1);
        std::string* dst = k == "occ" ? &q.occ : k == "bwd" ? &q.bwd : k == "occ_bwd" ? &q.occ_bwd
                         : k == "rgb2" ? &q.rgb2 : k == "mask2" ? &q.mask2 : nullptr;
        if (k == "mid") {
            if (!parse_mid(v, q.mid_steps, q.mid_prefix)) return false;
        } else if (!dst) return false;
        else *dst = v;
        if (q.first_out.empty()) q.first_out = v;
    }
    return !q.first_out.empty();
}

// PREFIX_sII: the stem of the files of the state after ramp step II (pipeline.mid_files)
static std::string mid_stem(const std::string& prefix, unsigned step)
{
    char tag[16];
    snprintf(tag, sizeof(tag), "_s%02u", step);
    return prefix + tag;
}

// the mid= token of a layers line (pipeline.run_layers_mid): `masks` [n][N] and `flows` [n][N][2] are the line's
// layers, already read.  One ArapFlow_WarpLayersStep per snapshot on the state's stream, synchronously.
static bool run_layers_mid(Opt_State* state, const LayersSpec& q, const arapio::Image& rgb,
                           const std::vector<uint8_t>& masks, const std::vector<float>& flows)
{
    const int w = rgb.w, h = rgb.h;
    const size_t N = (size_t)w * h, n = q.masks.size(), ns = q.mid_steps.size();
    // states[k]: the layers' flows after snapshot k; states[ns]: the final flows
    std::vector<std::vector<float>> states(ns);
    for (size_t k = 0; k < ns; ++k) {
        states[k].resize(n * N * 2);
        for (size_t l = 0; l < n; ++l) {
            const std::string& f = q.flows[l];
            if (f.size() < 4 || f.compare(f.size() - 4, 4, ".flo") != 0) {
                printf("layers: mid= needs flows named *.flo, got %s\n", f.c_str());
                return false;
            }
            const std::string snap = mid_stem(f.substr(0, f.size() - 4), q.mid_steps[k]) + ".flo";
            std::vector<float> fl;
            int fw = 0, fh = 0;
            if (!arapio::read_flo(snap, fl, fw, fh)) {
                printf("layers: snapshot %s is missing\n", snap.c_str());
                return false;
            }
            if (fw != w || fh != h) {
                printf("layers: %s differs in size from %s\n", snap.c_str(), q.rgb.c_str());
                return false;
            }
            memcpy(states[k].data() + l * N * 2, fl.data(), N * 8);
        }
    }
    const bool occ = !q.occ.empty();
    const uint64_t scr = std::max(ArapFlow_WarpLayersStepScratchBytes((unsigned)w, (unsigned)h, (unsigned)n),
                                  ArapFlow_WarpLayersScratchBytes((unsigned)w, (unsigned)h, (unsigned)n));
    const size_t off_msk = 3 * N, off_a = (off_msk + n * N + 255) / 256 * 256, off_b = off_a + n * N * 8;
    const size_t off_out = off_b + n * N * 8, out_bytes = 8 * N + 3 * N + N + N;        // step, rgb, mask, occ
    const size_t off_scr = (off_out + out_bytes + 255) / 256 * 256;
    char* d = nullptr;
    if (hipMalloc((void**)&d, off_scr + scr) != hipSuccess) { printf("layers: out of device memory\n"); return false; }
    char* o = d + off_out;
    std::vector<uint8_t> host(out_bytes);
    std::string err;
    auto png = [&](bool written) { if (!written) printf("%s\n", err.c_str()); return written; };
    // ok: the device work went through; wrote: so did the files (a file that did not has said so itself)
    bool wrote = true;
    bool ok = hipMemcpy(d, rgb.rgb.data(), 3 * N, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(d + off_msk, masks.data(), n * N, hipMemcpyHostToDevice) == hipSuccess;
    auto upload = [&](size_t off, size_t k) {
        const float* src = k < ns ? states[k].data() : flows.data();
        return hipMemcpy(d + off, src, n * N * 8, hipMemcpyHostToDevice) == hipSuccess;
    };
    if (ok && occ) {                          // frame 1 -> first snapshot: the layered warp's occlusion of that state
        ok = upload(off_a, 0) &&
             ArapFlow_WarpLayers(state, (unsigned)w, (unsigned)h, (unsigned)n, nullptr, d + off_msk, d + off_a, nullptr,
                                 nullptr, nullptr, nullptr, o + 12 * N, d + off_scr) == 0 &&
             hipDeviceSynchronize() == hipSuccess &&
             hipMemcpy(host.data(), o + 12 * N, N, hipMemcpyDeviceToHost) == hipSuccess;
        if (ok) wrote = png(arapio::write_png_gray8(mid_stem(q.mid_prefix, 0) + "_occ.png", w, h, host.data(), err));
    }
    std::vector<float> own(N * 2);
    for (size_t k = 0; ok && wrote && k < ns; ++k) {
        ok = upload(off_a, k) && upload(off_b, k + 1) &&
             ArapFlow_WarpLayersStep(state, (unsigned)w, (unsigned)h, (unsigned)n, d, d + off_msk, d + off_a, d + off_b,
                                     o + 8 * N, o + 11 * N, o, occ ? o + 12 * N : nullptr, d + off_scr) == 0 &&
             hipDeviceSynchronize() == hipSuccess &&
             hipMemcpy(host.data(), o, out_bytes, hipMemcpyDeviceToHost) == hipSuccess;
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
        const std::string stem = mid_stem(q.mid_prefix, q.mid_steps[k]);
        const uint8_t* hp = host.data();
        wrote = arapio::write_flo(stem + ".flo", own.data(), w, h) &&
                arapio::write_flo(stem + "_step.flo", (const float*)hp, w, h) &&
                png(arapio::write_png_rgb(stem + ".png", w, h, hp + 8 * N, err)) &&
                png(arapio::write_png_mask1(stem + "_mask.png", w, h, hp + 11 * N, err)) &&
                (!occ || png(arapio::write_png_gray8(stem + "_occ.png", w, h, hp + 12 * N, err)));
    }
    (void)hipFree(d);
    if (!ok) printf("ArapFlow_WarpLayersStep failed\n");
    return ok && wrote;
}

// the layered warp of one frame, synchronously: read the layers' files, one ArapFlow_WarpLayers on the state's stream
// (behind whatever solve is in flight there, never beside it), write the outputs asked for
static bool run_layers(Opt_State* state, const LayersSpec& q)
{
    std::string err;
    arapio::Image rgb;
    if (!arapio::read_png_rgb(q.rgb, rgb, err)) { printf("%s\n", err.c_str()); return false; }
    const int w = rgb.w, h = rgb.h;
    const size_t N = (size_t)w * h, n = q.masks.size();
    std::vector<uint8_t> masks(n * N);
    std::vector<float> flows(n * N * 2);
    for (size_t l = 0; l < n; ++l) {
        arapio::Image msk;
        if (!arapio::read_png_rgb(q.masks[l], msk, err)) { printf("%s\n", err.c_str()); return false; }
        std::vector<float> fl;
        int fw = 0, fh = 0;
        if (!arapio::read_flo(q.flows[l], fl, fw, fh)) { printf("Could not read %s\n", q.flows[l].c_str()); return false; }
        if (msk.w != w || msk.h != h || fw != w || fh != h) {
            printf("layers: %s / %s differ in size from %s\n", q.masks[l].c_str(), q.flows[l].c_str(), q.rgb.c_str());
            return false;
        }
        for (size_t i = 0; i < N; ++i) masks[l * N + i] = msk.rgb[3 * i];      // red channel
        memcpy(flows.data() + l * N * 2, fl.data(), N * 8);
    }
    if (!q.mid_steps.empty() && !run_layers_mid(state, q, rgb, masks, flows)) return false;
    if (q.occ.empty() && q.bwd.empty() && q.occ_bwd.empty() && q.rgb2.empty() && q.mask2.empty()) return true;
    const uint64_t scr = ArapFlow_WarpLayersScratchBytes((unsigned)w, (unsigned)h, (unsigned)n);
    const size_t off_msk = 3 * N, off_flow = (off_msk + n * N + 255) / 256 * 256, off_out = off_flow + n * N * 8;
    const size_t out_bytes = 3 * N + N + 8 * N + N + N;
    const size_t off_scr = (off_out + out_bytes + 255) / 256 * 256;
    char* d = nullptr;
    if (hipMalloc((void**)&d, off_scr + scr) != hipSuccess) { printf("layers: out of device memory\n"); return false; }
    char* o = d + off_out;
    void* o_bwd = q.bwd.empty() ? nullptr : o;                      // (float2: first, off_out is 8-byte aligned)
    void* o_rgb = q.rgb2.empty() ? nullptr : o + 8 * N;
    void* o_msk = q.mask2.empty() ? nullptr : o + 11 * N;
    void* o_obwd = q.occ_bwd.empty() ? nullptr : o + 12 * N;
    void* o_occ = q.occ.empty() ? nullptr : o + 13 * N;
    bool ok = hipMemcpy(d, rgb.rgb.data(), 3 * N, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(d + off_msk, masks.data(), n * N, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(d + off_flow, flows.data(), n * N * 8, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && ArapFlow_WarpLayers(state, (unsigned)w, (unsigned)h, (unsigned)n, d, d + off_msk, d + off_flow, o_rgb, o_msk,
                                   o_bwd, o_obwd, o_occ, d + off_scr) == 0;
    ok = ok && hipDeviceSynchronize() == hipSuccess;
    std::vector<uint8_t> host(out_bytes);
    ok = ok && hipMemcpy(host.data(), o, out_bytes, hipMemcpyDeviceToHost) == hipSuccess;
    (void)hipFree(d);
    if (!ok) { printf("ArapFlow_WarpLayers failed\n"); return false; }
    const uint8_t* hp = host.data();
    if (o_rgb && !arapio::write_png_rgb(q.rgb2, w, h, hp + 8 * N, err)) { printf("%s\n", err.c_str()); return false; }
    if (o_msk && !arapio::write_png_mask1(q.mask2, w, h, hp + 11 * N, err)) { printf("%s\n", err.c_str()); return false; }
    if (o_bwd && !arapio::write_flo(q.bwd, (const float*)hp, w, h)) return false;
    if (o_obwd && !arapio::write_png_gray8(q.occ_bwd, w, h, hp + 12 * N, err)) { printf("%s\n", err.c_str()); return false; }
    if (o_occ && !arapio::write_png_gray8(q.occ, w, h, hp + 13 * N, err)) { printf("%s\n", err.c_str()); return false; }
    return true;
}

static bool first_word_is(const std::string& line, const char* word)
{
    std::istringstream tok(line);
    std::string w;
    return (tok >> w) && w == word;
}

// pipeline.parse_bg
static bool parse_bg(const std::string& line, BgSpec& q)
{
    std::istringstream tok(line);
    std::string w;
    if (!(tok >> w >> q.bg >> q.rgb1 >> q.mask1 >> q.rgb2 >> q.mask2 >> q.flow) || w != "bg") return false;
    bool have_m = false;
    for (std::string t; tok >> t;) {
        const size_t eq = t.find('=');
        if (eq == std::string::npos || eq + 1 >= t.size()) return false;
        const std::string k = t.substr(0, eq), v = t.substr(eq + 1);
        if (k == "m") {
            size_t a = 0;
            for (int n = 0; n < 12; ++n) {
                size_t b = v.find(',', a);
                if (b == std::string::npos) b = v.size();
                if ((n < 11) != (b < v.size()) || b == a) return false;
                const std::string num = v.substr(a, b - a);
                char* end = nullptr;
                q.m[n] = strtof(num.c_str(), &end);
                if (end != num.c_str() + num.size()) return false;
                a = b + 1;
            }
            have_m = true;
        } else if (k == "out") {
            const size_t c1 = v.find(','), c2 = c1 == std::string::npos ? c1 : v.find(',', c1 + 1);
            if (c2 == std::string::npos || v.find(',', c2 + 1) != std::string::npos) return false;
            q.out_rgb1 = v.substr(0, c1); q.out_rgb2 = v.substr(c1 + 1, c2 - c1 - 1); q.out_flow = v.substr(c2 + 1);
        } else {
            std::string* dst = k == "occ" ? &q.occ : k == "bwd" ? &q.bwd : k == "occ_bwd" ? &q.occ_bwd
                             : k == "occ_out" ? &q.out_occ : k == "bwd_out" ? &q.out_bwd
                             : k == "occ_bwd_out" ? &q.out_occ_bwd : nullptr;
            if (!dst) return false;
            *dst = v;
        }
    }
    if ((!q.out_occ.empty() && q.occ.empty()) || (!q.out_bwd.empty() && q.bwd.empty()) ||
        (!q.out_occ_bwd.empty() && q.occ_bwd.empty()))
        return false;
    return have_m && !q.first_out().empty();
}

// the moving-background pass of one pair, synchronously (pipeline.run_background): read the line's files, one
// ArapFlow_Background on the state's stream, write the outputs asked for
static bool run_background(Opt_State* state, const BgSpec& q)
{
    std::string err;
    arapio::Image bg, rgb1, rgb2, m1, m2, occ, occ_bwd;
    auto png = [&](const std::string& path, arapio::Image& im) {
        if (arapio::read_png_rgb(path, im, err)) return true;
        printf("%s\n", err.c_str());
        return false;
    };
    if (!png(q.bg, bg) || !png(q.rgb1, rgb1) || !png(q.mask1, m1) || !png(q.rgb2, rgb2) || !png(q.mask2, m2)) return false;
    if (!q.occ.empty() && !png(q.occ, occ)) return false;
    if (!q.occ_bwd.empty() && !png(q.occ_bwd, occ_bwd)) return false;
    const int w = rgb1.w, h = rgb1.h;
    std::vector<float> flow, bwd;
    int fw = 0, fh = 0, bw = w, bh = h;
    if (!arapio::read_flo(q.flow, flow, fw, fh)) return false;
    if (!q.bwd.empty() && !arapio::read_flo(q.bwd, bwd, bw, bh)) return false;
    auto same = [&](const arapio::Image& im) { return im.w == w && im.h == h; };
    if (!same(m1) || !same(rgb2) || !same(m2) || fw != w || fh != h || bw != w || bh != h ||
        (!q.occ.empty() && !same(occ)) || (!q.occ_bwd.empty() && !same(occ_bwd))) {
        printf("bg: image, mask and flow sizes differ: %s\n", q.rgb1.c_str());
        return false;
    }
    const size_t N = (size_t)w * h, B = (size_t)bg.w * bg.h * 3;
    // host staging: the red channels of the masks (cover2 as it is read: non-zero = object) and of the occlusion maps
    std::vector<uint8_t> planes(4 * N, 0);
    for (size_t i = 0; i < N; ++i) {
        planes[i] = m1.rgb[3 * i];
        planes[N + i] = m2.rgb[3 * i] ? 255 : 0;
        if (!q.occ.empty()) planes[2 * N + i] = occ.rgb[3 * i];
        if (!q.occ_bwd.empty()) planes[3 * N + i] = occ_bwd.rgb[3 * i];
    }
    // device: flows first (8-byte aligned), then bytes.  in: flow, bwd, rgb1, rgb2, 4 planes, bg; out: flow_full,
    // bwd_full, rgb1, rgb2, occ_full, occ_bwd_full
    const size_t in_bytes = 16 * N + 6 * N + 4 * N, off_bg = in_bytes, off_out = (off_bg + B + 255) / 256 * 256;
    const size_t out_bytes = 16 * N + 6 * N + 2 * N;
    char* d = nullptr;
    if (hipMalloc((void**)&d, off_out + out_bytes) != hipSuccess) { printf("bg: out of device memory\n"); return false; }
    char* o = d + off_out;
    bool ok = hipMemcpy(d, flow.data(), 8 * N, hipMemcpyHostToDevice) == hipSuccess &&
              (bwd.empty() || hipMemcpy(d + 8 * N, bwd.data(), 8 * N, hipMemcpyHostToDevice) == hipSuccess) &&
              hipMemcpy(d + 16 * N, rgb1.rgb.data(), 3 * N, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(d + 19 * N, rgb2.rgb.data(), 3 * N, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(d + 22 * N, planes.data(), 4 * N, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(d + off_bg, bg.rgb.data(), B, hipMemcpyHostToDevice) == hipSuccess;
    auto want = [](const std::string& path, char* p) -> void* { return path.empty() ? nullptr : p; };
    ok = ok && ArapFlow_Background(state, (unsigned)w, (unsigned)h, d + off_bg, (unsigned)bg.w, (unsigned)bg.h, q.m, q.m + 6,
                                   d + 16 * N, d + 22 * N, d + 19 * N, d + 23 * N, d, q.occ.empty() ? nullptr : d + 24 * N,
                                   q.bwd.empty() ? nullptr : d + 8 * N, q.occ_bwd.empty() ? nullptr : d + 25 * N,
                                   want(q.out_rgb1, o + 16 * N), want(q.out_rgb2, o + 19 * N), want(q.out_flow, o),
                                   want(q.out_occ, o + 22 * N), want(q.out_bwd, o + 8 * N),
                                   want(q.out_occ_bwd, o + 23 * N)) == 0;
    ok = ok && hipDeviceSynchronize() == hipSuccess;
    std::vector<uint8_t> host(out_bytes);
    ok = ok && hipMemcpy(host.data(), o, out_bytes, hipMemcpyDeviceToHost) == hipSuccess;
    (void)hipFree(d);
    if (!ok) { printf("ArapFlow_Background failed\n"); return false; }
    const uint8_t* hp = host.data();
    auto say = [&](bool written) { if (!written) printf("%s\n", err.c_str()); return written; };
    if (!q.out_rgb1.empty() && !say(arapio::write_png_rgb(q.out_rgb1, w, h, hp + 16 * N, err))) return false;
    if (!q.out_rgb2.empty() && !say(arapio::write_png_rgb(q.out_rgb2, w, h, hp + 19 * N, err))) return false;
    if (!q.out_flow.empty() && !arapio::write_flo(q.out_flow, (const float*)hp, w, h)) return false;
    if (!q.out_bwd.empty() && !arapio::write_flo(q.out_bwd, (const float*)(hp + 8 * N), w, h)) return false;
    if (!q.out_occ.empty() && !say(arapio::write_png_gray8(q.out_occ, w, h, hp + 22 * N, err))) return false;
    if (!q.out_occ_bwd.empty() && !say(arapio::write_png_gray8(q.out_occ_bwd, w, h, hp + 23 * N, err))) return false;
    return true;
}

// ---- where the lines come from: a finished list, or stdin as it arrives (--serve) ------------------------------------
struct Loaded { bool ok = false; Frame f; bool is_layers = false, is_bg = false; LayersSpec layers; BgSpec bg; };

struct Item { bool is_layers = false, is_bg = false, bad = false; SolvePaths solve; LayersSpec layers; BgSpec bg; };

// a list / --serve line -> item; false for a line that is none of the forms (a bad `layers` or `bg` line and a bad mid=
// token are reported, and `bad` is set)
static bool parse_item(const std::string& line, Item& it)
{
    if (first_word_is(line, "bg")) {
        it.is_bg = true;
        if (parse_bg(line, it.bg)) return true;
        it.bad = true;
        printf("Invalid bg line: %s\n", line.c_str());
        fflush(stdout);
        return false;
    }
    if (is_layers_line(line)) {
        it.is_layers = true;
        if (parse_layers(line, it.layers)) return true;
        it.bad = true;
        printf("Invalid layers line: %s\n", line.c_str());
        fflush(stdout);
        return false;
    }
    const int rc = parse_line(line, it.solve);
    if (rc == 0) {
        it.bad = true;
        printf("Invalid mid= token: %s\n", line.c_str());
        fflush(stdout);
    }
    return rc == 1;
}

class FrameSource {
  public:
    explicit FrameSource(std::vector<Item> fixed) : eof_(true)
    {
        for (auto& q : fixed) lines_.push_back(std::move(q));
    }
    FrameSource() : eof_(false)                                         // --serve: a thread reads stdin
    {
        reader_ = std::thread([this]() {
            for (std::string line; std::getline(std::cin, line);) {
                Item q;
                if (!parse_item(line, q)) continue;
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
    int next(std::unique_ptr<Loaded>* out, int wait_ms)
    {
        using clock = std::chrono::steady_clock;
        const auto deadline = clock::now() + std::chrono::milliseconds(wait_ms < 0 ? 0 : wait_ms);
        for (;;) {
            start_loads();
            if (!loading_.empty()) {
                std::future<Loaded>& f = loading_.front();
                if (wait_ms < 0) f.wait();
                else if (f.wait_until(deadline) == std::future_status::timeout) return 0;
                out->reset(new Loaded(f.get()));
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
            if (q->is_layers || q->is_bg) {  // read when its turn comes: in a list its inputs may not exist yet
                loading_.push_back(std::async(std::launch::deferred, [q]() {
                    Loaded l; l.ok = true; l.is_layers = q->is_layers; l.is_bg = q->is_bg;
                    l.layers = q->layers; l.bg = q->bg; return l; }));
                continue;
            }
            loading_.push_back(std::async(std::launch::async, [q]() { Loaded l; l.ok = load_frame(q->solve, l.f); return l; }));
        }
    }
    static constexpr size_t kAhead = 48;
    std::mutex m_;
    std::condition_variable cv_;
    std::deque<Item> lines_;
    std::deque<std::future<Loaded>> loading_;
    bool eof_;
    std::thread reader_;
};

// ---- results: read back from the solver's pinned buffers, encoded and written by worker threads ---------------------
struct MidResult { std::vector<float> flow, step; std::vector<uint8_t> rgb, mask; };
struct Result {
    SolvePaths paths;
    std::vector<float> flow, bwd;
    std::vector<uint8_t> wrgb, wmsk, occ_bwd, occ;
    std::vector<MidResult> mid;            // one per snapshot step of the line's mid= token
};

class Writer {
  public:
    explicit Writer(bool report) : report_(report) {}
    void submit(std::shared_ptr<Result> r, int w, int h)
    {
        while (tasks_.size() >= 24) { tasks_.front().get(); tasks_.pop_front(); }
        const bool report = report_;
        std::mutex* pm = &print_;
        tasks_.push_back(std::async(std::launch::async, [r, w, h, report, pm]() {
            std::string err;
            if (!arapio::write_png_rgb(r->paths.warped_rgb, w, h, r->wrgb.data(), err)) printf("%s\n", err.c_str());
            if (!arapio::write_png_mask1(r->paths.warped_mask, w, h, r->wmsk.data(), err)) printf("%s\n", err.c_str());
            arapio::write_flo(r->paths.flow, r->flow.data(), w, h);
            if (!r->paths.bwd.empty()) arapio::write_flo(r->paths.bwd, r->bwd.data(), w, h);
            if (!r->paths.occ_bwd.empty() && !arapio::write_png_gray8(r->paths.occ_bwd, w, h, r->occ_bwd.data(), err))
                printf("%s\n", err.c_str());
            if (!r->paths.occ.empty() && !arapio::write_png_gray8(r->paths.occ, w, h, r->occ.data(), err))
                printf("%s\n", err.c_str());
            for (size_t k = 0; k < r->mid.size(); ++k) {
                const std::string stem = mid_stem(r->paths.mid_prefix, r->paths.mid_steps[k]);
                const MidResult& m = r->mid[k];
                arapio::write_flo(stem + ".flo", m.flow.data(), w, h);
                if (!arapio::write_png_rgb(stem + ".png", w, h, m.rgb.data(), err)) printf("%s\n", err.c_str());
                if (!arapio::write_png_mask1(stem + "_mask.png", w, h, m.mask.data(), err)) printf("%s\n", err.c_str());
                arapio::write_flo(stem + "_step.flo", m.step.data(), w, h);
            }
            std::lock_guard<std::mutex> g(*pm);
            if (report) printf("Done %s\n", r->paths.flow.c_str());     // --serve: one line per finished solve
            else printf("Saved\n");
            fflush(stdout);
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
    bool report_;
    std::mutex print_;
    std::deque<std::future<void>> tasks_;
};

struct Lane {                              // one of the two alternating solver objects
    ArapFlow_Solver* solver = nullptr;
    std::vector<SolvePaths> batch;         // frames set into the slots, in slot order
    bool inflight = false;
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
            if (parse_item(line, q)) lines.push_back(q);
            else if (q.bad) return 1;
        }
        if (lines.empty()) {
            printf("No file to be processed");
            return 1;
        }
        source.reset(new FrameSource(std::move(lines)));
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
    const unsigned numIter = 19, nonLinearIter = 8, linearIter = 400;    // main.cpp:215-221
    // Frames per solve call: the library gives every solve a group of the resident launch's workgroups sized by its
    // active tiles and a launch costs the same however full it is, so frames join a batch while they still fit ONE
    // launch (ArapFlow_SolverLaunchesFor); minFill frames per call when the resident kernel does not apply.
    // Both bounds follow the frame size: a solver object pins 24 bytes x vertices x maxBatch of host staging (two objects:
    // 0.6 GB at 854x480 x 32 -- but 3.2 GB at 1920x1080 x 32, where a launch holds four segment solves anyway).
    auto max_batch_for = [](int w, int h) -> unsigned {
        const double rel = (double)w * h / (854.0 * 480.0);
        const int m = (int)(32.0 / (rel < 1.0 ? 1.0 : rel));
        return (unsigned)(m < 8 ? 8 : m);
    };
    unsigned maxBatch = 32;
    const unsigned minFill = 8;
    // --serve: how long a partly filled batch waits for another line when the GPU is idle
    int linger_ms = 30;
    if (const char* e = getenv("ARAP_DEFORM_LINGER_MS")) linger_ms = atoi(e);

    Writer writer(serve);
    Lane lanes[2];
    int sw = 0, sh = 0, cur = 0;
    std::unique_ptr<Loaded> carry;           // decoded frame that did not fit the batch it was offered to
    bool exhausted = false;
    int rc = 0;

    auto drain = [&](Lane& L) -> bool {      // wait for the lane's solve, hand its results to the writer threads
        if (!L.inflight) return true;
        if (ArapFlow_SolverWait(L.solver) != 0) { printf("ARAP solve failed\n"); return false; }
        const size_t n = (size_t)sw * sh;
        for (size_t b = 0; b < L.batch.size(); ++b) {                    // copyResultToCPU
            const float* flow; const uint8_t *wrgb, *wmsk;
            if (ArapFlow_SolverHostResults(L.solver, (unsigned)b, &flow, &wrgb, &wmsk) != 0 || !wrgb) {
                printf("ARAP results unavailable\n");
                return false;
            }
            auto r = std::make_shared<Result>();
            r->paths = L.batch[b];
            r->flow.assign(flow, flow + 2 * n);
            r->wrgb.assign(wrgb, wrgb + 3 * n);
            r->wmsk.assign(wmsk, wmsk + n);
            if (r->paths.outputs()) {
                const float* bwd; const uint8_t *obwd, *occ;
                if (ArapFlow_SolverHostExtraResults(L.solver, (unsigned)b, &bwd, &obwd, &occ) != 0) {
                    printf("ARAP extra results unavailable\n");
                    return false;
                }
                if (bwd) { r->bwd.assign(bwd, bwd + 2 * n); r->occ_bwd.assign(obwd, obwd + n); }
                if (occ) r->occ.assign(occ, occ + n);
            }
            for (unsigned k = 0; k < r->paths.mid_steps.size(); ++k) {
                const float *mf, *ms; const uint8_t *mr, *mm;
                if (ArapFlow_SolverHostSnapshot(L.solver, (unsigned)b, k, &mf, &mr, &mm, &ms) != 0 || !mr) {
                    printf("ARAP snapshots unavailable\n");
                    return false;
                }
                MidResult m;
                m.flow.assign(mf, mf + 2 * n); m.step.assign(ms, ms + 2 * n);
                m.rgb.assign(mr, mr + 3 * n); m.mask.assign(mm, mm + n);
                r->mid.push_back(std::move(m));
            }
            writer.submit(r, sw, sh);
        }
        L.batch.clear();
        L.inflight = false;
        return true;
    };
    auto launch = [&](Lane& L) -> bool {
        if (L.batch.empty()) return true;
        int outputs = 0;                     // what any line of the batch asks for (off for plain lines: no extra kernel)
        for (const SolvePaths& q : L.batch) outputs |= q.outputs();
        if (ArapFlow_SolverSetOutputs(L.solver, outputs) != 0) {
            printf("ARAP outputs could not be set\n");
            return false;
        }
        // snapshots are on iff a line of the batch asks (plain batches run nothing new); its mid= lines name the same steps
        const std::vector<unsigned>* steps = nullptr;
        for (const SolvePaths& q : L.batch) {
            if (q.mid_steps.empty()) continue;
            if (steps && *steps != q.mid_steps) {
                printf("mid= steps differ from those of the batch: %s\n", q.flow.c_str());
                return false;
            }
            steps = &q.mid_steps;
        }
        if (ArapFlow_SolverSetSnapshots(L.solver, steps ? steps->data() : nullptr, steps ? (unsigned)steps->size() : 0) != 0) {
            printf("ARAP snapshots could not be set\n");
            return false;
        }
        if (ArapFlow_SolverSolveAsync(L.solver, (unsigned)L.batch.size(), numIter, nonLinearIter, linearIter, 1, 1) != 0) {
            printf("ARAP solve could not be started\n");
            return false;
        }
        if (serve) { printf("Batch %zu\n", L.batch.size()); fflush(stdout); }    // (para_gen.py keeps statistics)
        L.inflight = true;
        return true;
    };

    while (rc == 0) {
        Lane& L = lanes[cur];
        Lane& other = lanes[cur ^ 1];
        // ---- next frame: the carried one, or whatever the source has.  An empty batch with nothing in flight blocks;
        //      a partly filled one waits `linger_ms` (while the other lane is solving, waiting costs nothing: drain it
        //      first, new lines may arrive meanwhile)
        std::unique_ptr<Loaded> fr;
        bool full = false;
        if (carry) fr = std::move(carry);
        else if (!exhausted) {
            int got;
            if (L.batch.empty() && !other.inflight) got = source->next(&fr, -1);
            else {
                got = source->next(&fr, 0);
                if (got == 0 && other.inflight) {
                    if (!drain(other)) { rc = 1; break; }
                    got = source->next(&fr, 0);
                }
                if (got == 0) got = source->next(&fr, L.batch.empty() ? -1 : linger_ms);
            }
            if (got < 0) exhausted = true;
        }
        if (fr && (fr->is_layers || fr->is_bg)) {
            // A list: every earlier line is solved and written first (this line's inputs may be their outputs).  --serve:
            // the sender names only files that exist, so nothing is flushed; the call queues behind the solve in flight.
            if (!serve) {
                if (!launch(L) || !drain(other) || !drain(L)) { rc = 1; break; }
                writer.finish();
            }
            if (!(fr->is_bg ? run_background(state, fr->bg) : run_layers(state, fr->layers))) { rc = 1; break; }
            writer.say(serve ? "Done " + (fr->is_bg ? fr->bg.first_out() : fr->layers.first_out) : std::string("Saved"));
            continue;
        }
        if (fr) {
            if (!fr->ok) { rc = 1; break; }
            const int w = fr->f.rgb.w, h = fr->f.rgb.h;
            if (w != sw || h != sh) {
                // another frame size: finish everything of the old size, then re-build (CombinedSolver.h:149-160)
                if (!launch(L) || !drain(other) || !drain(L)) { rc = 1; break; }
                if (lanes[0].solver) {
                    printf("Warning: Input image has different size to one in the prebuilt plan.\n"
                           "To avoid re-building the plan and to save time, put images of the same size in the same list.\n"
                           "Starting to re-build plan...\n");            // CombinedSolver.h:151-153
                    ArapFlow_SolverFree(lanes[0].solver);
                    ArapFlow_SolverFree(lanes[1].solver);
                }
                maxBatch = max_batch_for(w, h);
                lanes[0].solver = ArapFlow_SolverCreate(state, (unsigned)w, (unsigned)h, maxBatch);
                lanes[1].solver = ArapFlow_SolverCreate(state, (unsigned)w, (unsigned)h, maxBatch);
                if (!lanes[0].solver || !lanes[1].solver) { rc = 1; break; }
                sw = w; sh = h;
            }
            const unsigned b = (unsigned)L.batch.size();
            if (ArapFlow_SolverSetFrame(L.solver, b, fr->f.rgb.rgb.data(), fr->f.mask_red.data(), fr->f.constraints.data(),
                                        (unsigned)(fr->f.constraints.size() / 4), 0) != 0) { rc = 1; break; }   // addImage
            bool fits = true;
            if (b > 0) {
                const int launches = ArapFlow_SolverLaunchesFor(L.solver, b + 1);
                fits = !(launches > 1 || (launches == 0 && b >= minFill));
            }
            if (fits) {
                L.batch.push_back(fr->f.paths);
                full = L.batch.size() >= maxBatch;
            } else {
                carry = std::move(fr);                                   // opens the next batch (set again there)
                full = true;
            }
            if (!full) continue;
        }
        // ---- nothing more joins this batch: start it, then turn to the other lane (its results, then its next batch)
        if (!L.batch.empty()) {
            if (!launch(L)) { rc = 1; break; }
            if (!drain(other)) { rc = 1; break; }
            cur ^= 1;
        } else if (exhausted && !carry) {
            break;
        }
    }
    if (rc == 0 && (!drain(lanes[cur ^ 1]) || !drain(lanes[cur]))) rc = 1;
    writer.finish();
    for (Lane& L : lanes)
        if (L.solver) ArapFlow_SolverFree(L.solver);
    ArapFlow_FreeState(state);
    fflush(stdout);
    if (rc != 0) _exit(rc);                  // (--serve: the stdin reader may still be blocked in getline)
    return rc;
}
