// list_line.h -- the grammar of one list / --serve line of arap_deform, and nothing else: no HIP, no files.  The C++ twin of
// pipeline.parse_line / done_token; line_tool.cpp prints what it reads so that a test can hold the two side by side.
//   solve line:   RGB MASK CONSTRAINTS FLOW WARPED_RGB WARPED_MASK [bwd=P] [occ=P] [occ_bwd=P] [mid=I1,I2,..:PREFIX]
//                 [diag=P.txt] [fold=P.png]
//                 other trailing tokens are ignored (a line's words after the sixth always were); a malformed mid= is
//                 the only error
//   layers line:  layers RGB n MASK_1 FLO_1 ... MASK_n FLO_n [occ=P] [bwd=P] [occ_bwd=P] [rgb2=P] [mask2=P] [mid=..:PREFIX]
//   bg line:      bg BG RGB1 MASK1 RGB2 MASK2 FLOW m=<12 numbers> [mid=I1,..,In:PREFIX mm=<6n numbers>] [occ=IN] [bwd=IN]
//                 [occ_bwd=IN] out=RGB1_OUT,RGB2_OUT,FLOW_OUT [occ_out=P] [bwd_out=P] [occ_bwd_out=P] [mid_out=PREFIX_OUT]
//                 mid=, mm= and mid_out= come together
//   tex line:     tex RGB1 n MASK_1 FLO_1 ... MASK_n FLO_n t=<layer 1>;...;<layer n> [rgb1=P] [rgb2=P] [mask2=P]
//                 a layer: 19 numbers, comma separated: kind, seed, the six of m, p0, p1, nine palette bytes
//                 (pipeline.TexLine); a repeated key is an error too
//   trk line:     trk PTS.trk n T  MASK_1 FLO_1,1 .. FLO_1,T  ..  MASK_n FLO_n,1 .. FLO_n,T  out=OUT.trk
//                 (pipeline.TrkLine): every state file named, exactly one token, out=, after them
//   blur line:    blur RGB1 n MASK_1 FLO_1 ... MASK_n FLO_n BG b=<shutter>,<samples> [m=<12 numbers: M1 then M2>]
//                 [rgb1=P] [rgb2=P] [alpha1=P] [alpha2=P]
//                 (pipeline.BlurLine): the shutter a finite number >= 0, 1 .. ARAPFLOW_MAX_BLUR_SAMPLES samples, the maps
//                 finite; without m= both maps are the identity; a repeated key is an error too
//   light line:   light RGB1 MASK1 RGB2 COVER2 l=<frame 1>;<frame 2> [rgb1=P] [rgb2=P]
//                 (pipeline.LightLine): a frame the 19 numbers of ArapFlow_LightFrame in field order, every one in the
//                 range ArapFlow_LightTables accepts; a repeated key is an error too
//   seg line:     seg n MASK_1 FLO_1 ... MASK_n FLO_n s=<tau>,<radius> [m=<12 numbers: M1 then M2>]
//                 [idx1=P] [idx2=P] [mb1=P] [mb2=P] [dist1=P] [dist2=P]
//                 (pipeline.SegLine): tau a finite number >= 0, the radius 0 .. ARAPFLOW_SEG_MAX_RADIUS, the maps finite;
//                 without m= the background is static; a repeated key is an error too
//   score line:   score GT.flo EST.flo [occ=PNG] [dist=PNG] [skip=PNG] [mask=PNG] out=TXT
//                 (pipeline.ScoreLine): a repeated key is an error too
//   tscore line:  tscore GT.trk EST.trk [s=SX,SY] out=TXT
//                 (pipeline.TScoreLine): the factors finite and > 0; a repeated key is an error too
//   chain line:   chain PTS.trk L FLO_1 .. FLO_L [bwd=B_1,..,B_L] out=OUT.trk
//                 (pipeline.ChainLine): 1 <= L < ARAPFLOW_TSCORE_MAX_FRAMES, bwd= names L files; a repeated key is an error too
//   fscore line:  fscore REF.png EST.png [occ=PNG] [dist=PNG] [skip=PNG] [obj=PNG] out=TXT
//                 (pipeline.FScoreLine): a repeated key is an error too
//   interp line:  interp A.png B.png FWD.flo s=I1,I2,.. n=N [bwd=BWD.flo] [src=1] out=PREFIX
//                 (pipeline.InterpLine): 1 to ARAPFLOW_INTERP_MAX_TIMES steps, 1 <= I1 < I2 < .. < N; a repeated key is an error too
//   lscore line:  lscore GT.png EST.png l=<L> r=<radius> [skip=PNG] out=TXT
//                 (pipeline.LScoreLine): 1 <= L <= 255, radius 0 .. ARAPFLOW_SEG_MAX_RADIUS; a repeated key is an error too
//   mscore line:  mscore GT.png EST.png [t=<thr,...> r=<radius>] [skip=PNG] out=TXT
//                 (pipeline.MScoreLine): 1 to ARAPFLOW_MSCORE_MAX_THR thresholds 1..255; t= and r= both or neither; a
//                 repeated key is an error too
//                 on these fourteen any unknown key, missing `=` or empty value is an error, and so is a line without output
#pragma once
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <sstream>
#include <string>
#include <vector>

extern "C" {
#include "../../include/arap_opt.h"
}

// ---- the one tokeniser: KEY=VALUE (the value may be empty; the first `=` splits) and the table a form looks KEY up in
inline bool split_token(const std::string& t, std::string& key, std::string& value)
{
    const size_t eq = t.find('=');
    if (eq == std::string::npos) return false;
    key = t.substr(0, eq);
    value = t.substr(eq + 1);
    return true;
}

struct TokenField { const char* key; std::string* dst; };

inline std::string* field_of(std::initializer_list<TokenField> fields, const std::string& key)
{
    for (const TokenField& f : fields)
        if (key == f.key) return f.dst;
    return nullptr;
}

// ---- mid=I1,I2,..:PREFIX with 1 <= I1 < I2 < .., at most ARAPFLOW_MAX_SNAPSHOTS indices (DESIGN.md "In-between frames")
struct Mid {
    std::string text;                      // as written after `mid=` (empty: not wanted)
    std::vector<unsigned> steps;
    std::string prefix;
};

inline bool parse_mid(const std::string& v, Mid& mid)
{
    const size_t colon = v.find(':');
    if (colon == std::string::npos || colon + 1 >= v.size()) return false;
    mid.steps.clear();
    unsigned x = 0, digits = 0;
    for (size_t k = 0; k <= colon; ++k) {                  // an index of at most six digits, ended by `,` or the `:`
        if (v[k] >= '0' && v[k] <= '9' && digits < 6) {
            x = 10 * x + (unsigned)(v[k] - '0');
            ++digits;
            continue;
        }
        if ((v[k] != ',' && v[k] != ':') || digits == 0 || x < 1 || (!mid.steps.empty() && x <= mid.steps.back())) return false;
        mid.steps.push_back(x);
        x = digits = 0;
    }
    if (mid.steps.size() > ARAPFLOW_MAX_SNAPSHOTS) return false;
    mid.prefix = v.substr(colon + 1);
    mid.text = v;
    return true;
}

// PREFIX_sII: the stem of the files of the state after ramp step II (pipeline.mid_files)
inline std::string mid_stem(const std::string& prefix, unsigned step)
{
    char tag[16];
    snprintf(tag, sizeof(tag), "_s%02u", step);
    return prefix + tag;
}

// ---- the fifteen forms
struct SolvePaths {                        // ARAP/deformation/src/main.cpp:4-11,183-191
    std::string rgb, mask, constraints, flow, warped_rgb, warped_mask;
    std::string bwd, occ, occ_bwd;         // optional outputs (empty: not wanted)
    Mid mid;
    std::string diag, fold;                // fold diagnostics (DESIGN.md "Fold diagnostics"; empty: not wanted)
    bool wants_diag() const { return !diag.empty() || !fold.empty(); }
    int outputs() const
    {
        return (bwd.empty() && occ_bwd.empty() ? 0 : ARAPFLOW_OUT_BACKWARD) | (occ.empty() ? 0 : ARAPFLOW_OUT_OCCLUSION);
    }
};

struct LayersSpec {
    std::string rgb;
    std::vector<std::string> masks, flows;
    std::string occ, bwd, occ_bwd, rgb2, mask2;
    Mid mid;                               // its prefix: that of the composite files
    std::string first_out;                 // the value of the first output token in line order: what --serve reports
};

struct BgSpec {                            // pipeline.BgLine
    std::string bg, rgb1, mask1, rgb2, mask2, flow;
    float m[12];                           // M1, M2
    std::string occ, bwd, occ_bwd;         // optional object-side inputs
    std::string out_rgb1, out_rgb2, out_flow, out_occ, out_bwd, out_occ_bwd;      // outputs (empty: not wanted)
    Mid mid;                               // the pair's in-between files (DESIGN.md "Moving background over in-between frames")
    std::vector<float> mm;                 // their sampling maps, six numbers each
    std::string mid_out;                   // the prefix of the sequence's files (pipeline.mid_bg_files)
    std::string first_out() const          // in the order of pipeline.bg_outputs
    {
        for (const std::string* q : {&out_rgb1, &out_rgb2, &out_flow, &out_occ, &out_bwd, &out_occ_bwd})
            if (!q->empty()) return *q;
        return mid_out.empty() ? std::string() : mid_stem(mid_out, mid.steps[0]) + ".png";
    }
};

struct TexSpec {                           // pipeline.TexLine
    std::string rgb;
    std::vector<std::string> masks, flows;
    std::vector<ArapFlow_TexLayer> tex;    // one per layer
    std::string rgb1, rgb2, mask2;         // outputs (empty: not wanted)
    std::string first_out;                 // the value of the first output token in line order: what --serve reports
};

struct TrkSpec {                           // pipeline.TrkLine
    std::string points;
    std::vector<std::string> masks;        // [n]
    std::vector<std::string> flows;        // [n][T]: layer l's state s is flows[l * T + s]
    unsigned states = 0;                   // T
    std::string out;
};

struct BlurSpec {                          // pipeline.BlurLine
    std::string rgb, bg;
    std::vector<std::string> masks, flows;
    float shutter = 0.f;
    unsigned samples = 0;                  // 0: no b= seen yet
    bool have_m = false;
    float m[12] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f};     // M1, M2; the identity without m=
    std::string rgb1, rgb2, alpha1, alpha2;        // outputs (empty: not wanted)
    std::string first_out;                 // the value of the first output token in line order: what --serve reports
};

struct LightSpec {                         // pipeline.LightLine
    std::string rgb1, mask1, rgb2, cover2;
    bool have_l = false;
    ArapFlow_LightFrame frames[2] = {};
    std::string out1, out2;                // outputs rgb1=, rgb2= (empty: not wanted)
    std::string first_out;                 // the value of the first output token in line order: what --serve reports
};

struct SegSpec {                           // pipeline.SegLine
    std::vector<std::string> masks, flows;
    bool have_s = false, have_m = false;
    float tau = 0.f;
    unsigned radius = 0;
    float m[12] = {};                      // M1, M2; read only with have_m
    std::string idx1, idx2, mb1, mb2, dist1, dist2;        // outputs (empty: not wanted)
    std::string first_out;                 // the value of the first output token in line order: what --serve reports
};

struct ScoreSpec {                         // pipeline.ScoreLine
    std::string gt, est;
    std::string occ, dist, skip, mask;     // optional planes (empty: not given)
    std::string out;
};

struct TScoreSpec {                        // pipeline.TScoreLine
    std::string gt, est;
    float sx = 1.f, sy = 1.f;
    bool have_s = false;
    std::string out;
};

struct ChainSpec {                         // pipeline.ChainLine
    std::string points;
    std::vector<std::string> flows, bwd;   // L files; bwd L or none
    std::string out;
};

struct FScoreSpec {                        // pipeline.FScoreLine
    std::string ref, est;
    std::string occ, dist, skip, obj;      // optional planes (empty: not given)
    std::string out;
};

struct LScoreSpec {                        // pipeline.LScoreLine
    std::string gt, est;
    unsigned L = 0, radius = 0;
    std::string skip;                      // optional plane (empty: not given)
    std::string out;
};

struct MScoreSpec {                        // pipeline.MScoreLine
    std::string gt, est;
    std::vector<unsigned> thr;             // none: the histogram alone
    unsigned radius = 0;
    std::string skip;                      // optional plane (empty: not given)
    std::string out;
};

struct InterpSpec {                        // pipeline.InterpLine
    std::string a, b, fwd;
    std::vector<unsigned> steps;           // ramp steps: the times are (float)step / (float)n
    unsigned n = 0;
    std::string bwd;                       // optional input (empty: not given)
    bool src = false;                      // also write the source maps
    std::string out;                       // the prefix of the files
};

struct Item {
    enum class Kind { Solve, Layers, Bg, Tex, Trk, Blur, Light, Seg, Score, TScore, Chain, FScore, Interp, LScore, MScore } kind = Kind::Solve;
    SolvePaths solve;
    LayersSpec layers;
    BgSpec bg;
    TexSpec tex;
    TrkSpec trk;
    BlurSpec blur;
    LightSpec light;
    SegSpec seg;
    ScoreSpec score;
    TScoreSpec tscore;
    ChainSpec chain;
    FScoreSpec fscore;
    InterpSpec interp;
    LScoreSpec lscore;
    MScoreSpec mscore;
};

// the path `arap_deform --serve` reports a line done by (pipeline.done_token)
inline std::string done_path(const Item& it)
{
    return it.kind == Item::Kind::Solve    ? it.solve.flow
           : it.kind == Item::Kind::Layers ? it.layers.first_out
           : it.kind == Item::Kind::Tex    ? it.tex.first_out
           : it.kind == Item::Kind::Trk    ? it.trk.out
           : it.kind == Item::Kind::Blur   ? it.blur.first_out
           : it.kind == Item::Kind::Light  ? it.light.first_out
           : it.kind == Item::Kind::Seg    ? it.seg.first_out
           : it.kind == Item::Kind::Score  ? it.score.out
           : it.kind == Item::Kind::TScore ? it.tscore.out
           : it.kind == Item::Kind::Chain  ? it.chain.out
           : it.kind == Item::Kind::FScore ? it.fscore.out
           : it.kind == Item::Kind::Interp ? it.interp.out
           : it.kind == Item::Kind::LScore ? it.lscore.out
           : it.kind == Item::Kind::MScore ? it.mscore.out
                                           : it.bg.first_out();
}

enum class Parsed { Skip, Bad, Good };     // Skip: none of the forms; Bad: a form, refused

inline Parsed parse_solve(std::istringstream& tok, SolvePaths& q)
{
    if (!(tok >> q.mask >> q.constraints >> q.flow >> q.warped_rgb >> q.warped_mask)) return Parsed::Skip;
    std::string k, v;
    for (std::string t; tok >> t;) {
        if (!split_token(t, k, v)) continue;
        if (k == "mid") {
            if (!v.empty() && !parse_mid(v, q.mid)) return Parsed::Bad;
        } else if (std::string* dst = field_of({{"bwd", &q.bwd}, {"occ", &q.occ}, {"occ_bwd", &q.occ_bwd},
                                                {"diag", &q.diag}, {"fold", &q.fold}}, k))
            *dst = v;
    }
    return Parsed::Good;
}

inline bool parse_layers(std::istringstream& tok, LayersSpec& q)
{
    long n = 0;
    if (!(tok >> q.rgb >> n) || n < 1 || n > 255) return false;
    for (long l = 0; l < n; ++l) {
        std::string m, f;
        if (!(tok >> m >> f)) return false;
        q.masks.push_back(m);
        q.flows.push_back(f);
    }
    std::string k, v;
    for (std::string t; tok >> t;) {
        if (!split_token(t, k, v) || v.empty()) return false;
        if (k == "mid") {
            if (!parse_mid(v, q.mid)) return false;
        } else if (std::string* dst = field_of({{"occ", &q.occ}, {"bwd", &q.bwd}, {"occ_bwd", &q.occ_bwd}, {"rgb2", &q.rgb2},
                                                {"mask2", &q.mask2}}, k))
            *dst = v;
        else return false;
        if (q.first_out.empty()) q.first_out = v;
    }
    return !q.first_out.empty();
}

// `count` numbers, comma separated, nothing else
inline bool parse_bg_maps(const std::string& v, float* m, size_t count)
{
    const char* p = v.c_str();
    for (size_t n = 0; n < count; ++n) {
        char* end = nullptr;
        m[n] = strtof(p, &end);
        if (end == p || *end != (n + 1 < count ? ',' : '\0')) return false;
        p = end + 1;
    }
    return true;
}

inline bool parse_bg(std::istringstream& tok, BgSpec& q)
{
    if (!(tok >> q.bg >> q.rgb1 >> q.mask1 >> q.rgb2 >> q.mask2 >> q.flow)) return false;
    bool have_m = false, have_mm = false;
    std::string k, v, mm;
    for (std::string t; tok >> t;) {
        if (!split_token(t, k, v) || v.empty()) return false;
        if (k == "m") {
            if (!parse_bg_maps(v, q.m, 12)) return false;
            have_m = true;
        } else if (k == "mid") {
            if (!parse_mid(v, q.mid)) return false;
        } else if (k == "mm") {            // (counted once the line is read: mid= may come after it)
            mm = v;
            have_mm = true;
        } else if (k == "out") {           // three places, each may be empty
            const size_t c1 = v.find(','), c2 = c1 == std::string::npos ? c1 : v.find(',', c1 + 1);
            if (c2 == std::string::npos || v.find(',', c2 + 1) != std::string::npos) return false;
            q.out_rgb1 = v.substr(0, c1); q.out_rgb2 = v.substr(c1 + 1, c2 - c1 - 1); q.out_flow = v.substr(c2 + 1);
        } else if (std::string* dst = field_of({{"occ", &q.occ}, {"bwd", &q.bwd}, {"occ_bwd", &q.occ_bwd},
                                                {"occ_out", &q.out_occ}, {"bwd_out", &q.out_bwd},
                                                {"occ_bwd_out", &q.out_occ_bwd}, {"mid_out", &q.mid_out}}, k))
            *dst = v;
        else return false;
    }
    if ((!q.out_occ.empty() && q.occ.empty()) || (!q.out_bwd.empty() && q.bwd.empty()) ||
        (!q.out_occ_bwd.empty() && q.occ_bwd.empty()))
        return false;                      // an output needs its input
    if (!q.mid.text.empty() || have_mm || !q.mid_out.empty()) {                    // all three or none
        if (q.mid.text.empty() || !have_mm || q.mid_out.empty()) return false;
        q.mm.resize(6 * q.mid.steps.size());
        if (!parse_bg_maps(mm, q.mm.data(), q.mm.size())) return false;
    }
    return have_m && !q.first_out().empty();
}

// 1 to 10 decimal digits, nothing else, at most `max`
inline bool parse_uint(const std::string& v, unsigned long long max, unsigned long long& x)
{
    if (v.empty() || v.size() > 10) return false;
    x = 0;
    for (char c : v) {
        if (c < '0' || c > '9') return false;
        x = 10 * x + (unsigned long long)(c - '0');
    }
    return x <= max;
}

// one layer of t=: 19 numbers, comma separated (pipeline.TexLayer); the floats finite
inline bool parse_tex_layer(const std::string& v, ArapFlow_TexLayer& q)
{
    std::vector<std::string> f(1);
    for (char c : v) {
        if (c == ',') f.emplace_back();
        else f.back() += c;
    }
    if (f.size() != 19) return false;
    unsigned long long x = 0;
    if (!parse_uint(f[0], ARAPFLOW_TEX_WAVE, x)) return false;
    q.kind = (uint32_t)x;
    if (!parse_uint(f[1], 0xffffffffull, x)) return false;
    q.seed = (uint32_t)x;
    float fl[8];
    for (int k = 0; k < 8; ++k)
        if (!parse_bg_maps(f[2 + k], fl + k, 1) || !std::isfinite(fl[k])) return false;
    for (int k = 0; k < 6; ++k) q.m[k] = fl[k];
    q.p0 = fl[6]; q.p1 = fl[7];
    uint8_t* const cols[3] = {q.c0, q.c1, q.c2};
    for (int k = 0; k < 9; ++k) {
        if (!parse_uint(f[10 + k], 255, x)) return false;
        cols[k / 3][k % 3] = (uint8_t)x;
    }
    q.reserved[0] = q.reserved[1] = q.reserved[2] = 0;
    return true;
}

inline bool parse_tex(std::istringstream& tok, TexSpec& q)
{
    std::string count;
    unsigned long long n = 0;
    if (!(tok >> q.rgb >> count) || !parse_uint(count, 255, n) || n < 1) return false;
    for (unsigned long long l = 0; l < n; ++l) {
        std::string m, f;
        if (!(tok >> m >> f)) return false;
        q.masks.push_back(m);
        q.flows.push_back(f);
    }
    std::string k, v;
    for (std::string t; tok >> t;) {
        if (!split_token(t, k, v) || v.empty()) return false;
        if (k == "t") {
            if (!q.tex.empty()) return false;
            size_t at = 0;
            for (;;) {                     // layers separated by `;`
                const size_t semi = v.find(';', at);
                ArapFlow_TexLayer layer;
                if (!parse_tex_layer(v.substr(at, semi == std::string::npos ? semi : semi - at), layer)) return false;
                q.tex.push_back(layer);
                if (semi == std::string::npos) break;
                at = semi + 1;
            }
            if (q.tex.size() != n) return false;
        } else if (std::string* dst = field_of({{"rgb1", &q.rgb1}, {"rgb2", &q.rgb2}, {"mask2", &q.mask2}}, k)) {
            if (!dst->empty()) return false;
            *dst = v;
            if (q.first_out.empty()) q.first_out = v;
        } else return false;
    }
    return !q.tex.empty() && !q.first_out.empty();
}

inline bool parse_trk(std::istringstream& tok, TrkSpec& q)
{
    std::string count, states;
    unsigned long long n = 0, T = 0;
    if (!(tok >> q.points >> count >> states) || !parse_uint(count, 255, n) || n < 1 ||
        !parse_uint(states, ARAPFLOW_MAX_SNAPSHOTS + 1, T) || T < 1)
        return false;
    q.states = (unsigned)T;
    std::string k, v;
    if (split_token(q.points, k, v)) return false;
    for (unsigned long long l = 0; l < n; ++l)
        for (unsigned long long s = 0; s <= T; ++s) {      // the mask, then the T states
            std::string path;
            if (!(tok >> path) || split_token(path, k, v)) return false;
            (s == 0 ? q.masks : q.flows).push_back(path);
        }
    std::string t, more;
    if (!(tok >> t) || !split_token(t, k, v) || k != "out" || v.empty() || (tok >> more)) return false;
    q.out = v;
    return true;
}

inline bool parse_blur(std::istringstream& tok, BlurSpec& q)
{
    std::string count, k, v;
    unsigned long long n = 0, x = 0;
    if (!(tok >> q.rgb >> count) || split_token(q.rgb, k, v) || !parse_uint(count, 255, n) || n < 1) return false;
    for (unsigned long long l = 0; l < n; ++l) {
        std::string m, f;
        if (!(tok >> m >> f) || split_token(m, k, v) || split_token(f, k, v)) return false;
        q.masks.push_back(m);
        q.flows.push_back(f);
    }
    if (!(tok >> q.bg) || split_token(q.bg, k, v)) return false;
    for (std::string t; tok >> t;) {
        if (!split_token(t, k, v) || v.empty()) return false;
        if (k == "b") {                    // <shutter>,<samples>
            const size_t comma = v.find(',');
            if (q.samples != 0 || comma == std::string::npos) return false;
            if (!parse_bg_maps(v.substr(0, comma), &q.shutter, 1) || !std::isfinite(q.shutter) || q.shutter < 0.f) return false;
            if (!parse_uint(v.substr(comma + 1), ARAPFLOW_MAX_BLUR_SAMPLES, x) || x < 1) return false;
            q.samples = (unsigned)x;
        } else if (k == "m") {
            if (q.have_m || !parse_bg_maps(v, q.m, 12)) return false;
            for (float c : q.m)
                if (!std::isfinite(c)) return false;
            q.have_m = true;
        } else if (std::string* dst = field_of({{"rgb1", &q.rgb1}, {"rgb2", &q.rgb2}, {"alpha1", &q.alpha1},
                                                {"alpha2", &q.alpha2}}, k)) {
            if (!dst->empty()) return false;
            *dst = v;
            if (q.first_out.empty()) q.first_out = v;
        } else return false;
    }
    return q.samples != 0 && !q.first_out.empty();
}

// 1 to 10 decimal digits after an optional `-`, nothing else
inline bool parse_int(const std::string& v, long long& x)
{
    const bool neg = !v.empty() && v[0] == '-';
    unsigned long long u = 0;
    if (!parse_uint(neg ? v.substr(1) : v, 9999999999ull, u)) return false;
    x = neg ? -(long long)u : (long long)u;
    return true;
}

// one frame of l=: 19 numbers, comma separated (pipeline.LightFrame), in the ranges ArapFlow_LightTables accepts
inline bool parse_light_frame(const std::string& v, ArapFlow_LightFrame& q)
{
    std::vector<std::string> f(1);
    for (char c : v) {
        if (c == ',') f.emplace_back();
        else f.back() += c;
    }
    if (f.size() != 19) return false;
    unsigned long long x = 0;
    if (!parse_uint(f[0], 0xffffffffull, x)) return false;
    q.seed = (uint32_t)x;
    float fl[14];
    for (int k = 0; k < 14; ++k)
        if (!parse_bg_maps(f[k < 12 ? 1 + k : 5 + k], fl + k, 1)) return false;
    for (int k = 0; k < 6; ++k) q.m[k] = fl[k];
    q.amp = fl[6]; q.vig = fl[7];
    for (int k = 0; k < 3; ++k) q.gain[k] = fl[8 + k];
    q.gamma = fl[11]; q.sigma0 = fl[12]; q.sigma1 = fl[13];
    long long s[4];
    if (!parse_int(f[13], s[0]) || !parse_int(f[14], s[1])) return false;
    for (int k = 2; k < 4; ++k) {
        if (!parse_uint(f[13 + k], 9999999999ull, x)) return false;
        s[k] = (long long)x;
    }
    for (long long t : s)
        if (t < -1000000 || t > 1000000) return false;             // (out of range anyway; what is left fits an int32)
    q.sh_dx = (int32_t)s[0]; q.sh_dy = (int32_t)s[1]; q.sh_r = (int32_t)s[2]; q.sh_g = (int32_t)s[3];
    uint8_t lut[3][256];
    float geom[3];
    return ArapFlow_LightTables(&q, 1, 1, lut, geom) == 0;         // the ranges, stated once (host only)
}

inline bool parse_light(std::istringstream& tok, LightSpec& q)
{
    std::string k, v;
    if (!(tok >> q.rgb1 >> q.mask1 >> q.rgb2 >> q.cover2)) return false;
    for (const std::string* p : {&q.rgb1, &q.mask1, &q.rgb2, &q.cover2})
        if (split_token(*p, k, v)) return false;
    for (std::string t; tok >> t;) {
        if (!split_token(t, k, v) || v.empty()) return false;
        if (k == "l") {                    // two frames separated by `;`
            const size_t semi = v.find(';');
            if (q.have_l || semi == std::string::npos) return false;
            if (!parse_light_frame(v.substr(0, semi), q.frames[0]) || !parse_light_frame(v.substr(semi + 1), q.frames[1])) return false;
            q.have_l = true;
        } else if (std::string* dst = field_of({{"rgb1", &q.out1}, {"rgb2", &q.out2}}, k)) {
            if (!dst->empty()) return false;
            *dst = v;
            if (q.first_out.empty()) q.first_out = v;
        } else return false;
    }
    return q.have_l && !q.first_out.empty();
}

inline bool parse_seg(std::istringstream& tok, SegSpec& q)
{
    std::string count, k, v;
    unsigned long long n = 0, x = 0;
    if (!(tok >> count) || !parse_uint(count, 255, n) || n < 1) return false;
    for (unsigned long long l = 0; l < n; ++l) {
        std::string m, f;
        if (!(tok >> m >> f) || split_token(m, k, v) || split_token(f, k, v)) return false;
        q.masks.push_back(m);
        q.flows.push_back(f);
    }
    for (std::string t; tok >> t;) {
        if (!split_token(t, k, v) || v.empty()) return false;
        if (k == "s") {                    // <tau>,<radius>
            const size_t comma = v.find(',');
            if (q.have_s || comma == std::string::npos) return false;
            if (!parse_bg_maps(v.substr(0, comma), &q.tau, 1) || !std::isfinite(q.tau) || q.tau < 0.f) return false;
            if (!parse_uint(v.substr(comma + 1), ARAPFLOW_SEG_MAX_RADIUS, x)) return false;
            q.radius = (unsigned)x;
            q.have_s = true;
        } else if (k == "m") {
            if (q.have_m || !parse_bg_maps(v, q.m, 12)) return false;
            for (float c : q.m)
                if (!std::isfinite(c)) return false;
            q.have_m = true;
        } else if (std::string* dst = field_of({{"idx1", &q.idx1}, {"idx2", &q.idx2}, {"mb1", &q.mb1}, {"mb2", &q.mb2},
                                                {"dist1", &q.dist1}, {"dist2", &q.dist2}}, k)) {
            if (!dst->empty()) return false;
            *dst = v;
            if (q.first_out.empty()) q.first_out = v;
        } else return false;
    }
    return q.have_s && !q.first_out.empty();
}

inline bool parse_score(std::istringstream& tok, ScoreSpec& q)
{
    std::string k, v;
    if (!(tok >> q.gt >> q.est) || split_token(q.gt, k, v) || split_token(q.est, k, v)) return false;
    for (std::string t; tok >> t;) {
        if (!split_token(t, k, v) || v.empty()) return false;
        std::string* const dst = field_of({{"occ", &q.occ}, {"dist", &q.dist}, {"skip", &q.skip}, {"mask", &q.mask}, {"out", &q.out}}, k);
        if (!dst || !dst->empty()) return false;
        *dst = v;
    }
    return !q.out.empty();
}

inline bool parse_tscore(std::istringstream& tok, TScoreSpec& q)
{
    std::string k, v;
    if (!(tok >> q.gt >> q.est) || split_token(q.gt, k, v) || split_token(q.est, k, v)) return false;
    for (std::string t; tok >> t;) {
        if (!split_token(t, k, v) || v.empty()) return false;
        if (k == "s") {                    // <sx>,<sy>
            float s[2];
            if (q.have_s || !parse_bg_maps(v, s, 2)) return false;
            for (float c : s)
                if (!std::isfinite(c) || !(c > 0.f)) return false;
            q.sx = s[0]; q.sy = s[1];
            q.have_s = true;
        } else if (k == "out") {
            if (!q.out.empty()) return false;
            q.out = v;
        } else return false;
    }
    return !q.out.empty();
}

inline bool parse_chain(std::istringstream& tok, ChainSpec& q)
{
    std::string count, k, v;
    unsigned long long L = 0;
    if (!(tok >> q.points >> count) || split_token(q.points, k, v) || !parse_uint(count, ARAPFLOW_TSCORE_MAX_FRAMES - 1, L) || L < 1)
        return false;
    for (unsigned long long j = 0; j < L; ++j) {
        std::string path;
        if (!(tok >> path) || split_token(path, k, v)) return false;
        q.flows.push_back(path);
    }
    for (std::string t; tok >> t;) {
        if (!split_token(t, k, v) || v.empty()) return false;
        if (k == "bwd") {                  // L files, comma separated, none empty
            if (!q.bwd.empty()) return false;
            q.bwd.emplace_back();
            for (char c : v) {
                if (c == ',') q.bwd.emplace_back();
                else q.bwd.back() += c;
            }
            if (q.bwd.size() != L) return false;
            for (const std::string& b : q.bwd)
                if (b.empty()) return false;
        } else if (k == "out") {
            if (!q.out.empty()) return false;
            q.out = v;
        } else return false;
    }
    return !q.out.empty();
}

inline bool parse_fscore(std::istringstream& tok, FScoreSpec& q)
{
    std::string k, v;
    if (!(tok >> q.ref >> q.est) || split_token(q.ref, k, v) || split_token(q.est, k, v)) return false;
    for (std::string t; tok >> t;) {
        if (!split_token(t, k, v) || v.empty()) return false;
        std::string* const dst = field_of({{"occ", &q.occ}, {"dist", &q.dist}, {"skip", &q.skip}, {"obj", &q.obj}, {"out", &q.out}}, k);
        if (!dst || !dst->empty()) return false;
        *dst = v;
    }
    return !q.out.empty();
}

inline bool parse_interp(std::istringstream& tok, InterpSpec& q)
{
    std::string k, v, steps, n, src;
    if (!(tok >> q.a >> q.b >> q.fwd) || split_token(q.a, k, v) || split_token(q.b, k, v) || split_token(q.fwd, k, v)) return false;
    for (std::string t; tok >> t;) {
        if (!split_token(t, k, v) || v.empty()) return false;
        std::string* const dst = field_of({{"s", &steps}, {"n", &n}, {"bwd", &q.bwd}, {"src", &src}, {"out", &q.out}}, k);
        if (!dst || !dst->empty()) return false;
        *dst = v;
    }
    unsigned long long x = 0;
    if (steps.empty() || q.out.empty() || !parse_uint(n, 0xffffffffull, x) || (!src.empty() && src != "1")) return false;
    q.n = (unsigned)x;
    q.src = !src.empty();
    steps += ',';
    std::string one;
    for (char c : steps) {                 // decimal steps, comma separated, strictly ascending, 1 <= step < n
        if (c != ',') { one += c; continue; }
        if (!parse_uint(one, 0xffffffffull, x) || x < 1 || x >= q.n || (!q.steps.empty() && x <= q.steps.back())) return false;
        q.steps.push_back((unsigned)x);
        one.clear();
    }
    return q.steps.size() <= ARAPFLOW_INTERP_MAX_TIMES;
}

inline bool parse_lscore(std::istringstream& tok, LScoreSpec& q)
{
    std::string k, v, l, r;
    if (!(tok >> q.gt >> q.est) || split_token(q.gt, k, v) || split_token(q.est, k, v)) return false;
    for (std::string t; tok >> t;) {
        if (!split_token(t, k, v) || v.empty()) return false;
        std::string* const dst = field_of({{"l", &l}, {"r", &r}, {"skip", &q.skip}, {"out", &q.out}}, k);
        if (!dst || !dst->empty()) return false;
        *dst = v;
    }
    unsigned long long x = 0, y = 0;
    if (q.out.empty() || !parse_uint(l, 255, x) || x < 1 || !parse_uint(r, ARAPFLOW_SEG_MAX_RADIUS, y)) return false;
    q.L = (unsigned)x;
    q.radius = (unsigned)y;
    return true;
}

inline bool parse_mscore(std::istringstream& tok, MScoreSpec& q)
{
    std::string k, v, thr, r;
    if (!(tok >> q.gt >> q.est) || split_token(q.gt, k, v) || split_token(q.est, k, v)) return false;
    for (std::string t; tok >> t;) {
        if (!split_token(t, k, v) || v.empty()) return false;
        std::string* const dst = field_of({{"t", &thr}, {"r", &r}, {"skip", &q.skip}, {"out", &q.out}}, k);
        if (!dst || !dst->empty()) return false;
        *dst = v;
    }
    if (q.out.empty() || thr.empty() != r.empty()) return false;
    if (thr.empty()) return true;
    unsigned long long x = 0;
    if (!parse_uint(r, ARAPFLOW_SEG_MAX_RADIUS, x)) return false;
    q.radius = (unsigned)x;
    thr += ',';
    std::string one;
    for (char c : thr) {                   // decimal thresholds, comma separated, each 1..255
        if (c != ',') { one += c; continue; }
        if (!parse_uint(one, 255, x) || x < 1) return false;
        q.thr.push_back((unsigned)x);
        one.clear();
    }
    return q.thr.size() <= ARAPFLOW_MSCORE_MAX_THR;
}

// a list / --serve line -> item.  A refused form is reported here, on stdout.
inline Parsed parse_item(const std::string& line, Item& it)
{
    std::istringstream tok(line);
    std::string first;
    if (!(tok >> first)) return Parsed::Skip;
    it.kind = first == "bg" ? Item::Kind::Bg : first == "layers" ? Item::Kind::Layers : first == "tex" ? Item::Kind::Tex
              : first == "trk" ? Item::Kind::Trk : first == "blur" ? Item::Kind::Blur : first == "light" ? Item::Kind::Light
              : first == "seg" ? Item::Kind::Seg : first == "score" ? Item::Kind::Score : first == "tscore" ? Item::Kind::TScore
              : first == "chain" ? Item::Kind::Chain : first == "fscore" ? Item::Kind::FScore : first == "interp" ? Item::Kind::Interp
              : first == "lscore" ? Item::Kind::LScore : first == "mscore" ? Item::Kind::MScore : Item::Kind::Solve;
    it.solve.rgb = first;
    Parsed p;
    if (it.kind == Item::Kind::Solve) p = parse_solve(tok, it.solve);
    else if (it.kind == Item::Kind::Tex) p = parse_tex(tok, it.tex) ? Parsed::Good : Parsed::Bad;
    else if (it.kind == Item::Kind::Trk) p = parse_trk(tok, it.trk) ? Parsed::Good : Parsed::Bad;
    else if (it.kind == Item::Kind::Blur) p = parse_blur(tok, it.blur) ? Parsed::Good : Parsed::Bad;
    else if (it.kind == Item::Kind::Light) p = parse_light(tok, it.light) ? Parsed::Good : Parsed::Bad;
    else if (it.kind == Item::Kind::Seg) p = parse_seg(tok, it.seg) ? Parsed::Good : Parsed::Bad;
    else if (it.kind == Item::Kind::Score) p = parse_score(tok, it.score) ? Parsed::Good : Parsed::Bad;
    else if (it.kind == Item::Kind::TScore) p = parse_tscore(tok, it.tscore) ? Parsed::Good : Parsed::Bad;
    else if (it.kind == Item::Kind::Chain) p = parse_chain(tok, it.chain) ? Parsed::Good : Parsed::Bad;
    else if (it.kind == Item::Kind::FScore) p = parse_fscore(tok, it.fscore) ? Parsed::Good : Parsed::Bad;
    else if (it.kind == Item::Kind::Interp) p = parse_interp(tok, it.interp) ? Parsed::Good : Parsed::Bad;
    else if (it.kind == Item::Kind::LScore) p = parse_lscore(tok, it.lscore) ? Parsed::Good : Parsed::Bad;
    else if (it.kind == Item::Kind::MScore) p = parse_mscore(tok, it.mscore) ? Parsed::Good : Parsed::Bad;
    else p = (it.kind == Item::Kind::Bg ? parse_bg(tok, it.bg) : parse_layers(tok, it.layers)) ? Parsed::Good : Parsed::Bad;
    if (p == Parsed::Bad) {
        const char* const what[] = {"mid= token", "layers line", "bg line", "tex line", "trk line", "blur line", "light line", "seg line", "score line",
                                    "tscore line", "chain line", "fscore line", "interp line", "lscore line",
                                    "mscore line"};      // by Item::Kind
        printf("Invalid %s: %s\n", what[(int)it.kind], line.c_str());
        fflush(stdout);
    }
    return p;
}
