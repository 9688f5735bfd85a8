// line_tool -- test helper for the list-line grammar (list_line.h): reads lines on stdin and prints, per line,
//   SKIP                      the line is none of the forms
//   BAD                       a form, refused (after parse_item's own "Invalid ..." line)
//   <canonical> done=<path>   what was read, written as pipeline.format_line writes it, and the path the line is
//                             reported done by (pipeline.done_token)
// and, as `line_tool format score|fscore|tscore|lscore|mscore [frames|L|thresholds]` with a table's integers on stdin,
// the text device_pass.h's format_* makes of it.  Neither mode needs a device.
#include <cstdlib>
#include <iostream>
#include <vector>

#include "device_pass.h"
#include "list_line.h"

struct Canon {
    std::string text;
    void word(const std::string& s) { text += (text.empty() ? "" : " ") + s; }
    void token(const char* key, const std::string& value)              // left out when empty, as format_line does
    {
        if (!value.empty()) word(std::string(key) + "=" + value);
    }
};

static std::string canonical(const Item& it)
{
    Canon c;
    if (it.kind == Item::Kind::Solve) {
        const SolvePaths& q = it.solve;
        for (const std::string* s : {&q.rgb, &q.mask, &q.constraints, &q.flow, &q.warped_rgb, &q.warped_mask}) c.word(*s);
        c.token("bwd", q.bwd); c.token("occ", q.occ); c.token("occ_bwd", q.occ_bwd); c.token("mid", q.mid.text);
        c.token("diag", q.diag); c.token("fold", q.fold);
    } else if (it.kind == Item::Kind::Layers) {
        const LayersSpec& q = it.layers;
        c.word("layers"); c.word(q.rgb); c.word(std::to_string(q.masks.size()));
        for (size_t l = 0; l < q.masks.size(); ++l) { c.word(q.masks[l]); c.word(q.flows[l]); }
        c.token("occ", q.occ); c.token("bwd", q.bwd); c.token("occ_bwd", q.occ_bwd); c.token("rgb2", q.rgb2);
        c.token("mask2", q.mask2); c.token("mid", q.mid.text);
    } else if (it.kind == Item::Kind::Tex) {
        const TexSpec& q = it.tex;
        c.word("tex"); c.word(q.rgb); c.word(std::to_string(q.masks.size()));
        for (size_t l = 0; l < q.masks.size(); ++l) { c.word(q.masks[l]); c.word(q.flows[l]); }
        std::string t;
        for (const ArapFlow_TexLayer& L : q.tex) {
            char num[512];
            snprintf(num, sizeof(num), "%s%u,%u,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%u,%u,%u,%u,%u,%u,%u,%u,%u", t.empty() ? "" : ";",
                     L.kind, L.seed, L.m[0], L.m[1], L.m[2], L.m[3], L.m[4], L.m[5], L.p0, L.p1, L.c0[0], L.c0[1], L.c0[2],
                     L.c1[0], L.c1[1], L.c1[2], L.c2[0], L.c2[1], L.c2[2]);
            t += num;
        }
        c.token("t", t); c.token("rgb1", q.rgb1); c.token("rgb2", q.rgb2); c.token("mask2", q.mask2);
    } else if (it.kind == Item::Kind::Trk) {
        const TrkSpec& q = it.trk;
        c.word("trk"); c.word(q.points); c.word(std::to_string(q.masks.size())); c.word(std::to_string(q.states));
        for (size_t l = 0; l < q.masks.size(); ++l) {
            c.word(q.masks[l]);
            for (unsigned s = 0; s < q.states; ++s) c.word(q.flows[l * q.states + s]);
        }
        c.token("out", q.out);
    } else if (it.kind == Item::Kind::Blur) {
        const BlurSpec& q = it.blur;
        c.word("blur"); c.word(q.rgb); c.word(std::to_string(q.masks.size()));
        for (size_t l = 0; l < q.masks.size(); ++l) { c.word(q.masks[l]); c.word(q.flows[l]); }
        c.word(q.bg);
        char num[64];
        snprintf(num, sizeof(num), "%.9g,%u", q.shutter, q.samples);
        c.token("b", num);
        std::string m;
        for (int k = 0; q.have_m && k < 12; ++k) {
            snprintf(num, sizeof(num), "%s%.9g", k ? "," : "", q.m[k]);
            m += num;
        }
        c.token("m", m); c.token("rgb1", q.rgb1); c.token("rgb2", q.rgb2); c.token("alpha1", q.alpha1); c.token("alpha2", q.alpha2);
    } else if (it.kind == Item::Kind::Seg) {
        const SegSpec& q = it.seg;
        c.word("seg"); c.word(std::to_string(q.masks.size()));
        for (size_t l = 0; l < q.masks.size(); ++l) { c.word(q.masks[l]); c.word(q.flows[l]); }
        char num[64];
        snprintf(num, sizeof(num), "%.9g,%u", q.tau, q.radius);
        c.token("s", num);
        std::string m;
        for (int k = 0; q.have_m && k < 12; ++k) {
            snprintf(num, sizeof(num), "%s%.9g", k ? "," : "", q.m[k]);
            m += num;
        }
        c.token("m", m); c.token("idx1", q.idx1); c.token("idx2", q.idx2); c.token("mb1", q.mb1); c.token("mb2", q.mb2);
        c.token("dist1", q.dist1); c.token("dist2", q.dist2);
    } else if (it.kind == Item::Kind::Score) {
        const ScoreSpec& q = it.score;
        c.word("score"); c.word(q.gt); c.word(q.est);
        c.token("occ", q.occ); c.token("dist", q.dist); c.token("skip", q.skip); c.token("mask", q.mask); c.token("out", q.out);
    } else if (it.kind == Item::Kind::TScore) {
        const TScoreSpec& q = it.tscore;
        c.word("tscore"); c.word(q.gt); c.word(q.est);
        char num[64];
        snprintf(num, sizeof(num), "%.9g,%.9g", q.sx, q.sy);
        if (q.sx != 1.f || q.sy != 1.f) c.token("s", num);
        c.token("out", q.out);
    } else if (it.kind == Item::Kind::Chain) {
        const ChainSpec& q = it.chain;
        c.word("chain"); c.word(q.points); c.word(std::to_string(q.flows.size()));
        for (const std::string& f : q.flows) c.word(f);
        std::string b;
        for (size_t j = 0; j < q.bwd.size(); ++j) b += (j ? "," : "") + q.bwd[j];
        c.token("bwd", b); c.token("out", q.out);
    } else if (it.kind == Item::Kind::FScore) {
        const FScoreSpec& q = it.fscore;
        c.word("fscore"); c.word(q.ref); c.word(q.est);
        c.token("occ", q.occ); c.token("dist", q.dist); c.token("skip", q.skip); c.token("obj", q.obj); c.token("out", q.out);
    } else if (it.kind == Item::Kind::Interp) {
        const InterpSpec& q = it.interp;
        c.word("interp"); c.word(q.a); c.word(q.b); c.word(q.fwd);
        std::string steps;
        for (size_t j = 0; j < q.steps.size(); ++j) steps += (j ? "," : "") + std::to_string(q.steps[j]);
        c.token("s", steps); c.token("n", std::to_string(q.n)); c.token("bwd", q.bwd); c.token("src", q.src ? "1" : "");
        c.token("out", q.out);
    } else if (it.kind == Item::Kind::LScore) {
        const LScoreSpec& q = it.lscore;
        c.word("lscore"); c.word(q.gt); c.word(q.est);
        c.token("l", std::to_string(q.L)); c.token("r", std::to_string(q.radius)); c.token("skip", q.skip); c.token("out", q.out);
    } else if (it.kind == Item::Kind::MScore) {
        const MScoreSpec& q = it.mscore;
        c.word("mscore"); c.word(q.gt); c.word(q.est);
        std::string thr;
        for (size_t j = 0; j < q.thr.size(); ++j) thr += (j ? "," : "") + std::to_string(q.thr[j]);
        c.token("t", thr); c.token("r", q.thr.empty() ? "" : std::to_string(q.radius)); c.token("skip", q.skip); c.token("out", q.out);
    } else if (it.kind == Item::Kind::Light) {
        const LightSpec& q = it.light;
        c.word("light"); c.word(q.rgb1); c.word(q.mask1); c.word(q.rgb2); c.word(q.cover2);
        std::string l;
        char num[64];
        for (int f = 0; f < 2; ++f) {
            const ArapFlow_LightFrame& a = q.frames[f];
            snprintf(num, sizeof(num), "%s%u", f ? ";" : "", a.seed);
            l += num;
            const float fl[12] = {a.m[0], a.m[1], a.m[2], a.m[3], a.m[4], a.m[5], a.amp, a.vig, a.gain[0], a.gain[1], a.gain[2], a.gamma};
            for (float v : fl) { snprintf(num, sizeof(num), ",%.9g", v); l += num; }
            snprintf(num, sizeof(num), ",%d,%d,%d,%d,%.9g,%.9g", a.sh_dx, a.sh_dy, a.sh_r, a.sh_g, a.sigma0, a.sigma1);
            l += num;
        }
        c.token("l", l); c.token("rgb1", q.out1); c.token("rgb2", q.out2);
    } else {
        const BgSpec& q = it.bg;
        c.word("bg");
        for (const std::string* s : {&q.bg, &q.rgb1, &q.mask1, &q.rgb2, &q.mask2, &q.flow}) c.word(*s);
        auto numbers = [](const float* v, size_t count) {
            std::string m;
            for (size_t n = 0; n < count; ++n) {
                char num[32];
                snprintf(num, sizeof(num), "%s%.9g", n ? "," : "", v[n]);
                m += num;
            }
            return m;
        };
        c.token("m", numbers(q.m, 12)); c.token("mid", q.mid.text); c.token("mm", numbers(q.mm.data(), q.mm.size()));
        c.token("occ", q.occ); c.token("bwd", q.bwd); c.token("occ_bwd", q.occ_bwd);
        if (!(q.out_rgb1 + q.out_rgb2 + q.out_flow).empty()) c.word("out=" + q.out_rgb1 + "," + q.out_rgb2 + "," + q.out_flow);
        c.token("occ_out", q.out_occ); c.token("bwd_out", q.out_bwd); c.token("occ_bwd_out", q.out_occ_bwd);
        c.token("mid_out", q.mid_out);
    }
    return c.text + " done=" + done_path(it);
}

// `line_tool format KIND [SIZE]`: the table's integers on stdin -> the text of its score file; false for a bad call
static bool print_score_file(const std::string& kind, unsigned size)
{
    std::vector<uint64_t> v;
    for (uint64_t x; std::cin >> x;) v.push_back(x);
    const size_t want = kind == "score"    ? ARAPFLOW_SCORE_ROWS * ARAPFLOW_SCORE_FIELDS
                        : kind == "fscore" ? ARAPFLOW_FSCORE_ROWS * ARAPFLOW_FSCORE_FIELDS
                        : kind == "tscore" ? (size_t)size * ARAPFLOW_TSCORE_CLASSES * ARAPFLOW_TSCORE_FIELDS
                        : kind == "lscore" ? ((size_t)size + 1) * ARAPFLOW_LSCORE_FIELDS
                        : kind == "mscore" ? 512 + (size_t)size * 5
                                           : 0;
    if (!want || v.size() != want) return false;
    std::vector<unsigned> thr(v.begin() + (kind == "mscore" ? 512 : 0), v.begin() + (kind == "mscore" ? 512 + size : 0));
    const std::string text = kind == "score"    ? format_score(v.data())
                             : kind == "fscore" ? format_frame_score(v.data())
                             : kind == "tscore" ? format_track_score(v.data(), size)
                             : kind == "lscore" ? format_label_score(v.data(), size)
                                                : format_map_score(v.data(), thr.data(), size, v.data() + 512 + size);
    fputs(text.c_str(), stdout);
    return true;
}

int main(int argc, char** argv)
{
    if (argc > 1)               // mscore's integers: the histogram, SIZE thresholds, SIZE match rows
        return argc >= 3 && std::string(argv[1]) == "format" && print_score_file(argv[2], argc > 3 ? (unsigned)atoi(argv[3]) : 0) ? 0 : 2;
    for (std::string line; std::getline(std::cin, line);) {
        Item it;
        const Parsed p = parse_item(line, it);
        printf("%s\n", p == Parsed::Skip ? "SKIP" : p == Parsed::Bad ? "BAD" : canonical(it).c_str());
    }
    return 0;
}
