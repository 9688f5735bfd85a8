// device_pass.h -- what the synchronous passes of the host programs share (warp_image; the layers and bg lines of
// arap_deform): one device allocation laid out part by part, one table of the outputs a pass may write, one file writer.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../include/arap_opt.h"
#include "flo_io.h"
#include "png_io.h"

enum class FileKind { flo, rgb, mask1, gray8 };      // .flo float2; RGB PNG; 1-bit PNG of a 0/255 mask; 8-bit L PNG

inline size_t bytes_per_pixel(FileKind kind) { return kind == FileKind::flo ? 8 : kind == FileKind::rgb ? 3 : 1; }

// one output file of [h][w] pixels; a failure is reported here, in the codec's words
inline bool save(FileKind kind, const std::string& path, int w, int h, const void* data)
{
    if (kind == FileKind::flo) return arapio::write_flo(path, (const float*)data, w, h);      // (says so itself)
    const uint8_t* px = (const uint8_t*)data;
    std::string err;
    const bool ok = kind == FileKind::rgb     ? arapio::write_png_rgb(path, w, h, px, err)
                    : kind == FileKind::mask1 ? arapio::write_png_mask1(path, w, h, px, err)
                                              : arapio::write_png_gray8(path, w, h, px, err);
    if (!ok) printf("%s\n", err.c_str());
    return ok;
}

// the text of a diag file (pipeline.format_diag): the struct's fields in order, without `reserved`
inline std::string format_diag(const ArapFlow_MeshStats& s)
{
    char text[512];
    snprintf(text, sizeof(text),
             "vertices %u\noutside %u\ntriangles %u\nfolded %u\nnonfinite %u\ndet_min %.9g\ndet_max %.9g\ndisp2_max %.9g\n",
             s.vertices, s.outside, s.triangles, s.folded, s.nonfinite, (double)s.det_min, (double)s.det_max,
             (double)s.disp2_max);
    return text;
}

// one row of a score file (scores.format_row): `head`, then ` key=value` for each of `count` integers, then the newline
inline void append_row(std::string& text, const std::string& head, const char* const* keys, const uint64_t* values, int count)
{
    text += head;
    char cell[64];
    for (int k = 0; k < count; ++k) {
        snprintf(cell, sizeof(cell), " %s=%llu", keys[k], (unsigned long long)values[k]);
        text += cell;
    }
    text += "\n";
}

// a fixed table (scores.FixedTable): a row of `nfields` fields per name of `rows`, then `left_out` with its two keys
inline std::string format_fixed_table(const uint64_t* table, const char* const* rows, int nrows, const char* const* fields, int nfields,
                                      const char* const* left_keys)
{
    std::string text;
    for (int r = 0; r < nrows; ++r) append_row(text, rows[r], fields, table + r * nfields, nfields);
    append_row(text, "left_out", left_keys, table + nrows * nfields, 2);
    return text;
}

// the text of a score file (pipeline.format_score): one line per row of ArapFlow_FlowScore's table, integers only
inline std::string format_score(const uint64_t* table)
{
    static const char* const rows[ARAPFLOW_SCORE_ROWS - 1] = {"all", "noc", "occ", "d0-10", "d10-60", "d60-140", "s0-10", "s10-40", "s40+"};
    static const char* const fields[ARAPFLOW_SCORE_FIELDS] = {"count", "sum", "n1", "n3", "n5", "fl", "nonfinite", "max"};
    static const char* const left[2] = {"skipped", "gt_nonfinite"};
    return format_fixed_table(table, rows, ARAPFLOW_SCORE_ROWS - 1, fields, ARAPFLOW_SCORE_FIELDS, left);
}

// the text of a track score file (pipeline.format_track_score): one line per frame and class of ArapFlow_TrackScore's
// table, integers only
inline std::string format_track_score(const uint64_t* table, unsigned frames)
{
    static const char* const classes[ARAPFLOW_TSCORE_CLASSES] = {"all", "tracked", "reappeared"};
    static const char* const fields[ARAPFLOW_TSCORE_FIELDS] = {"count", "gt_vis", "est_vis", "agree", "within_1", "within_2", "within_4",
                                                               "within_8", "within_16", "tp_1", "tp_2", "tp_4", "tp_8", "tp_16", "sum", "max"};
    std::string text;
    for (unsigned f = 0; f < frames; ++f)
        for (int c = 0; c < ARAPFLOW_TSCORE_CLASSES; ++c)
            append_row(text, std::to_string(f) + " " + classes[c], fields,
                       table + ((size_t)f * ARAPFLOW_TSCORE_CLASSES + c) * ARAPFLOW_TSCORE_FIELDS, ARAPFLOW_TSCORE_FIELDS);
    return text;
}

// the text of a frame score file (pipeline.format_frame_score): one line per row of ArapFlow_FrameScore's table, integers only
inline std::string format_frame_score(const uint64_t* table)
{
    static const char* const rows[ARAPFLOW_FSCORE_ROWS - 1] = {"all", "noc", "occ", "d0-10", "d10-60", "d60-140", "obj", "bg"};
    static const char* const fields[ARAPFLOW_FSCORE_FIELDS] = {"count", "sse", "sad", "max", "windows", "ssim_sum", "ssim_worst"};
    static const char* const left[2] = {"pixels", "windows"};
    return format_fixed_table(table, rows, ARAPFLOW_FSCORE_ROWS - 1, fields, ARAPFLOW_FSCORE_FIELDS, left);
}

// the text of a label score file (pipeline.format_label_score): the frame's row, then one line per label of
// ArapFlow_LabelScore's table uint64[L + 1][8], integers only
inline std::string format_label_score(const uint64_t* table, unsigned L)
{
    static const char* const frame[5] = {"counted", "skipped", "equal", "gt_above", "est_above"};
    static const char* const fields[ARAPFLOW_LSCORE_FIELDS - 1] = {"gt", "est", "inter", "gt_b", "est_b", "gt_hit", "est_hit"};
    std::string text;
    append_row(text, "frame", frame, table, 5);
    for (unsigned k = 1; k <= L; ++k)
        append_row(text, "label " + std::to_string(k), fields, table + k * ARAPFLOW_LSCORE_FIELDS, ARAPFLOW_LSCORE_FIELDS - 1);
    return text;
}

// the text of a map score file (pipeline.format_map_score): the two rows of ArapFlow_MapScore's histogram, which have no
// keys, then one line per threshold of its match table, integers only
inline std::string format_map_score(const uint64_t* hist, const unsigned* thr, unsigned m, const uint64_t* match)
{
    static const char* const fields[4] = {"a", "b", "a_hit", "b_hit"};
    std::string text;
    for (int c = 0; c < 2; ++c) {
        text += c ? "pos" : "neg";
        for (int v = 0; v < 256; ++v) text += " " + std::to_string(hist[c * 256 + v]);
        text += "\n";
    }
    for (unsigned j = 0; j < m; ++j) append_row(text, "match thr=" + std::to_string(thr[j]), fields, match + 4 * j, 4);
    return text;
}

// a text file, as it is; says why not
inline bool save_text(const std::string& path, const void* data, size_t bytes)
{
    FILE* f = fopen(path.c_str(), "wb");
    const bool ok = f && fwrite(data, 1, bytes, f) == bytes;
    if (f && fclose(f) != 0) return printf("Could not write %s\n", path.c_str()), false;
    if (!ok) printf("Could not write %s\n", path.c_str());
    return ok;
}

// One hipMalloc per pass.  Lay the parts out first -- take(), or stage() for an input that is there already; each part
// starts 256-byte aligned, the library's rule for scratch and enough for float2 -- then alloc(), then upload().  A part
// is named by what take() returned; kNone names no part and has the address NULL.  Freed with the object.
class DeviceArena {
  public:
    static constexpr size_t kNone = ~(size_t)0;
    DeviceArena() = default;
    DeviceArena(const DeviceArena&) = delete;
    DeviceArena& operator=(const DeviceArena&) = delete;
    ~DeviceArena() { if (base_) (void)hipFree(base_); }
    size_t take(size_t bytes)
    {
        const size_t part = size_;
        size_ = (size_ + bytes + 255) / 256 * 256;
        return part;
    }
    size_t stage(const void* src, size_t bytes)
    {
        staged_.push_back(Staged{take(bytes), src, bytes});
        return staged_.back().part;
    }
    hipError_t alloc() { return hipMalloc((void**)&base_, size_ ? size_ : 256); }
    hipError_t upload() const                              // every staged input
    {
        hipError_t e = hipSuccess;
        for (const Staged& s : staged_)
            if (e == hipSuccess) e = copy_in(s.part, s.src, s.bytes);
        return e;
    }
    hipError_t copy_in(size_t part, const void* src, size_t bytes) const
    {
        return hipMemcpy(at(part), src, bytes, hipMemcpyHostToDevice);
    }
    char* at(size_t part) const { return part == kNone ? nullptr : base_ + part; }

  private:
    struct Staged { size_t part; const void* src; size_t bytes; };
    char* base_ = nullptr;
    size_t size_ = 0;
    std::vector<Staged> staged_;
};

// The outputs a pass may write, one row each, in the order their files are written.  The row gives the library call its
// "pointer or NULL", then downloads and writes that same part, so an output cannot end in another one's file.
class OutputTable {
  public:
    OutputTable(DeviceArena& arena, int w, int h) : arena_(arena), w_(w), h_(h) {}
    // a row; an empty path (not wanted) takes no device memory unless `keep` (set_path names it later, per call)
    size_t add(FileKind kind, const std::string& path, bool keep = false)
    {
        rows_.push_back(Row{kind, path, path.empty() && !keep ? DeviceArena::kNone : arena_.take(bytes(kind)), {}});
        return rows_.size() - 1;
    }
    void set_path(size_t row, const std::string& path) { if (rows_[row].part != DeviceArena::kNone) rows_[row].path = path; }
    void* dev(size_t row) const { return rows_[row].path.empty() ? nullptr : arena_.at(rows_[row].part); }
    void* part(size_t row) const { return arena_.at(rows_[row].part); }       // a kept row's memory, named or not
    hipError_t download()                                  // every wanted row, once the call has been waited for
    {
        hipError_t e = hipSuccess;
        for (Row& r : rows_) {
            if (r.path.empty() || e != hipSuccess) continue;
            r.data.resize(bytes(r.kind));
            e = hipMemcpy(r.data.data(), arena_.at(r.part), r.data.size(), hipMemcpyDeviceToHost);
        }
        return e;
    }
    bool write() const                                     // stops at the first file that could not be written
    {
        for (const Row& r : rows_)
            if (!r.path.empty() && !save(r.kind, r.path, w_, h_, r.data.data())) return false;
        return true;
    }

  private:
    struct Row { FileKind kind; std::string path; size_t part; std::vector<uint8_t> data; };
    size_t bytes(FileKind kind) const { return bytes_per_pixel(kind) * (size_t)w_ * (size_t)h_; }
    DeviceArena& arena_;
    const int w_, h_;
    std::vector<Row> rows_;
};
