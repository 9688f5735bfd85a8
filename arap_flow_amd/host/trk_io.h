// trk_io.h -- track files (DESIGN.md "Point tracks"), the twin of arap_flow_amd/trk.py.  Little-endian: the bytes "ATRK",
// int32 version = 1, W, H, F, P, then float32 pos[F][P][2], then uint8 occ[F][P] (255 = hidden in that frame).  Frame 0
// of a written track file holds the query points themselves; a points file is the same format with F = 1.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace arapio {

static const char TRK_TAG_STRING[] = "ATRK";
static const int32_t TRK_VERSION = 1;

struct Tracks {
    int32_t w = 0, h = 0, frames = 0, points = 0;
    std::vector<float> pos;                // [F][P][2]
    std::vector<uint8_t> occ;              // [F][P]
};

inline bool write_trk(const std::string& path, const Tracks& t)
{
    const size_t n = (size_t)t.frames * (size_t)t.points;
    FILE* stream = fopen(path.c_str(), "wb");
    if (!stream) { printf("WriteTrackFile(%s): could not open\n", path.c_str()); return false; }
    const int32_t head[5] = {TRK_VERSION, t.w, t.h, t.frames, t.points};
    bool ok = t.pos.size() == 2 * n && t.occ.size() == n && fwrite(TRK_TAG_STRING, 1, 4, stream) == 4 &&
              fwrite(head, sizeof(int32_t), 5, stream) == 5 && fwrite(t.pos.data(), sizeof(float), 2 * n, stream) == 2 * n &&
              fwrite(t.occ.data(), 1, n, stream) == n;
    ok = (fclose(stream) == 0) && ok;
    if (!ok) printf("WriteTrackFile(%s): problem writing\n", path.c_str());
    return ok;
}

inline bool read_trk(const std::string& path, Tracks& t)       // says why not
{
    FILE* stream = fopen(path.c_str(), "rb");
    if (!stream) { printf("ReadTrackFile: could not open %s\n", path.c_str()); return false; }
    char tag[4];
    int32_t head[5];
    if (fread(tag, 1, 4, stream) != 4 || fread(head, sizeof(int32_t), 5, stream) != 5) {
        printf("ReadTrackFile(%s): truncated track file (header)\n", path.c_str());
        fclose(stream);
        return false;
    }
    bool ok = true;
    if (memcmp(tag, TRK_TAG_STRING, 4) != 0) { printf("ReadTrackFile(%s): not a track file\n", path.c_str()); ok = false; }
    else if (head[0] != TRK_VERSION) { printf("ReadTrackFile(%s): track file version %d, %d expected\n", path.c_str(), head[0], TRK_VERSION); ok = false; }
    else if (head[1] < 1 || head[2] < 1 || head[3] < 1 || head[4] < 1) {
        printf("ReadTrackFile(%s): bad track file sizes W=%d H=%d F=%d P=%d\n", path.c_str(), head[1], head[2], head[3], head[4]);
        ok = false;
    }
    if (!ok) { fclose(stream); return false; }
    t.w = head[1]; t.h = head[2]; t.frames = head[3]; t.points = head[4];
    const size_t n = (size_t)t.frames * (size_t)t.points;
    t.pos.resize(2 * n);
    t.occ.resize(n);
    if (fread(t.pos.data(), sizeof(float), 2 * n, stream) != 2 * n || fread(t.occ.data(), 1, n, stream) != n) {
        printf("ReadTrackFile(%s): truncated track file\n", path.c_str());
        ok = false;
    } else if (fgetc(stream) != EOF) {
        printf("ReadTrackFile(%s): mis-sized track file, it is too long\n", path.c_str());
        ok = false;
    }
    fclose(stream);
    return ok;
}

}  // namespace arapio
