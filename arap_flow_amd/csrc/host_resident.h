// host_resident.h -- host side of the resident PCG path (arap_resident.h): the kernel table, the plan's resident
// resources, the work lists of a frame (32x8 tiles for the resident kernel, 64x4 tiles for the list launches), the deal
// of a batch's solves to launches and workgroups, and what happens when a launch gives up (failure + back-off).
#pragma once

// The resident kernel is instantiated per number of tile slots its loops run over (arap_resident.h): a launch takes
// the instantiation for the most tiles any of its workgroups holds -- and per group-sum flavour (RES_SUMS_*): the one
// that carries only the flat sum when every group dealt to the launch has <= 64 workgroups (resident_launch_sums).
typedef void (*ResidentKernel)(PlanDev, ResDev, int);
template <bool STAMPS, int SUMS, int... NS>
static const void* resident_kernel_of(int ns, std::integer_sequence<int, NS...>)
{
    static const ResidentKernel table[] = {k_pcg_resident<STAMPS, NS + 1, SUMS>...};
    return (const void*)table[ns - 1];
}
static const void* resident_kernel(bool stamps, int ns, int sums)
{
    if (ns < 1) ns = 1;
    if (ns > RES_SLOTS) ns = RES_SLOTS;
    const auto slots = std::make_integer_sequence<int, RES_SLOTS>();
    if (sums == RES_SUMS_FLAT)
        return stamps ? resident_kernel_of<true, RES_SUMS_FLAT>(ns, slots) : resident_kernel_of<false, RES_SUMS_FLAT>(ns, slots);
    return stamps ? resident_kernel_of<true, RES_SUMS_ANY>(ns, slots) : resident_kernel_of<false, RES_SUMS_ANY>(ns, slots);
}
static const char* resident_sums_name(int sums) { return sums == RES_SUMS_FLAT ? "flat" : "any"; }

// resident-path resources: active-tile lists, granules, error word
static void plan_enable_resident(Opt_Plan* p)
{
    Opt_State* st = p->st;
    const Knobs knobs = read_knobs();
    p->knob_res_groups = knobs.res_groups;
    p->knob_res_ns = knobs.res_ns;
    p->knob_res_sums_any = knobs.res_sums_any;
    if (knobs.no_resident) return;
    hipDeviceProp_t prop;
    HC(hipGetDeviceProperties(&prop, st->device));
    if (prop.multiProcessorCount * 2 < RES_WGS) return;        // two resident workgroups per CU
    for (int sums = 0; sums < RES_SUMS_COUNT; ++sums)
        for (int ns = 1; ns <= RES_SLOTS; ++ns) {
            const void* kern = resident_kernel(false, ns, sums);
            if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, RES_LDS_BYTES) != hipSuccess) {
                (void)hipGetLastError();
                return;
            }
            int occ = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, RES_THREADS, RES_LDS_BYTES) != hipSuccess || occ < 2) {
                (void)hipGetLastError();
                return;
            }
        }
    const size_t B = (size_t)p->batch;
    const size_t sz_map = align_up(B * RES_WGS * sizeof(ResWg), 256);
    p->rd.rtX = (p->W + RT_X - 1) / RT_X;
    p->rd.rtY = (p->H + RT_Y - 1) / RT_Y;
    {
        // border z of every tile (arap_resident.h: ResDev::zx)
        const size_t nz = B * RES_MAX_TILES * RES_ZG * sizeof(unsigned long long);
        HC(hipMalloc((void**)&p->rd.zx, nz));
        HC(hipMemsetAsync(p->rd.zx, 0, nz, st->stream));
    }
    HC(hipHostMalloc((void**)&p->pin_wgmap, sz_map, hipHostMallocDefault));
    p->res_block = device_block(st, true, [&](Carver& part) {
        part(p->rd.gran, B * RES_GRAN_PER_LAUNCH * 8);                   // one block per launch of a step
        part(p->rd.tilelist, B * RES_MAX_TILES * sizeof(int));
        part(p->rd.ntiles, B * sizeof(int));
        part(p->rd.err, sizeof(unsigned));
        part(p->d_wgmap, sz_map);
        part(p->rd.tilepos, B * p->rd.rtX * p->rd.rtY * sizeof(int));
        part(p->rd.bandx0, B * p->rd.rtY * sizeof(int));
        part(p->d_resact, (size_t)p->rd.rtX * p->rd.rtY);                // drop-in analysis: tile activity
    });
    p->pd.res_err = p->rd.err;
    p->rd.stamps = nullptr;
    p->rd.force_fail = knobs.force_res_fail == 1 ? 1 : 0;   // test hook
    // 2: ONE real timeout -- the first table upload of this plan leaves a workgroup of the first group out, so the
    // rest of that group spins in its first group wait until the bounded spin gives up (arap_resident.h: group_sum)
    p->hole_pending = knobs.force_res_fail == 2;
    p->rd.allow_fast = knobs.no_xcd_fast ? 0 : 1;
    p->rd.flat_runs = knobs.flat_runs;
    p->rd.nowait = knobs.res_nowait ? 1 : 0;
    if (knobs.stamps) {
        for (int sums = 0; sums < RES_SUMS_COUNT; ++sums)
            for (int ns = 1; ns <= RES_SLOTS; ++ns)
                HC(hipFuncSetAttribute(resident_kernel(true, ns, sums), hipFuncAttributeMaxDynamicSharedMemorySize, RES_LDS_BYTES));
        HC(hipMalloc(&p->rd.stamps, 2 * RES_WGS * 16 * sizeof(unsigned long long)));     // two tables (arap_resident.h)
        HC(hipMemset(p->rd.stamps, 0, 2 * RES_WGS * 16 * sizeof(unsigned long long)));
    }
    p->res_capable = true;
}

// The resident kernel's work list of one solve (arap_resident.h): 32 x 8 tiles in bands of 8 rows; within a band the
// tiles start at `bandx0` (the band's first active x when `aligned`, else 0) and follow each other every 32 columns;
// tiles without an active vertex are left out.  `tiles` receives the origins (x0 + W y0) band by band.
static void build_resident_tiles(const uint8_t* mask_red, int W, int H, bool aligned, std::vector<int>& tiles,
                                 std::vector<int>& bandx0, uint64_t* nactive)
{
    const int rtY = (H + RT_Y - 1) / RT_Y;
    tiles.clear();
    bandx0.assign(rtY, 0);
    std::vector<uint8_t> col(W);
    uint64_t na = 0;
    for (int band = 0; band < rtY; ++band) {
        std::fill(col.begin(), col.end(), 0);
        const int y0 = band * RT_Y, y1 = std::min(H, y0 + RT_Y);
        for (int y = y0; y < y1; ++y) {
            const uint8_t* row = mask_red + (size_t)W * y;
            for (int x = 0; x < W; ++x) {
                const uint8_t a = row[x] == 0;
                col[x] |= a;
                na += a;
            }
        }
        int xmin = 0, xmax = -1;
        for (int x = 0; x < W; ++x)
            if (col[x]) { if (xmax < 0) xmin = x; xmax = x; }
        if (xmax < 0) continue;
        const int xs = aligned ? xmin : 0;
        bandx0[band] = xs;
        for (int x0 = xs; x0 <= xmax; x0 += RT_X) {
            bool any = false;
            for (int x = x0; x < W && x < x0 + RT_X && !any; ++x) any = col[x] != 0;
            if (any) tiles.push_back(x0 + W * y0);
        }
    }
    if (nactive) *nactive = na;
}

// A frame's active 64x4 tiles (indices ty * tX + tx, row-major) for the list launches of k_gn_prep / k_gn_init /
// k_gn_update.
static void build_t64_list(const uint8_t* mask_red, int W, int H, int tX, int tY, std::vector<int>& l64)
{
    l64.clear();
    for (int ty = 0; ty < tY; ++ty)
        for (int tx = 0; tx < tX; ++tx) {
            bool any = false;
            for (int y = ty * TILE_Y; y < H && y < (ty + 1) * TILE_Y && !any; ++y) {
                const uint8_t* row = mask_red + (size_t)W * y;
                for (int x = tx * TILE_X; x < W && x < (tx + 1) * TILE_X; ++x)
                    if (row[x] == 0) { any = true; break; }
            }
            if (any) l64.push_back(ty * tX + tx);
        }
}

// Upload one slot's work list: origins, their count, the bands' first x and the inverse map (band, column) -> position.
// Enqueued on `cs` (the caller orders it before the kernels that read the lists and after those that still use the
// old ones).  The sources are plan-owned host vectors that live until the next upload of the slot.
static void plan_upload_tiles(Opt_Plan* p, int slot, const std::vector<int>& tiles, const std::vector<int>& bandx0,
                              hipStream_t cs)
{
    const int nt = (int)tiles.size();
    p->h_ntiles[slot] = nt;
    if (!p->res_capable) return;
    if (p->h_tiles_valid[slot] && p->h_tiles[slot] == tiles && p->h_bandx0[slot] == bandx0) return;   // already there
    p->h_tiles[slot] = tiles;
    p->h_bandx0[slot] = bandx0;
    p->h_tiles_valid[slot] = 1;
    const int rtX = p->rd.rtX, rtY = p->rd.rtY;
    if (nt <= RES_MAX_TILES) {
        std::vector<int>& pos = p->h_tilepos[slot];
        pos.assign((size_t)rtX * rtY, -1);
        for (int i = 0; i < nt; ++i) {
            const int y0 = tiles[i] / p->W, x0 = tiles[i] - y0 * p->W;
            const int band = y0 / RT_Y, k = (x0 - bandx0[band]) / RT_X;
            pos[(size_t)band * rtX + k] = i;
        }
        if (nt > 0)
            HC(hipMemcpyAsync((void*)(p->rd.tilelist + (size_t)slot * RES_MAX_TILES), p->h_tiles[slot].data(),
                              sizeof(int) * nt, hipMemcpyHostToDevice, cs));
        HC(hipMemcpyAsync((void*)(p->rd.tilepos + (size_t)slot * rtX * rtY), pos.data(), sizeof(int) * pos.size(),
                          hipMemcpyHostToDevice, cs));
        HC(hipMemcpyAsync((void*)(p->rd.bandx0 + (size_t)slot * rtY), p->h_bandx0[slot].data(), sizeof(int) * rtY,
                          hipMemcpyHostToDevice, cs));
    }
    HC(hipMemcpyAsync((void*)(p->rd.ntiles + slot), &p->h_ntiles[slot], sizeof(int), hipMemcpyHostToDevice, cs));
}

// Opt_ProblemInit and every Opt_ProblemStep of a drop-in plan: look at the caller's Mask and UrShape (one small
// kernel + a read-back of one byte per tile; the reference's init and step block on a device read-back too,
// solverGPUGaussNewton.t:1006,1117,790-797) to decide whether the step can take the resident kernel and with which
// active-tile list.  The reference re-reads every parameter at every Step (:960,1026) and lets the caller change
// them in between (Opt.h:58-66): so does this -- new Mask / UrShape contents or swapped buffers are seen here.
static void plan_analyse_for_resident(Opt_Plan* p)
{
    p->opt_res_ok = false;
    if (p->res_frames) return;
    Opt_State* st = p->st;
    // without the resident resources there is still one use of the result: the share of active tiles steers the
    // automatic phase-A variant of the two-kernel path
    const int rtX = (p->W + RT_X - 1) / RT_X, rtY = (p->H + RT_Y - 1) / RT_Y;
    const int nt_all = rtX * rtY;
    if (!p->d_notgrid) HC(hipMalloc(&p->d_notgrid, sizeof(int) + (size_t)nt_all));
    uint8_t* d_act = p->d_resact ? p->d_resact : (uint8_t*)(p->d_notgrid + 1);
    HC(hipMemsetAsync(p->d_notgrid, 0, sizeof(int), st->stream));
    hipLaunchKernelGGL(k_analyse, dim3(rtX, rtY, 1), dim3(RT_X, RT_Y, 1), 0, st->stream, p->pd, d_act, p->d_notgrid);
    std::vector<uint8_t> act(nt_all);
    int notgrid = 1;
    HC(hipMemcpyAsync(act.data(), d_act, nt_all, hipMemcpyDeviceToHost, st->stream));
    HC(hipMemcpyAsync(&notgrid, p->d_notgrid, sizeof(int), hipMemcpyDeviceToHost, st->stream));
    HC(hipStreamSynchronize(st->stream));
    std::vector<int> tiles, bandx0(rtY, 0);                     // fixed grid: every band starts at x = 0
    for (int t = 0; t < nt_all; ++t)
        if (act[t]) tiles.push_back((t % rtX) * RT_X + p->W * ((t / rtX) * RT_Y));
    const int nt = (int)tiles.size();
    p->h_ntiles[0] = nt;
    p->res_tiles_all = nt_all;
    p->grid_u = notgrid == 0;
    if (notgrid || !p->res_capable || !st->use_resident || st->res_cooldown > 0 || nt > RES_MAX_TILES) return;
    plan_upload_tiles(p, 0, tiles, bandx0, st->stream);
    p->opt_res_ok = true;
    p->opt_res_slot = p->hslots[0];
}

static bool plan_resident_eligible(const Opt_Plan* p)
{
    if (!p->res_capable || !p->st->use_resident) return false;
    if (p->st->res_cooldown > 0) return false;          // pausing after a timed-out launch (plan_resident_failed)
    if (p->sp.lIterations > RES_MAX_L) return false;    // (the border-z granules carry 16-bit iteration tags)
    if (!p->res_frames) {
        // drop-in plan: only with the images analysed just before this step (plan_analyse_for_resident)
        const Slot& a = p->opt_res_slot;
        const Slot& c = p->hslots[0];
        if (!p->opt_res_ok || a.M != c.M || a.U != c.U) return false;
    }
    for (int b = 0; b < p->nb; ++b)
        if (p->h_ntiles[b] > RES_MAX_TILES) return false;
    return true;
}

// Deal the solves of the current batch to resident launches and their 512 workgroups (ResWg tables).
// A launch is 8 bins of 64 workgroups: the workgroups that land on one XCD (blockIdx & 7 equal, local index
// blockIdx >> 3).  A solve of nt active tiles needs ceil(nt / 9) workgroups.
//  * NARROW (needs <= 64): shares a bin with others: the narrow solves are bin-packed into as few launches as
//    first-fit-decreasing needs, spread evenly over the shared bins (least-loaded first), and every group is then
//    widened to use its bin's spare workgroups (fewer tiles per workgroup = shorter phases).  Groups of one bin take
//    consecutive local indices, so the two workgroups of a CU (j, j + 32) usually serve different solves.
//  * MEDIUM (65 .. 128: the 1920x1080 --multseg segments, ~716 tiles = 80 workgroups): a whole bin as HOME for ranks
//    0 .. 63 plus a PIECE of need - 64 workgroups (ranks 64 ..) in a bin it shares with other pieces and narrow solves,
//    widened like those.  Six such solves fit a launch (six homes, two shared bins) where whole pairs of bins held four.
//    Tiles are dealt in list (row-major) order, so nearly all of a workgroup's halo neighbours share its XCD; the
//    group's sums are gathered in one hop (arap_resident.h: group_sum_x, runs of 64 ranks).
//  * WIDE (> 128): 4 or 8 whole bins, aligned to the width; every bin holds a run of 64 consecutive ranks; sums in two
//    levels (group_sum_h).
// Placement is for speed only: the kernel checks at run time which runs really share an XCD.
// `forced` > 0 (Knobs::res_groups, experiments only): that many equal groups instead, where the solves fit them.
// Returns the number of launches; fills `map` ([launches][RES_WGS]) and `inflight_out` when given.
static int resident_deal(const int* ntiles, int nb, int forced, std::vector<ResWg>* map_out, int* inflight_out)
{
    const int XW = RES_WGS / 8;                                  // workgroups per XCD
    enum { NARROW = 0, MEDIUM = 1, WIDE = 2 };
    std::vector<int> need(nb), width(nb), kind(nb);
    int mx = 1;
    for (int b = 0; b < nb; ++b) {
        need[b] = (ntiles[b] + RES_TILES_PER_WG - 1) / RES_TILES_PER_WG;
        if (need[b] < 1) need[b] = 1;
        mx = need[b] > mx ? need[b] : mx;
        kind[b] = need[b] <= XW ? NARROW : (need[b] <= 2 * XW ? MEDIUM : WIDE);
        width[b] = 1;                                            // whole bins a WIDE solve takes: 4 or 8
        if (kind[b] == WIDE) { width[b] = 4; while (width[b] * XW < need[b]) width[b] *= 2; }
    }
    std::vector<ResWg> map;
    int nsets = 0, inflight = 0;
    const ResWg idle = {-1, 0, 0, 0};
    if (forced && forced <= RES_MAX_GROUPS && (RES_WGS / forced) >= mx && (RES_WGS % forced) == 0) {
        const int groups = forced, wgs = RES_WGS / groups;
        nsets = (nb + groups - 1) / groups;
        map.assign((size_t)nsets * RES_WGS, idle);
        for (int set = 0; set < nsets; ++set)
            for (int i = 0; i < RES_WGS; ++i) {
                int g, rank;
                const int x = i & 7, j = i >> 3;
                if (groups >= 8) { g = x + 8 * (j / wgs); rank = j % wgs; }
                else { const int xper = 8 / groups; g = x / xper; rank = (x % xper) * XW + j; }
                const int sb = set * groups + g;
                if (sb < nb) map[(size_t)set * RES_WGS + i] = ResWg{sb, rank, wgs, 2 * RES_GS * g * wgs};
            }
        inflight = nb < groups ? nb : groups;
    } else {
        std::vector<int> order(nb);
        for (int b = 0; b < nb; ++b) order[b] = b;
        std::stable_sort(order.begin(), order.end(), [&](int a, int c) {
            return kind[a] != kind[c] ? kind[a] > kind[c] : (width[a] != width[c] ? width[a] > width[c] : need[a] > need[c]);
        });
        // bin state over all launches.  owner >= 0: a wide solve, or a medium solve's home, holds the whole bin;
        // owner == -1: shared / free (load = workgroups spoken for)
        std::vector<int> owner, load;
        auto add_launch = [&]() { owner.insert(owner.end(), 8, -1); load.insert(load.end(), 8, 0); };
        // (1) wide solves: first launch with `width` aligned bins that nothing has touched yet
        for (int b : order) {
            if (kind[b] != WIDE) continue;
            size_t at = owner.size();
            for (size_t k = 0; k + width[b] <= owner.size() && at == owner.size(); k += width[b]) {
                bool free_run = true;
                for (int q = 0; q < width[b]; ++q) free_run = free_run && owner[k + q] < 0 && load[k + q] == 0;
                if (free_run) at = k;
            }
            if (at == owner.size()) add_launch();                // 8 is a multiple of every width: `at` is aligned
            for (int q = 0; q < width[b]; ++q) { owner[at + q] = b; load[at + q] = XW; }
        }
        // (2) medium solves: a free bin as home, the piece first-fit into a bin of the same launch that pieces already
        //     share (so that free bins stay available as homes), else into a free one
        std::vector<int> home(nb, -1);                           // medium: its home bin (global index)
        std::vector<int> ffbin(nb, -1);                          // first-fit bin of every shared item (piece or narrow solve)
        auto item_size = [&](int b) { return kind[b] == MEDIUM ? need[b] - XW : need[b]; };
        for (int b : order) {
            if (kind[b] != MEDIUM) continue;
            const int piece = item_size(b);
            int hb = -1, pb = -1;
            for (size_t L = 0; L * 8 < owner.size() && hb < 0; ++L) {
                int h = -1, pshared = -1, pfree = -1;
                for (int x = 0; x < 8; ++x) {
                    const size_t k = L * 8 + x;
                    if (owner[k] >= 0) continue;
                    if (load[k] == 0) { if (h < 0) h = (int)k; else if (pfree < 0) pfree = (int)k; }
                    else if (pshared < 0 && load[k] + piece <= XW) pshared = (int)k;
                }
                const int pk = pshared >= 0 ? pshared : pfree;
                if (h >= 0 && pk >= 0) { hb = h; pb = pk; }
            }
            if (hb < 0) { hb = (int)owner.size(); pb = hb + 1; add_launch(); }
            owner[hb] = b; load[hb] = XW; home[b] = hb;
            load[pb] += piece; ffbin[b] = pb;
        }
        // (3) narrow solves: number of launches by first fit decreasing over the shared bins ...
        for (int b : order) {
            if (kind[b] != NARROW) continue;
            size_t k = 0;
            while (k < owner.size() && (owner[k] >= 0 || load[k] + need[b] > XW)) ++k;
            if (k == owner.size()) add_launch();
            load[k] += need[b]; ffbin[b] = (int)k;
        }
        nsets = (int)owner.size() / 8;
        // ... then spread: pieces over the shared bins of their launch, narrow solves over all shared bins, least-loaded
        // bin that still fits first; keep the first-fit deal if that ever fails
        std::vector<int> bin_of(nb, -1), l2(owner.size(), 0);
        bool ok = true;
        for (int pass = 0; pass < 2 && ok; ++pass)
            for (int b : order) {
                if (kind[b] == WIDE || (pass == 0) != (kind[b] == MEDIUM)) continue;
                const int sz = item_size(b);
                const size_t lo = kind[b] == MEDIUM ? (size_t)(home[b] / 8) * 8 : 0;
                const size_t hi = kind[b] == MEDIUM ? lo + 8 : owner.size();
                int best = -1;
                for (size_t k = lo; k < hi; ++k)
                    if (owner[k] < 0 && l2[k] + sz <= XW && (best < 0 || l2[k] < l2[best])) best = (int)k;
                if (best < 0) { ok = false; break; }
                l2[best] += sz;
                bin_of[b] = best;
            }
        if (!ok) {
            bin_of = ffbin;
            std::fill(l2.begin(), l2.end(), 0);
            for (int b = 0; b < nb; ++b)
                if (kind[b] != WIDE) l2[bin_of[b]] += item_size(b);
        }
        // workgroups of every group: a shared item gets its bin's spare workgroups in proportion (>= its need)
        std::vector<int> wgs_of(nb, 0), part_w(nb, 0);
        for (int b = 0; b < nb; ++b) {
            if (kind[b] == WIDE) { wgs_of[b] = width[b] * XW; continue; }
            part_w[b] = XW * item_size(b) / l2[bin_of[b]];       // >= the item's size; a bin's parts sum to <= 64
            wgs_of[b] = kind[b] == MEDIUM ? XW + part_w[b] : part_w[b];
        }
        map.assign((size_t)nsets * RES_WGS, idle);
        std::vector<int> gran_of(nb, -1);
        for (int set = 0; set < nsets; ++set) {
            // granule space per group, in units of workgroups: a group of several runs addresses its runs in blocks of 64
            int ordinal = 0, count = 0;
            auto take_gran = [&](int b) {
                if (gran_of[b] >= 0) return;
                gran_of[b] = 2 * RES_GS * ordinal;
                ordinal += wgs_of[b] > XW ? ((wgs_of[b] + XW - 1) / XW) * XW : wgs_of[b];
                ++count;
            };
            for (int x = 0; x < 8; ++x) {
                const size_t k = (size_t)set * 8 + x;
                if (owner[k] >= 0) {
                    const int b = owner[k];
                    take_gran(b);
                    if (kind[b] == MEDIUM) {                     // home: ranks 0 .. 63
                        for (int j = 0; j < XW; ++j)
                            map[(size_t)set * RES_WGS + (size_t)j * 8 + x] = ResWg{b, j, wgs_of[b], gran_of[b]};
                        continue;
                    }
                    const bool first = x == 0 || owner[k - 1] != b;
                    if (!first) continue;                        // dealt with its first bin
                    for (int q = 0; q < width[b]; ++q)
                        for (int j = 0; j < XW; ++j)
                            map[(size_t)set * RES_WGS + (size_t)j * 8 + x + q] = ResWg{b, q * XW + j, wgs_of[b], gran_of[b]};
                    continue;
                }
                int j = 0;
                for (int b : order) {                            // the bin's items, largest first
                    if (kind[b] == WIDE || bin_of[b] != (int)k) continue;
                    take_gran(b);
                    const int r0 = kind[b] == MEDIUM ? XW : 0;
                    for (int r = 0; r < part_w[b]; ++r, ++j)
                        map[(size_t)set * RES_WGS + (size_t)j * 8 + x] = ResWg{b, r0 + r, wgs_of[b], gran_of[b]};
                }
            }
            inflight = count > inflight ? count : inflight;
        }
    }
    if (map_out) map_out->swap(map);
    if (inflight_out) *inflight_out = inflight;
    return nsets;
}

// The group-sum flavour of one launch, from its table: the flat-only kernel exactly when every group dealt to it has
// <= 64 workgroups (the kernel would take group_sum for all of them anyway), else the kernel that carries all three.
// This is an invariant the flat kernel relies on, not only a choice of speed: its sweep is one trip, lane k reads rank
// k's granules, and it never looks at a rank beyond 63 (arap_resident.h: group_sum<true>; checked in plan_resident_pack).
static int resident_launch_sums(const ResWg* map, bool force_any)
{
    if (force_any) return RES_SUMS_ANY;
    for (int i = 0; i < RES_WGS; ++i)
        if (map[i].slot >= 0 && map[i].wgs > RES_WGS / 8) return RES_SUMS_ANY;
    return RES_SUMS_FLAT;
}

// Deal the current batch; true if the tables changed (the caller re-uploads them: plan_upload_wgmap).
static bool plan_resident_pack(Opt_Plan* p)
{
    std::vector<ResWg> map;
    const int nsets = resident_deal(p->h_ntiles.data(), p->nb, p->knob_res_groups, &map, &p->res_inflight);
    std::vector<int> ns(nsets, 1);
    for (size_t i = 0; i < map.size(); ++i)
        if (map[i].slot >= 0) {
            const int t = (p->h_ntiles[map[i].slot] + map[i].wgs - 1) / map[i].wgs;      // tiles of the group's fullest workgroup
            int& m = ns[i / RES_WGS];
            m = t > m ? t : m;
        }
    if (p->knob_res_ns > 0)                                      // experiments: run at least this many tile slots
        for (int& m : ns) m = std::max(m, std::min(p->knob_res_ns, (int)RES_SLOTS));
    std::vector<int> sums(nsets, RES_SUMS_ANY);
    for (int set = 0; set < nsets; ++set)
        sums[set] = resident_launch_sums(map.data() + (size_t)set * RES_WGS, p->knob_res_sums_any);
    for (size_t i = 0; i < map.size(); ++i)
        if (map[i].slot >= 0 && sums[i / RES_WGS] == RES_SUMS_FLAT && map[i].wgs > 64) {
            fprintf(stderr, "arapopt: a group of %d workgroups was dealt to a launch of the flat group-sum flavour, "
                            "whose one-trip sweep covers 64\n", map[i].wgs);
            exit(3);
        }
    const bool same = nsets == p->res_sets && ns == p->res_ns && sums == p->res_sums && map.size() == p->h_wgmap.size() &&
                      memcmp(map.data(), p->h_wgmap.data(), map.size() * sizeof(ResWg)) == 0;
    if (same) return false;
    p->h_wgmap.swap(map);
    p->res_ns.swap(ns);
    p->res_sums.swap(sums);
    p->res_sets = nsets;
    return true;
}

// A new deal of solves to workgroups (the frames' active-tile counts changed): upload the tables, stream ordered
// behind earlier launches.  (The captured launches bake in only the number of launches, their slot counts and the list
// length, and through the kernel function the group-sum flavour -- all in the StepRecipe -- so a new deal of the same shape replays the old graph.)
static void plan_upload_wgmap(Opt_Plan* p)
{
    Opt_State* st = p->st;
    if (p->hole_pending) {
        std::vector<ResWg> holed = p->h_wgmap;
        for (ResWg& w : holed)
            if (w.slot >= 0 && w.wgs > 1 && w.rank == w.wgs - 1) { w = ResWg{-1, 0, 0, 0}; break; }
        HC(hipStreamSynchronize(st->stream));
        HC(hipMemcpy(p->d_wgmap, holed.data(), holed.size() * sizeof(ResWg), hipMemcpyHostToDevice));
        p->hole_pending = false;
    } else {
        // (from pinned staging: a pageable source makes the call wait until the stream has drained -- i.e. for the
        //  other solver object's whole solve.  The staging buffer is rewritten only by this plan's next deal, which
        //  comes after this solve has been waited for.)
        memcpy(p->pin_wgmap, p->h_wgmap.data(), p->h_wgmap.size() * sizeof(ResWg));
        HC(hipMemcpyAsync(p->d_wgmap, p->pin_wgmap, p->h_wgmap.size() * sizeof(ResWg), hipMemcpyHostToDevice,
                          st->stream));
    }
}

// Did a resident launch of this plan give up (a bounded group wait timed out: its 512 workgroups were not all
// resident, e.g. because another process uses the GPU)?  Then the step's update was skipped on the device
// (k_gn_update), the error word is cleared, the resident path is switched off for this state and the caller redoes
// the work on the two-kernel path.  Requires a synchronised stream.
static bool plan_resident_failed(Opt_Plan* p)
{
    if (!p->res_capable || p->res_launches == 0) return false;
    unsigned e = 0;
    HC(hipMemcpyAsync(&e, p->rd.err, sizeof(e), hipMemcpyDeviceToHost, p->st->stream));
    HC(hipStreamSynchronize(p->st->stream));
    if (e == 0) return false;
    Opt_State* st = p->st;
    fprintf(stderr, "arapopt: resident PCG kernel gave up at a group wait (code 0x%08x); is the GPU shared? "
                    "Falling back to the two-kernel path for the next %d solve calls.\n", e, st->res_backoff);
    st->resident_failed = true;
    st->res_cooldown = st->res_backoff;
    st->res_backoff = st->res_backoff >= 1024 ? 1024 : 2 * st->res_backoff;
    HC(hipMemsetAsync((void*)p->rd.err, 0, sizeof(unsigned), st->stream));
    HC(hipStreamSynchronize(st->stream));
    p->h_wgmap.clear();                     // (the test hook's table with a hole must not survive: re-deal next time)
    p->res_sets = 0;
    return true;
}

static void plan_check_resident_error(Opt_Plan* p)
{
    if (plan_resident_failed(p)) {        // reached only if a caller consumed results without the checks below
        fprintf(stderr, "arapopt: resident PCG failure detected after results were consumed\n");
        exit(3);
    }
}
