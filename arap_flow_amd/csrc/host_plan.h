// host_plan.h -- what every host file builds on: the HIP error check, the per-kernel timer, the run-time knobs, the
// state / plan objects with their creation, buffer reservation, slot upload and release, and the timed-launch macro.
#pragma once

// Device API failure -> message + exit, as the reference does (solverGPUGaussNewton.t:59-73).
static void hip_fatal(hipError_t e, const char* what, const char* file, int line)
{
    fprintf(stderr, "arapopt: HIP error %d (%s) in %s at %s:%d\n", (int)e, hipGetErrorString(e), what, file, line);
    exit((int)e ? (int)e : 1);
}
#define HC(call)                                                     \
    do {                                                             \
        hipError_t e_ = (call);                                      \
        if (e_ != hipSuccess) hip_fatal(e_, #call, __FILE__, __LINE__); \
    } while (0)

// ---------------------------------------------------------------------------------------------
struct KernelTimer {            // collectPerKernelTimingInfo (Opt.h:23-25, util.t:414-511)
    struct Rec { std::string name; hipEvent_t a, b; };
    std::vector<Rec> recs;
    void clear()
    {
        for (auto& r : recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
        recs.clear();
    }
    void report()
    {
        std::map<std::string, std::pair<int, double>> agg;
        for (auto& r : recs) {
            float ms = 0.f;
            (void)hipEventSynchronize(r.b);
            (void)hipEventElapsedTime(&ms, r.a, r.b);
            agg[r.name].first++;
            agg[r.name].second += ms;
        }
        printf("--------------------------------------------------------\n");
        printf("        Kernel        |   Count  |   Total   | Average \n");
        printf("----------------------+----------+-----------+----------\n");
        for (auto& kv : agg)
            printf(" %-20s |   %4d   | %8.3fms| %7.4fms\n", kv.first.c_str(), kv.second.first,
                   kv.second.second, kv.second.second / kv.second.first);
        printf("--------------------------------------------------------\n");
        clear();
    }
};

// phase A of the two-kernel path: direct-load kernel or an LDS-staged tile shape (ArapFlow_SetTile)
static const int kTileShapes[6][2] = {{0, 0}, {16, 16}, {32, 8}, {64, 4}, {32, 16}, {64, 8}};
static int tile_shape_index(int tx, int ty)
{
    for (int v = 0; v < 6; ++v)
        if (kTileShapes[v][0] == tx && kTileShapes[v][1] == ty) return v;
    return -1;
}

// Every ARAPOPT_* run-time knob, read in one place.  read_knobs() is called when a state is created
// (Opt_NewState takes the state-level knobs from it) and when a plan is created (plan_enable_resident takes the
// plan-level ones); ArapFlow_ResidentDeal, which has no plan, takes res_groups per call.  Nothing else reads the
// environment.
struct Knobs {
    // state level
    bool no_graph = false;      // ARAPOPT_NO_GRAPH=1: launch a step's kernels one by one
    int tile = -1;              // ARAPOPT_TILE=TXxTY: index into kTileShapes, -1 = not given / no such shape
    bool b8 = false;            // ARAPOPT_B8=1: the 8-byte-per-lane form of phase B
    int stream_a = 0;           // ARAPOPT_STREAM_A
    bool mscore_plain = false;  // ARAPOPT_MSCORE_PLAIN=1 (experiments: k_mscore_hist with one LDS atomic per pixel, no wave aggregation)
    bool aug_bytes = false;     // ARAPOPT_AUG_BYTES=1 (experiments: k_augment reads a tap's three bytes one by one, not as one dword)
    // plan level
    bool no_resident = false;   // ARAPOPT_NO_RESIDENT=1
    int force_res_fail = 0;     // ARAPOPT_FORCE_RES_FAIL=1 / 2 (test hooks)
    bool no_xcd_fast = false;   // ARAPOPT_NO_XCD_FAST=1
    int flat_runs = RES_FLAT_MAX_RUNS;   // ARAPOPT_FLAT_RUNS=n (experiments: 0 = always two levels, 4 / 8 = wider one-hop sums)
    bool res_nowait = false;    // ARAPOPT_RES_NOWAIT=1 (diagnostic: iteration time without the group waits)
    bool stamps = false;        // ARAPOPT_STAMPS=1: diagnostic build of the resident kernel (tools/res_stamps.py)
    int res_groups = 0;         // ARAPOPT_RES_GROUPS=n (experiments only: n equal groups), 0 = the packed deal
    int res_ns = 0;             // ARAPOPT_RES_NS=n (experiments: run at least this many tile slots), 0 = as dealt
    bool res_sums_any = false;  // ARAPOPT_RES_SUMS=any (tests, A/B): every launch takes the kernel that carries all group-sum flavours
};

static Knobs read_knobs()
{
    auto is = [](const char* name, char c) { const char* v = getenv(name); return v && v[0] == c; };
    auto num = [](const char* name, int absent) { const char* v = getenv(name); return v ? atoi(v) : absent; };
    Knobs k;
    k.no_graph = is("ARAPOPT_NO_GRAPH", '1');
    if (const char* tv = getenv("ARAPOPT_TILE")) {                     // "TXxTY" or "0x0"
        int tx = -1, ty = -1;
        if (sscanf(tv, "%dx%d", &tx, &ty) == 2) k.tile = tile_shape_index(tx, ty);
    }
    k.b8 = is("ARAPOPT_B8", '1');
    k.stream_a = num("ARAPOPT_STREAM_A", 0);
    k.mscore_plain = is("ARAPOPT_MSCORE_PLAIN", '1');
    k.aug_bytes = is("ARAPOPT_AUG_BYTES", '1');
    k.no_resident = is("ARAPOPT_NO_RESIDENT", '1');
    k.force_res_fail = is("ARAPOPT_FORCE_RES_FAIL", '1') ? 1 : (is("ARAPOPT_FORCE_RES_FAIL", '2') ? 2 : 0);
    k.no_xcd_fast = is("ARAPOPT_NO_XCD_FAST", '1');
    k.flat_runs = num("ARAPOPT_FLAT_RUNS", RES_FLAT_MAX_RUNS);
    k.res_nowait = is("ARAPOPT_RES_NOWAIT", '1');
    k.stamps = is("ARAPOPT_STAMPS", '1');
    k.res_groups = std::max(0, num("ARAPOPT_RES_GROUPS", 0));
    k.res_ns = std::max(0, num("ARAPOPT_RES_NS", 0));
    k.res_sums_any = is("ARAPOPT_RES_SUMS", 'a');
    return k;
}

struct Opt_State {
    int verbosity = 0;
    int timing = 0;
    int device = 0;
    hipStream_t stream = nullptr;     // where all work is enqueued (NULL = null stream)
    hipStream_t cap = nullptr;        // private stream used only for graph capture
    hipStream_t own_stream = nullptr; // ArapFlow_UseOwnStream
    hipEvent_t t0 = nullptr, t1 = nullptr;
    KernelTimer ktimer;
    bool use_graph = true;
    bool use_resident = true;   // ArapFlow_SetResident
    bool resident_failed = false;   // a resident launch has timed out at least once (GPU shared with another process?)
    // After a timeout the resident path pauses for `res_cooldown` solve calls (ArapFlow_SolverSolve / Opt_ProblemInit),
    // then it is tried again; every further timeout doubles the pause (8, 16, ... 1024), a checked success resets it.
    int res_cooldown = 0, res_backoff = 8;
    int tile = -1;              // ArapFlow_SetTile: phase-A variant of the two-kernel path; -1 = choose per solve
    bool force_b8 = false;      // ARAPOPT_B8=1 (counter calibration): the 8-byte-per-lane form of phase B
    int stream_a = 0;           // ARAPOPT_STREAM_A=1 (experiments): the tiled k_pcg_a_grid instead of the marching kernel
    bool mscore_plain = false;  // ARAPOPT_MSCORE_PLAIN=1 (experiments): k_mscore_hist without the wave aggregation
    void* diag = nullptr;       // ArapFlow_WarpDiag: device, the call's WarpJob (256 bytes) and its accumulator; at first use
    void* tex = nullptr;        // ArapFlow_Texture: device, the call's layer table (255 layers); at first use
    void* light = nullptr;      // ArapFlow_Relight: device, the call's tone table (3 x 256 bytes); at first use
    void* aug = nullptr;        // ArapFlow_AugmentPairs: device, the call's sample table (aug_cap samples); at first use, grown with B
    unsigned aug_cap = 0;
    void* clip = nullptr;       // ArapFlow_AugmentClips: device, the call's frame table (clip_cap frames) and link table; at first use, grown with B * T
    unsigned clip_cap = 0;
    bool aug_bytes = false;     // ARAPOPT_AUG_BYTES=1 (experiments): k_augment and k_augment_clip without the dword loads of the taps
};

struct Opt_Problem {
    int kind;    // 0 = gaussNewtonGPU, 1 = LMGPU
};

// solver parameter table and defaults: solverGPUGaussNewton.t:26-39, :148-163
struct SolverParameters {
    int residual_reset_period = 10;
    float min_relative_decrease = 1e-3f, min_trust_region_radius = 1e-32f, max_trust_region_radius = 1e16f,
          q_tolerance = 1e-4f, function_tolerance = 1e-6f, trust_region_radius = 1e4f,
          radius_decrease_factor = 2.0f, min_lm_diagonal = 1e-6f, max_lm_diagonal = 1e32f;
    int nIterations = 10, lIterations = 10;
    int nIter = 0;
};

// What one call of plan_gn_step launches, decided in one place (host_step.h: plan_step_recipe).  The enqueue code
// reads nothing but this and the plan's buffers, and the captured graph is replayed while the recipe stays equal to
// the one it was captured with.  Canonical: a field the chosen path does not read is zero (lag: -1).
enum { GN_STEP_ALL = 0, GN_STEP_PREP = 1, GN_STEP_FUSED = 2 };
enum PhaseA { PA_NONE = 0, PA_DIRECT, PA_LDS_16x16, PA_LDS_32x8, PA_LDS_64x4, PA_LDS_32x16, PA_LDS_64x8,   // PA_DIRECT + kTileShapes index
              PA_MARCH, PA_MARCH2, PA_GRID };
enum PhaseB { PB_NONE = 0, PB_B, PB_B4, PB_B4_LEAN, PB_B4_R };
struct StepRecipe {
    bool resident = false;          // all PCG iterations in resident launches / a kernel per phase
    int part = GN_STEP_ALL;         // GN_STEP_ALL or GN_STEP_FUSED
    int L = -1, nb = 0, nsteps = 0; // lIterations, active slots, Gauss-Newton steps in one graph
    // resident path
    std::vector<int> res_ns;        // per launch of a step: the kernel instantiation (tile slots)
    std::vector<int> res_sums;      // ... and its group-sum flavour (RES_SUMS_*): the kernel function is baked into the graph node
    bool stamped = false;           // ... of the instrumented build
    int list_blocks = 0;            // > 0: the per-step kernels run over the frames' 64x4 tile lists, with this grid.x
    // kernel-per-phase path
    int a_kern = PA_NONE, b_kern = PB_NONE;
    dim3 a_grid{0, 0, 0}, a_block{0, 0, 0};
    int a_arg[3] = {0, 0, 0};       // march / grid kernels: strips or tiles in x, in y, blocks per XCD chunk
    int lag = -1;                   // iteration whose delta update is left to k_gn_update (lean streaming schedule)
};
// every field
static bool same_recipe(const StepRecipe& a, const StepRecipe& b)
{
    auto same3 = [](dim3 x, dim3 y) { return x.x == y.x && x.y == y.y && x.z == y.z; };
    return a.resident == b.resident && a.part == b.part && a.L == b.L && a.nb == b.nb && a.nsteps == b.nsteps &&
           a.res_ns == b.res_ns && a.res_sums == b.res_sums && a.stamped == b.stamped && a.list_blocks == b.list_blocks && a.a_kern == b.a_kern &&
           a.b_kern == b.b_kern && same3(a.a_grid, b.a_grid) && same3(a.a_block, b.a_block) &&
           std::equal(a.a_arg, a.a_arg + 3, b.a_arg) && a.lag == b.lag;
}

struct Opt_Plan {
    Opt_State* st = nullptr;
    int W = 0, H = 0, N = 0, batch = 1;
    PlanDev pd{};
    SolverParameters sp;
    std::vector<Slot> hslots;       // host mirror of pd.slots
    std::vector<Slot> uploaded;
    void* block = nullptr;          // all plan-owned images
    int lcap = 0;                   // lIterations capacity of pd.red
    int ccap = 0;                   // cost entries capacity of pd.costred
    int nb = 1;                     // slots active in the current solve (grid.z)
    // captured graph of the Gauss-Newton step(s) last launched, and the recipe it was captured with (host_step.h)
    hipGraphExec_t gexec = nullptr;
    hipGraph_t graph = nullptr;
    StepRecipe g_recipe;
    // resident PCG (arap_resident.h): only for the frame solver (pixel-grid UrShape, host-known masks)
    bool res_capable = false;       // device has 256 CUs and the kernel fits one workgroup per CU
    bool res_frames = false;        // plan is driven by ArapFlow_Solver (and the resident resources exist)
    bool res_frames_any = false;    // plan is driven by ArapFlow_Solver, whatever the device
    bool grid_u = false;            // UrShape is the pixel grid on every active vertex (frame solver: always; drop-in:
                                    // what the last analysis found): the streaming phase A without UrShape loads applies
    // ArapFlow_Solver reports one cost, the one after the last step of the last ramp iteration: the costs the
    // reference evaluates at Init and after every step (for its log) are skipped unless cost_wanted
    bool lazy_cost = false, cost_wanted = true;
    ResDev rd{};
    void* res_block = nullptr;
    std::vector<int> h_ntiles;
    std::vector<std::vector<int>> h_tiles;   // what rd.tilelist holds per slot (skip the upload when nothing changed)
    std::vector<uint8_t> h_tiles_valid;
    std::vector<std::vector<int>> h_tilepos, h_bandx0;
    uint8_t* d_resact = nullptr;    // [rtX * rtY] drop-in analysis: 32x8 tiles (fixed grid) that hold an active vertex
    // frame solver: every slot's active 64x4 tiles, for the list launches of k_gn_prep / k_gn_init / k_gn_update
    int* d_t64list = nullptr;       // [batch][tilesX * tilesY]
    int* d_t64n = nullptr;          // [batch]
    std::vector<std::vector<int>> h_t64;
    std::vector<int> h_t64n;
    int res_tiles_all = 0;          // 32x8 tiles of the whole grid (share of active tiles: plan_active_tiles_majority)
    bool hole_pending = false;      // test hook ARAPOPT_FORCE_RES_FAIL=2: the next table upload leaves one workgroup out
    ResWg* d_wgmap = nullptr;       // [batch][RES_WGS]: one table per resident launch of a GN step
    ResWg* pin_wgmap = nullptr;     // pinned staging of the same size
    std::vector<ResWg> h_wgmap;     // what d_wgmap holds
    int res_sets = 0;               // resident launches per GN step
    std::vector<int> res_ns;        // per launch: tile slots in use = most tiles any of its workgroups holds
    std::vector<int> res_sums;      // per launch: group-sum flavour (RES_SUMS_FLAT when all its groups have <= 64 workgroups)
    int knob_res_groups = 0, knob_res_ns = 0;   // Knobs::res_groups / res_ns as of this plan's creation
    bool knob_res_sums_any = false; // Knobs::res_sums_any
    int res_inflight = 0;           // solves of the fullest launch (diagnostic)
    unsigned res_launches = 0;
    // drop-in (Opt_*) plans: result of the Init-time analysis (k_analyse) of the caller's Mask / UrShape
    bool opt_res_ok = false;
    bool prep_done = false;         // the last enqueued step left flags and cos/sin ready for the next (resident launch with fuse_update)
    Slot opt_res_slot{};
    int* d_notgrid = nullptr;
    // "LMGPU" plans
    int kind = 0;
    void* lm_block = nullptr;       // b, CtC, SSq, Adelta, prevX
    float2* prevO = nullptr;
    float* prevA = nullptr;
    int lm_lcap = 0;
    float lm_radius = 0.f, lm_decrease = 0.f;      // pd.parameters.trust_region_radius / radius_decrease_factor
    double lm_prev_cost = 0.0;
    bool lm_done = false;
    int lm_last_pcg = 0, lm_last_outcome = -1;     // of the last step attempted since Init (ArapFlow_LMState)

    dim3 grid() const { return dim3(pd.tilesX, pd.tilesY, nb); }
    dim3 blk() const { return dim3(TILE_X, TILE_Y, 1); }
};

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// the argument checks the scoring and map calls share.  buffers_overlap: of a table {pointer, bytes} with the outputs
// first, does any of the first `outs` overlap a later one?  A null pointer is a buffer not given.  sizes_ok: n maps of
// W x H pixels that 31-bit indices address, one map and all together
static bool buffers_overlap(const std::pair<const void*, uint64_t>* bufs, int outs, int count)
{
    for (int o = 0; o < outs; ++o)
        for (int k = o + 1; k < count; ++k) {
            const uintptr_t a = (uintptr_t)bufs[o].first, b = (uintptr_t)bufs[k].first;
            if (a && b && a < b + bufs[k].second && b < a + bufs[o].second) return true;
        }
    return false;
}
static bool sizes_ok(unsigned W, unsigned H, unsigned n)
{
    const uint64_t N = (uint64_t)W * H;
    return n != 0 && N != 0 && N < (1ull << 31) && n * N < (1ull << 31);
}

// One way to lay out a device block.  `layout` names the block's parts in order through the Carver it is given, each
// with its size in bytes; every part starts 256-aligned.  It runs twice: over a null base, which gives the block's
// size, then over the allocation, which gives the pointers.  `zero`: cleared on the state's stream.
struct Carver {
    uintptr_t at;
    template <class T> void operator()(T*& p, size_t bytes) { p = (T*)at; at += align_up(bytes, 256); }
};
template <class Layout> static void* device_block(Opt_State* st, bool zero, Layout&& layout)
{
    Carver size{0};
    layout(size);
    void* block = nullptr;
    HC(hipMalloc(&block, size.at));
    if (zero) HC(hipMemsetAsync(block, 0, size.at, st->stream));
    Carver parts{(uintptr_t)block};
    layout(parts);
    return block;
}

static Opt_Plan* plan_create(Opt_State* st, int W, int H, int batch)
{
    HC(hipSetDevice(st->device));
    Opt_Plan* p = new Opt_Plan();
    p->st = st;
    p->W = W; p->H = H; p->N = W * H; p->batch = batch;
    PlanDev& pd = p->pd;
    pd.W = W; pd.H = H; pd.N = p->N;
    pd.tilesX = (W + TILE_X - 1) / TILE_X;
    pd.tilesY = (H + TILE_Y - 1) / TILE_Y;
    const size_t BN = (size_t)batch * p->N;
    // order-fixed reductions (arap_device.h: block_reduce_fixed): a slot per workgroup of the largest launch of any
    // kernel of this plan -- every tile shape is at least 16 wide and 4 high -- and the groups' tickets
    pd.maxblk = ((W + 15) / 16) * ((H + 3) / 4) + 16;
    // 8 float2 images + 7 float images + flags + tileact + slots, zero initialised (o.t:627-632)
    p->block = device_block(st, true, [&](Carver& part) {
        for (float2** f : {&pd.deltaO, &pd.rO, &pd.zO, &pd.pO0, &pd.pO1, &pd.ApO, &pd.preO, &pd.cs}) part(*f, BN * sizeof(float2));
        for (float** f : {&pd.deltaA, &pd.rA, &pd.zA, &pd.pA0, &pd.pA1, &pd.ApA, &pd.preA}) part(*f, BN * sizeof(float));
        part(pd.flags, BN);
        part(pd.tileact, (size_t)batch * pd.tilesX * pd.tilesY);
        part(pd.slots, sizeof(Slot) * batch);
        part(pd.part, (size_t)batch * pd.maxblk * 4 * sizeof(unsigned long long));
        part(pd.tick, (size_t)batch * NSHARD * RED_TICK_STRIDE * sizeof(unsigned));
        part(pd.gen, (size_t)batch * NSHARD * sizeof(unsigned));
    });
    pd.red = nullptr; pd.costred = nullptr; pd.nslots = 0; pd.ncost = 0;
    p->hslots.assign(batch, Slot{});
    p->h_ntiles.assign(batch, 0);
    p->h_tiles.assign(batch, std::vector<int>());
    p->h_tiles_valid.assign(batch, 0);
    p->h_tilepos.assign(batch, std::vector<int>());
    p->h_bandx0.assign(batch, std::vector<int>());
    p->h_t64.assign(batch, std::vector<int>());
    p->h_t64n.assign(batch, 0);
    return p;
}

static void plan_drop_graph(Opt_Plan* p)
{
    if (p->gexec) { (void)hipGraphExecDestroy(p->gexec); p->gexec = nullptr; }
    if (p->graph) { (void)hipGraphDestroy(p->graph); p->graph = nullptr; }
}

static void plan_free(Opt_Plan* p)
{
    if (!p) return;
    HC(hipStreamSynchronize(p->st->stream));
    plan_drop_graph(p);
    if (p->pd.red) (void)hipFree(p->pd.red);
    if (p->pd.costred) (void)hipFree(p->pd.costred);
    if (p->res_block) (void)hipFree(p->res_block);
    if (p->rd.zx) (void)hipFree(p->rd.zx);
    if (p->pin_wgmap) (void)hipHostFree(p->pin_wgmap);
    if (p->rd.stamps) (void)hipFree(p->rd.stamps);
    if (p->d_notgrid) (void)hipFree(p->d_notgrid);
    if (p->d_t64list) (void)hipFree(p->d_t64list);
    if (p->lm_block) (void)hipFree(p->lm_block);
    if (p->pd.lmred) (void)hipFree(p->pd.lmred);
    if (p->block) (void)hipFree(p->block);
    delete p;
}

// make sure the scalar arrays can hold lIterations PCG iterations / ncost cost entries
static void plan_reserve(Opt_Plan* p, int lIterations, int ncost)
{
    Opt_State* st = p->st;
    // (the stream is drained only where a buffer that earlier launches may still use is replaced: a first allocation
    //  must not wait for another solver object's running solve)
    if (lIterations > p->lcap || !p->pd.red) {
        if (p->pd.red) HC(hipStreamSynchronize(st->stream));
        plan_drop_graph(p);
        if (p->pd.red) HC(hipFree(p->pd.red));
        p->lcap = lIterations < 16 ? 16 : lIterations;
        p->pd.nslots = 2 * p->lcap + 1;
        HC(hipMalloc(&p->pd.red, (size_t)p->batch * p->pd.nslots * NSHARD * sizeof(double)));
    }
    if (ncost > p->ccap || !p->pd.costred) {
        if (p->pd.costred) HC(hipStreamSynchronize(st->stream));
        plan_drop_graph(p);
        if (p->pd.costred) HC(hipFree(p->pd.costred));
        p->ccap = ncost < 16 ? 16 : ncost;
        p->pd.ncost = p->ccap;
        HC(hipMalloc(&p->pd.costred, (size_t)p->batch * p->pd.ncost * NSHARD * sizeof(double)));
    }
}

static void plan_upload_slots(Opt_Plan* p)
{
    if (p->uploaded.size() == p->hslots.size() &&
        memcmp(p->uploaded.data(), p->hslots.data(), sizeof(Slot) * p->hslots.size()) == 0)
        return;
    // pageable source: the copy is staged before the call returns
    HC(hipMemcpyAsync(p->pd.slots, p->hslots.data(), sizeof(Slot) * p->hslots.size(), hipMemcpyHostToDevice,
                      p->st->stream));
    p->uploaded = p->hslots;
}

// launch `kern` with `lds_` bytes of dynamic LDS on stream `st_`; between two events when the state collects
// per-kernel times
#define LAUNCH(p, st_, kname_, kern, grid, blk, lds_, ...)                                   \
    do {                                                                                    \
        if ((p)->st->timing) {                                                              \
            KernelTimer::Rec r_;                                                            \
            r_.name = kname_;                                                               \
            HC(hipEventCreate(&r_.a)); HC(hipEventCreate(&r_.b));                           \
            HC(hipEventRecord(r_.a, st_));                                                  \
            hipLaunchKernelGGL(kern, grid, blk, lds_, st_, __VA_ARGS__);                    \
            HC(hipEventRecord(r_.b, st_));                                                  \
            (p)->st->ktimer.recs.push_back(r_);                                             \
        } else {                                                                            \
            hipLaunchKernelGGL(kern, grid, blk, lds_, st_, __VA_ARGS__);                    \
        }                                                                                   \
    } while (0)
