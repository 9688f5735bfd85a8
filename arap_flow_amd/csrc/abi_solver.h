// abi_solver.h -- the batched frame solver (ArapFlow_Solver: CombinedSolver on the device): per-slot images, upload of
// a frame with its work lists, the whole ramp / Gauss-Newton schedule of a batch enqueued without waiting, the wait with
// its one retry on the kernel-per-phase path, warps of the solved fields and the result downloads.
#pragma once

namespace arap {
struct FrameExt {              // per-slot optional warp outputs + occlusion scratch (ArapFlow_SolverSetOutputs)
    float2* bwd;
    uint8_t *occ_bwd, *occ;
    unsigned *cell, *rank;
    int4* bin;
};
struct MidDev {                // per snapshot and slot (ArapFlow_SolverSetSnapshots): the state and its four outputs
    float2 *state, *flow, *step;
    uint8_t *rgb, *mask;
};
}  // namespace arap

// Every entry point that touches a slot's images or results first waits for the solve (or warp) in flight, if any:
// ArapFlow_SolverWait returns 0 at once when there is none.
extern "C" int ArapFlow_SolverWait(ArapFlow_Solver* s);

// ---- the result groups ---------------------------------------------------------------------------------------------------
// What a solver hands out comes in four groups, each described once below: its planes in the order they have in the
// pinned staging of a `download` solve.  A plane's pinned offset is the sum of the planes before it, a slot's stride
// that sum rounded up to 256; the downloads, the Get* copies and the Host* pointers all read this table.
enum { G_BASE, G_EXTRA, G_MID, G_DIAG, G_COUNT, MAX_PLANES = 5 };
// what selects a plane: a positive value is an ARAPFLOW_OUT_* bit of the group's state
enum { SEL_ALWAYS = 0, SEL_RGB = -1 /* the slot has RGB */, SEL_DEVICE = -2 /* Get* only: never staged */ };
struct Plane {
    size_t per_vertex, fixed;       // bytes per vertex, or a fixed size (staged in the next multiple of 256)
    int sel;
    const void* (*dev)(const ArapFlow_Solver* s, unsigned slot, unsigned k);   // its device home
};
// A group's state is one number, kept three times (ResultGroup): the ARAPFLOW_OUT_* bits (extra), the number of
// snapshots (mid), 1 or 0 (base: always 1; diag).  group_items: how many sets of planes per slot that makes.
static unsigned group_items(int g, unsigned state) { return g == G_MID ? state : state != 0; }
struct ResultGroup {
    unsigned want = 0;              // for the next warps (mid: the snapshots of the next solves)
    unsigned at_warp = 0;           // ... in effect at the last warp (written by solver_enqueue_warp alone)
    unsigned at_dl = 0;             // ... carried by the last solve call's download (written by solver_download alone)
                                    // (solver_mid_alloc zeroes both when it remakes the snapshot buffers)
    char* pin = nullptr;            // pinned staging: [items][batch] slots of `stride` bytes (solver_pin)
    size_t stride = 0, off[MAX_PLANES] = {};
};

struct ArapFlow_Solver {
    Opt_State* st = nullptr;
    int W = 0, H = 0, N = 0, batch = 0;
    Opt_Plan* plan = nullptr;
    void* block = nullptr;
    std::vector<FrameDev> hfr;
    FrameDev* dfr = nullptr;
    WarpJob* djobs = nullptr;
    WarpJob* pin_jobs = nullptr;     // pinned staging of the warp jobs of one solve call
    unsigned* pin_err = nullptr;     // the resident kernel's error word as of the end of the last solve call (pinned)
    std::vector<uint8_t> has_rgb;
    std::vector<uint64_t> nactive;
    uint64_t last_pcg = 0, last_active = 0, last_grid = 0;
    unsigned last_n = 0;
    int last_cost_index = 0;
    // Host <-> device traffic runs on the solver's own copy stream through pinned staging, ordered against the
    // state's compute stream by events, so that a host can upload the next batch into one solver object and download
    // the previous results from it while ANOTHER solver object's solve occupies the compute stream (arap_deform).
    hipStream_t copy = nullptr;
    hipEvent_t ev_up = nullptr, ev_done = nullptr, ev_dl = nullptr;
    char* pin_in = nullptr;          // [batch] x {T float2[N], mask u8[N], rgb u8[3N]}
    size_t pin_in_slot = 0;
    bool uploads_pending = false;    // SetFrame since the last solve: the solve waits for ev_up
    bool inflight = false;           // a solve has been enqueued and not waited for
    bool retried = false;            // the last wait redid the schedule on the two-kernel path
    unsigned launches_at_enqueue = 0; // plan->res_launches when the pending solve call was enqueued
    unsigned a_n = 0, a_numIter = 0, a_nIt = 0, a_lIt = 0;
    int a_warp = 0, a_download = 0;
    ResultGroup res[G_COUNT];        // (the staging of a group is allocated on first download, or earlier: solver_pin)
    // optional warp outputs (ArapFlow_SolverSetOutputs); every buffer is allocated when first asked for
    void* ext = nullptr;             // device: [batch] x FrameExt buffers, then the [batch] cell arrays
    std::vector<FrameExt> hext;
    unsigned* ext_cells = nullptr;
    size_t ext_cell_slot = 0;
    // in-between frames (ArapFlow_SolverSetSnapshots, DESIGN.md "In-between frames"); nothing is allocated while off
    unsigned snap_steps[ARAPFLOW_MAX_SNAPSHOTS] = {};   // the steps of the res[G_MID].want snapshots of the next solves
    unsigned a_snap_n = 0, a_snap_steps[ARAPFLOW_MAX_SNAPSHOTS] = {};   // ... of the solve call pending or last done
    unsigned taken_n = 0;            // states the last solve call copied (they stay valid until the next one)
    void* mid = nullptr;             // device: [mid_cap][batch] x MidDev buffers, then [mid_cap][batch] WarpJobs
    unsigned mid_cap = 0;            // snapshots `mid`, `pin_mid_jobs` (and the staging, once there) are sized for
    std::vector<MidDev> hmid;        // [k * batch + slot]  (as the staging; the warp jobs of a solve: [k * nframes + slot])
    WarpJob* dmid_jobs = nullptr;
    WarpJob* pin_mid_jobs = nullptr;
    // fold diagnostics (ArapFlow_SolverSetDiag, DESIGN.md "Fold diagnostics"); nothing is allocated while off
    void* dgn = nullptr;             // device: [batch] fold maps u8[N], then [batch] DiagAcc, then [batch] ArapFlow_MeshStats
    size_t dgn_fold_slot = 0;
    DiagAcc* dgn_acc = nullptr;
    ArapFlow_MeshStats* dgn_stats = nullptr;
};

using SolverC = const ArapFlow_Solver*;
static const MidDev& mid_of(SolverC s, unsigned slot, unsigned k) { return s->hmid[(size_t)k * s->batch + slot]; }
static const Plane kPlanes[G_COUNT][MAX_PLANES] = {
    {   // base: every solve; offset and angle stay on the device
        {8, 0, SEL_ALWAYS, [](SolverC s, unsigned b, unsigned) -> const void* { return s->hfr[b].flow; }},
        {3, 0, SEL_RGB, [](SolverC s, unsigned b, unsigned) -> const void* { return s->hfr[b].out_rgb; }},
        {1, 0, SEL_ALWAYS, [](SolverC s, unsigned b, unsigned) -> const void* { return s->hfr[b].out_mask; }},
        {8, 0, SEL_DEVICE, [](SolverC s, unsigned b, unsigned) -> const void* { return s->hfr[b].O; }},
        {4, 0, SEL_DEVICE, [](SolverC s, unsigned b, unsigned) -> const void* { return s->hfr[b].A; }},
    },
    {   // extra: bwd, occ_bwd, occ
        {8, 0, ARAPFLOW_OUT_BACKWARD, [](SolverC s, unsigned b, unsigned) -> const void* { return s->hext[b].bwd; }},
        {1, 0, ARAPFLOW_OUT_BACKWARD, [](SolverC s, unsigned b, unsigned) -> const void* { return s->hext[b].occ_bwd; }},
        {1, 0, ARAPFLOW_OUT_OCCLUSION, [](SolverC s, unsigned b, unsigned) -> const void* { return s->hext[b].occ; }},
    },
    {   // mid, per snapshot k: flow, step, rgb, mask
        {8, 0, SEL_ALWAYS, [](SolverC s, unsigned b, unsigned k) -> const void* { return mid_of(s, b, k).flow; }},
        {8, 0, SEL_ALWAYS, [](SolverC s, unsigned b, unsigned k) -> const void* { return mid_of(s, b, k).step; }},
        {3, 0, SEL_RGB, [](SolverC s, unsigned b, unsigned k) -> const void* { return mid_of(s, b, k).rgb; }},
        {1, 0, SEL_ALWAYS, [](SolverC s, unsigned b, unsigned k) -> const void* { return mid_of(s, b, k).mask; }},
    },
    {   // diag: the statistics in a fixed head, fold
        {0, sizeof(ArapFlow_MeshStats), SEL_ALWAYS, [](SolverC s, unsigned b, unsigned) -> const void* { return s->dgn_stats + b; }},
        {1, 0, SEL_ALWAYS, [](SolverC s, unsigned b, unsigned) -> const void* { return (const uint8_t*)s->dgn + s->dgn_fold_slot * b; }},
    },
};
static size_t plane_bytes(const Plane& p, size_t N) { return p.fixed ? p.fixed : p.per_vertex * N; }
static bool plane_pinned(const Plane& p) { return (p.per_vertex || p.fixed) && p.sel != SEL_DEVICE; }   // (an unused entry is all zero)
// does the staging of a slot carry the plane, the group being in `state`
static bool plane_staged(SolverC s, const Plane& p, unsigned state, unsigned slot)
{
    if (!plane_pinned(p)) return false;
    return p.sel == SEL_ALWAYS || (p.sel == SEL_RGB ? s->has_rgb[slot] != 0 : (state & (unsigned)p.sel) != 0);
}
static void solver_layout_results(ArapFlow_Solver* s)
{
    for (int g = 0; g < G_COUNT; ++g) {
        size_t at = 0;
        for (int i = 0; i < MAX_PLANES; ++i) {
            const Plane& p = kPlanes[g][i];
            if (!plane_pinned(p)) continue;
            s->res[g].off[i] = at;
            at += p.fixed ? align_up(p.fixed, 256) : p.per_vertex * (size_t)s->N;
        }
        s->res[g].stride = align_up(at, 256);
    }
    s->res[G_BASE].want = s->res[G_BASE].at_warp = 1;
}

// pinned staging of a group's downloads, allocated when first needed: in the asynchronous use (`own_stream`) when the
// group is set up -- at creation, SetOutputs, SetDiag, the first solve with snapshots -- (hipHostMalloc waits for the
// device, i.e. for another solver object's running solve), else at the first download
static void solver_pin(ArapFlow_Solver* s, int g)
{
    ResultGroup& r = s->res[g];
    if (r.pin) return;
    HC(hipHostMalloc((void**)&r.pin, r.stride * s->batch * (g == G_MID ? s->mid_cap : 1), hipHostMallocDefault));
}

// device buffers of `n` snapshots: 8 B per vertex, snapshot and slot for the state, 20 B for the four outputs
static void solver_mid_alloc(ArapFlow_Solver* s, unsigned n)
{
    if (n <= s->mid_cap) return;
    HC(hipSetDevice(s->st->device));
    ResultGroup& r = s->res[G_MID];
    if (s->mid) HC(hipFree(s->mid));
    if (s->pin_mid_jobs) HC(hipHostFree(s->pin_mid_jobs));
    if (r.pin) HC(hipHostFree(r.pin));
    r.pin = nullptr;
    const size_t N = s->N, B = s->batch;
    s->hmid.resize(n * B);
    s->mid = device_block(s->st, true, [&](Carver& part) {
        for (MidDev& m : s->hmid) {
            part(m.state, 8 * N); part(m.flow, 8 * N); part(m.step, 8 * N);
            part(m.rgb, 3 * N); part(m.mask, N);
        }
        part(s->dmid_jobs, sizeof(WarpJob) * n * B);
    });
    HC(hipHostMalloc((void**)&s->pin_mid_jobs, sizeof(WarpJob) * n * B, hipHostMallocDefault));
    HC(hipStreamSynchronize(s->st->stream));
    s->mid_cap = n;
    s->taken_n = r.at_warp = r.at_dl = 0;
    if (s->st->own_stream) solver_pin(s, G_MID);
}

static void solver_enqueue_warp(ArapFlow_Solver* s, unsigned nframes)
{
    Opt_State* st = s->st;
    WarpJob* jobs = s->pin_jobs;             // (pinned: see plan_gn_step on pageable sources)
    const bool diag = s->res[G_DIAG].want != 0;
    for (unsigned b = 0; b < nframes; ++b) {
        const FrameDev& f = s->hfr[b];
        WarpJob& j = jobs[b];
        j.field = f.O; j.flow_in = nullptr;
        j.rgb = s->has_rgb[b] ? f.rgb : nullptr;
        j.mask = f.mask; j.flow_out = f.flow; j.key = f.key;
        j.out_rgb = s->has_rgb[b] ? f.out_rgb : nullptr;
        j.out_mask = f.out_mask;
        const int o = (int)s->res[G_EXTRA].want;
        const FrameExt* e = o ? &s->hext[b] : nullptr;
        j.bwd = (o & ARAPFLOW_OUT_BACKWARD) ? e->bwd : nullptr;
        j.occ_bwd = (o & ARAPFLOW_OUT_BACKWARD) ? e->occ_bwd : nullptr;
        j.occ = (o & ARAPFLOW_OUT_OCCLUSION) ? e->occ : nullptr;
        j.cell = e ? e->cell : nullptr; j.rank = e ? e->rank : nullptr; j.bin = e ? e->bin : nullptr;
        j.fold = diag ? (uint8_t*)s->dgn + s->dgn_fold_slot * b : nullptr;
        j.acc = diag ? s->dgn_acc + b : nullptr;
        j.stats = diag ? s->dgn_stats + b : nullptr;
    }
    HC(hipMemcpyAsync(s->djobs, jobs, sizeof(WarpJob) * nframes, hipMemcpyHostToDevice, st->stream));
    enqueue_warp(st->stream, s->djobs, nframes, s->W, s->H, (int)s->res[G_EXTRA].want, s->ext_cells, s->ext_cell_slot * nframes);
    if (diag) enqueue_warp_diag(st->stream, s->djobs, nframes, s->W, s->H, s->dgn_acc, sizeof(DiagAcc) * nframes);
    // the in-between frames of the last solve: one warp pass per snapshot over the slots, on the field S_{i_k}, with the
    // step towards the next state; the slot's key image serves every pass (k_warp_resolve left it cleared)
    const unsigned n = s->taken_n;
    for (int g = 0; g < G_COUNT; ++g) s->res[g].at_warp = g == G_MID ? n : s->res[g].want;
    if (n == 0) return;
    WarpJob* mj = s->pin_mid_jobs;
    for (unsigned k = 0; k < n; ++k)
        for (unsigned b = 0; b < nframes; ++b) {
            const FrameDev& f = s->hfr[b];
            const MidDev& m = mid_of(s, b, k);
            WarpJob j{};
            j.field = m.state;
            j.rgb = s->has_rgb[b] ? f.rgb : nullptr;
            j.mask = f.mask; j.flow_out = m.flow; j.key = f.key;
            j.out_rgb = s->has_rgb[b] ? m.rgb : nullptr;
            j.out_mask = m.mask;
            j.field_b = k + 1 < n ? mid_of(s, b, k + 1).state : f.O;
            j.step = m.step;
            mj[(size_t)k * nframes + b] = j;
        }
    HC(hipMemcpyAsync(s->dmid_jobs, mj, sizeof(WarpJob) * n * nframes, hipMemcpyHostToDevice, st->stream));
    for (unsigned k = 0; k < n; ++k)
        enqueue_warp(st->stream, s->dmid_jobs + (size_t)k * nframes, nframes, s->W, s->H, 0, nullptr, 0, true);
}

// one group's downloads of a solve call on the copy stream: of every slot (and snapshot) the planes that it has
static void solver_download(ArapFlow_Solver* s, int g, unsigned nframes, unsigned state)
{
    ResultGroup& r = s->res[g];
    r.at_dl = state;
    const unsigned items = group_items(g, state);
    if (!items) return;
    solver_pin(s, g);
    for (unsigned k = 0; k < items; ++k)
        for (unsigned b = 0; b < nframes; ++b) {
            char* o = r.pin + r.stride * ((size_t)k * s->batch + b);
            for (int i = 0; i < MAX_PLANES; ++i) {
                const Plane& p = kPlanes[g][i];
                if (plane_staged(s, p, state, b))
                    HC(hipMemcpyAsync(o + r.off[i], p.dev(s, b, k), plane_bytes(p, s->N), hipMemcpyDeviceToHost, s->copy));
            }
        }
}

// the whole schedule of slots [0, a_n) on the compute stream (+ warp, + download on the copy stream), no waiting
static void solver_enqueue(ArapFlow_Solver* s)
{
    Opt_State* st = s->st;
    Opt_Plan* p = s->plan;
    const unsigned nframes = s->a_n, numIter = s->a_numIter;
    p->nb = (int)nframes;
    p->sp.nIterations = (int)s->a_nIt;
    p->sp.lIterations = (int)s->a_lIt;
    if (s->uploads_pending) {
        HC(hipEventRecord(s->ev_up, s->copy));
        HC(hipStreamWaitEvent(st->stream, s->ev_up, 0));
        s->uploads_pending = false;
    }
    const dim3 g1((s->N + 255) / 256, 1, nframes);
    // preSingleSolve = resetGPU (CombinedSolver.h:191-193)
    hipLaunchKernelGGL(k_frame_reset, g1, dim3(256), 0, st->stream, s->dfr, s->W, s->N);
    for (unsigned i = 0; i < numIter; ++i) {
        const float alpha = (float)(i + 1) / (float)numIter;          // CombinedSolver.h:199-201
        hipLaunchKernelGGL(k_frame_ramp, g1, dim3(256), 0, st->stream, s->dfr, s->W, s->N, alpha);
        p->lazy_cost = true;
        p->cost_wanted = i + 1 == numIter;
        plan_init(p);
        if (!plan_steps_batched(p))
            while (plan_step(p) != 0) {}
        // a snapshot of ramp step i + 1: Offset is current here on every path (the resident launch and k_gn_update both
        // apply the step to Offset itself), so the state is a copy between two ramp steps' launches
        for (unsigned k = 0; k < s->a_snap_n; ++k)
            if (s->a_snap_steps[k] == i + 1)
                for (unsigned b = 0; b < nframes; ++b)
                    HC(hipMemcpyAsync(mid_of(s, b, k).state, s->hfr[b].O, sizeof(float2) * s->N, hipMemcpyDeviceToDevice, st->stream));
    }
    s->taken_n = s->a_snap_n;
    if (s->a_warp) solver_enqueue_warp(s, nframes);
    if (p->res_capable) {
        *s->pin_err = 0u;
        HC(hipMemcpyAsync(s->pin_err, p->rd.err, sizeof(unsigned), hipMemcpyDeviceToHost, st->stream));
    }
    HC(hipEventRecord(s->ev_done, st->stream));
    if (s->a_download) {
        HC(hipStreamWaitEvent(s->copy, s->ev_done, 0));
        // (without a warp in this call the optional groups are not carried: their buffers are an earlier warp's)
        for (int g = 0; g < G_COUNT; ++g)
            solver_download(s, g, nframes, g == G_BASE || s->a_warp ? s->res[g].at_warp : 0u);
        HC(hipEventRecord(s->ev_dl, s->copy));
    }
    s->last_cost_index = p->sp.nIter;
    s->last_n = nframes;
    s->last_pcg = (uint64_t)numIter * s->a_nIt * s->a_lIt;
    s->last_active = 0;
    for (unsigned b = 0; b < nframes; ++b) s->last_active += s->nactive[b];
    s->last_grid = (uint64_t)nframes * s->N;
}

extern "C" {

ArapFlow_Solver* ArapFlow_SolverCreate(Opt_State* st, unsigned W, unsigned H, unsigned batch)
{
    if (!st || W == 0 || H == 0 || batch == 0) return nullptr;
    HC(hipSetDevice(st->device));
    ArapFlow_Solver* s = new ArapFlow_Solver();
    s->st = st; s->W = (int)W; s->H = (int)H; s->N = (int)(W * H); s->batch = (int)batch;
    s->plan = plan_create(st, (int)W, (int)H, (int)batch);
    plan_enable_resident(s->plan);
    s->plan->res_frames = s->plan->res_capable;
    s->plan->res_frames_any = true;
    s->plan->grid_u = true;                                   // k_frame_reset writes U = the pixel grid
    {
        const size_t T = (size_t)s->plan->pd.tilesX * s->plan->pd.tilesY;
        HC(hipMalloc(&s->plan->d_t64list, (batch * T + batch) * sizeof(int)));
        HC(hipMemsetAsync(s->plan->d_t64list, 0, (batch * T + batch) * sizeof(int), st->stream));
        s->plan->d_t64n = s->plan->d_t64list + batch * T;
    }
    const size_t N = s->N;
    s->hfr.resize(batch);
    s->block = device_block(st, true, [&](Carver& part) {
        for (FrameDev& f : s->hfr) {
            for (float2** q : {&f.O, &f.U, &f.C, &f.T, &f.flow}) part(*q, N * sizeof(float2));
            part(f.A, N * sizeof(float)); part(f.M, N * sizeof(float));
            part(f.mask, N); part(f.out_mask, N);
            part(f.rgb, 3 * N); part(f.out_rgb, 3 * N);
            part(f.key, N * 8);
        }
        part(s->dfr, sizeof(FrameDev) * batch);
        part(s->djobs, sizeof(WarpJob) * batch);
    });
    HC(hipMemcpyAsync(s->dfr, s->hfr.data(), sizeof(FrameDev) * batch, hipMemcpyHostToDevice, st->stream));
    HC(hipStreamSynchronize(st->stream));
    HC(hipStreamCreateWithFlags(&s->copy, hipStreamNonBlocking));
    HC(hipEventCreateWithFlags(&s->ev_up, hipEventDisableTiming));
    HC(hipEventCreateWithFlags(&s->ev_done, hipEventDisableTiming));
    HC(hipEventCreateWithFlags(&s->ev_dl, hipEventDisableTiming));
    s->pin_in_slot = align_up((8 + 1 + 3) * N, 256);
    HC(hipHostMalloc((void**)&s->pin_in, s->pin_in_slot * batch, hipHostMallocDefault));
    // (allocated here, not at first use: hipHostMalloc waits for the device, i.e. for another solver object's running solve)
    HC(hipHostMalloc((void**)&s->pin_jobs, sizeof(WarpJob) * batch, hipHostMallocDefault));
    HC(hipHostMalloc((void**)&s->pin_err, 64, hipHostMallocDefault));
    solver_layout_results(s);
    if (st->own_stream) solver_pin(s, G_BASE);   // the asynchronous use (ArapFlow_UseOwnStream first): downloads will be asked for
    s->has_rgb.assign(batch, 0);
    s->nactive.assign(batch, 0);
    const float wfit = sqrtf(100.0f), wreg = sqrtf(0.01f);   // CombinedSolver.h:173-177
    for (unsigned b = 0; b < batch; ++b) {
        Slot& sl = s->plan->hslots[b];
        const FrameDev& f = s->hfr[b];
        sl.O = f.O; sl.A = f.A; sl.U = f.U; sl.C = f.C; sl.M = f.M;
        sl.wf = wfit; sl.wr = wreg;
    }
    return s;
}

void ArapFlow_SolverFree(ArapFlow_Solver* s)
{
    if (!s) return;
    (void)ArapFlow_SolverWait(s);
    (void)hipStreamSynchronize(s->copy);
    plan_free(s->plan);
    (void)hipStreamDestroy(s->copy);
    (void)hipEventDestroy(s->ev_up); (void)hipEventDestroy(s->ev_done); (void)hipEventDestroy(s->ev_dl);
    if (s->pin_in) (void)hipHostFree(s->pin_in);
    for (ResultGroup& r : s->res)
        if (r.pin) (void)hipHostFree(r.pin);
    if (s->pin_jobs) (void)hipHostFree(s->pin_jobs);
    if (s->pin_err) (void)hipHostFree(s->pin_err);
    if (s->ext) (void)hipFree(s->ext);
    if (s->mid) (void)hipFree(s->mid);
    if (s->pin_mid_jobs) (void)hipHostFree(s->pin_mid_jobs);
    if (s->dgn) (void)hipFree(s->dgn);
    (void)hipFree(s->block);
    delete s;
}

int ArapFlow_SolverSetFrame(ArapFlow_Solver* s, unsigned slot, const uint8_t* rgb, const uint8_t* mask_red,
                            const int32_t* cons, unsigned ncons, int add_border_pins)
{
    if (!s || slot >= (unsigned)s->batch || !mask_red || (ncons && !cons)) return -1;
    // the previous solve of THIS solver may still read the slot's images and tile lists
    if (const int rc = ArapFlow_SolverWait(s)) return rc;                                   // (-2: the retry failed too)
    const int W = s->W, H = s->H;
    const size_t N = s->N;
    // the staging of this slot may still be the source of an earlier upload
    HC(hipStreamSynchronize(s->copy));
    char* stage = s->pin_in + s->pin_in_slot * slot;
    float2* T = (float2*)stage;
    uint8_t* smask = (uint8_t*)(T + N);
    uint8_t* srgb = smask + N;
    // host pre-pass of setConstraintImage's placement loop (CombinedSolver.h:230-240): file
    // constraints first, then border pins (main.cpp:130-136); later entries overwrite earlier ones;
    // only where Mask == 0.
    const float2 none = make_float2(NAN, NAN);
    for (size_t i = 0; i < N; ++i) T[i] = none;
    auto place = [&](int x, int y, int tx, int ty) {
        if (x < 0 || x >= W || y < 0 || y >= H) return;
        if (mask_red[x + (size_t)W * y] == 0) T[x + (size_t)W * y] = make_float2((float)tx, (float)ty);
    };
    for (unsigned k = 0; k < ncons; ++k) place(cons[4 * k], cons[4 * k + 1], cons[4 * k + 2], cons[4 * k + 3]);
    if (add_border_pins) {
        for (int x = 0; x < W; ++x) place(x, 0, x, 0);
        for (int y = 1; y + 1 < H; ++y) { place(0, y, 0, y); if (W > 1) place(W - 1, y, W - 1, y); }
        if (H > 1) for (int x = 0; x < W; ++x) place(x, H - 1, x, H - 1);
    }
    memcpy(smask, mask_red, N);
    if (rgb) memcpy(srgb, rgb, 3 * N);
    // active vertices and the resident kernel's work list of this frame (aligned 32x8 tiles, band by band)
    std::vector<int> tiles, bandx0;
    uint64_t na = 0;
    build_resident_tiles(mask_red, W, H, true, tiles, bandx0, &na);
    s->nactive[slot] = na;
    plan_upload_tiles(s->plan, (int)slot, tiles, bandx0, s->copy);
    {
        // active 64x4 tiles (list launches of the per-step kernels).  Those kernels then rewrite flags / tile activity
        // inside the listed tiles only, so what an earlier frame left in this slot is cleared here.
        Opt_Plan* p = s->plan;
        const int tX = p->pd.tilesX, tY = p->pd.tilesY;
        std::vector<int>& l64 = p->h_t64[slot];
        build_t64_list(mask_red, W, H, tX, tY, l64);
        p->h_t64n[slot] = (int)l64.size();
        const size_t T = (size_t)tX * tY;
        if (!l64.empty())
            HC(hipMemcpyAsync(p->d_t64list + slot * T, l64.data(), l64.size() * sizeof(int), hipMemcpyHostToDevice, s->copy));
        HC(hipMemcpyAsync(p->d_t64n + slot, &p->h_t64n[slot], sizeof(int), hipMemcpyHostToDevice, s->copy));
        HC(hipMemsetAsync(p->pd.flags + (size_t)slot * N, 0, N, s->copy));
        HC(hipMemsetAsync(p->pd.tileact + (size_t)slot * T, 0, T, s->copy));
    }
    const FrameDev& f = s->hfr[slot];
    HC(hipMemcpyAsync(f.T, T, N * sizeof(float2), hipMemcpyHostToDevice, s->copy));
    HC(hipMemcpyAsync(f.mask, smask, N, hipMemcpyHostToDevice, s->copy));
    if (rgb) HC(hipMemcpyAsync(f.rgb, srgb, 3 * N, hipMemcpyHostToDevice, s->copy));
    s->has_rgb[slot] = rgb ? 1 : 0;
    s->uploads_pending = true;
    return 0;
}

int ArapFlow_SolverSolveAsync(ArapFlow_Solver* s, unsigned nframes, unsigned numIter, unsigned nIterations,
                              unsigned lIterations, int warp, int download)
{
    if (!s || nframes == 0 || nframes > (unsigned)s->batch || numIter == 0) return -1;
    const unsigned snaps = s->res[G_MID].want;
    if (snaps && s->snap_steps[snaps - 1] > numIter) return -1;     // (increasing: the last is the largest)
    if (ArapFlow_SolverWait(s) != 0) return -1;
    Opt_State* st = s->st;
    HC(hipSetDevice(st->device));
    s->a_snap_n = snaps;
    memcpy(s->a_snap_steps, s->snap_steps, sizeof(s->snap_steps));
    solver_mid_alloc(s, snaps);                              // (the first solve that needs it; nothing with none)
    const bool paused = st->res_cooldown > 0;                 // this call runs on the two-kernel path: counts as one
    s->a_n = nframes; s->a_numIter = numIter; s->a_nIt = nIterations; s->a_lIt = lIterations;
    s->a_warp = warp; s->a_download = download;
    s->retried = false;
    s->launches_at_enqueue = s->plan->res_launches;
    solver_enqueue(s);
    if (paused) --st->res_cooldown;
    s->inflight = true;
    return 0;
}

int ArapFlow_SolverWait(ArapFlow_Solver* s)
{
    if (!s) return -1;
    if (!s->inflight) return 0;
    Opt_State* st = s->st;
    Opt_Plan* p = s->plan;
    HC(hipEventSynchronize(s->ev_done));
    // The resident path needs all its workgroups co-resident; if a launch gave up (GPU shared with another process) the
    // device skipped every later update: redo the whole schedule once, now on the two-kernel path (plan_resident_failed
    // pauses the resident path), from the reset.
    // (The error word came back with the solve, in stream order, into pinned memory: reading it through the compute
    //  stream here would wait for whatever ANOTHER solver object has enqueued there since -- with two alternating solver
    //  objects, for the other one's whole solve.  Only a non-zero word takes the blocking path.)
    if (p->res_launches > 0 && s->pin_err && *s->pin_err != 0u && plan_resident_failed(p)) {
        HC(hipStreamSynchronize(s->copy));
        solver_enqueue(s);
        s->retried = true;
        HC(hipEventSynchronize(s->ev_done));
        if (plan_resident_failed(p)) {
            fprintf(stderr, "arapopt: the two-kernel retry reported a resident failure\n");
            s->inflight = false;
            return -2;
        }
    } else if (p->res_launches != s->launches_at_enqueue) {
        st->res_backoff = 8;                                  // a CHECKED resident success (this call launched the kernel)
    }
    if (s->a_download) HC(hipEventSynchronize(s->ev_dl));
    s->inflight = false;
    return 0;
}

int ArapFlow_SolverSolve(ArapFlow_Solver* s, unsigned nframes, unsigned numIter, unsigned nIterations,
                         unsigned lIterations)
{
    const int rc = ArapFlow_SolverSolveAsync(s, nframes, numIter, nIterations, lIterations, 0, 0);
    return rc != 0 ? rc : ArapFlow_SolverWait(s);
}

int ArapFlow_SolverWarp(ArapFlow_Solver* s, unsigned nframes)
{
    if (!s || nframes == 0 || nframes > (unsigned)s->batch) return -1;
    if (const int rc = ArapFlow_SolverWait(s)) return rc;
    solver_enqueue_warp(s, nframes);
    // the rasteriser reads the slots' mask / rgb and rewrites their outputs: every later call on this solver that touches
    // them (SetFrame, GetResults, ...) waits for it like for a solve
    HC(hipEventRecord(s->ev_done, s->st->stream));
    s->launches_at_enqueue = s->plan->res_launches;
    s->inflight = true;
    return 0;
}

int ArapFlow_SolverSetOutputs(ArapFlow_Solver* s, int which)
{
    if (!s || (which & ~(ARAPFLOW_OUT_BACKWARD | ARAPFLOW_OUT_OCCLUSION))) return -1;
    if (const int rc = ArapFlow_SolverWait(s)) return rc;
    if (which && !s->ext) {
        HC(hipSetDevice(s->st->device));
        const size_t N = s->N;
        const WarpScratch L = warp_scratch(s->W, s->H, WARP_OCC);      // the occlusion scratch of one job
        s->ext_cell_slot = L.rank - L.cell;
        s->hext.resize(s->batch);
        s->ext = device_block(s->st, true, [&](Carver& part) {
            for (FrameExt& e : s->hext) {
                part(e.bwd, 8 * N); part(e.occ_bwd, N); part(e.occ, N);
                part(e.rank, L.bin - L.rank); part(e.bin, L.owner - L.bin);
            }
            for (FrameExt& e : s->hext) part(e.cell, s->ext_cell_slot);
        });
        s->ext_cells = s->hext[0].cell;
        HC(hipStreamSynchronize(s->st->stream));
        if (s->st->own_stream) solver_pin(s, G_EXTRA);
    }
    s->res[G_EXTRA].want = (unsigned)which;
    return 0;
}

int ArapFlow_SolverSetSnapshots(ArapFlow_Solver* s, const unsigned* steps, unsigned n)
{
    if (!s || n > ARAPFLOW_MAX_SNAPSHOTS || (n && !steps)) return -1;
    for (unsigned k = 0; k < n; ++k)
        if (steps[k] < 1 || (k && steps[k] <= steps[k - 1])) return -1;
    if (const int rc = ArapFlow_SolverWait(s)) return rc;
    s->res[G_MID].want = n;
    for (unsigned k = 0; k < n; ++k) s->snap_steps[k] = steps[k];
    return 0;
}

// What the Get* entry points do: wait, check that the last warp wrote what is asked for, and copy it to the host
// behind the compute stream.  `dst`: a host buffer per plane in the table's order, nullptr = not asked.
static int solver_get(ArapFlow_Solver* s, int g, unsigned slot, unsigned k, void* const (&dst)[MAX_PLANES])
{
    if (!s || slot >= (unsigned)s->batch) return -1;
    if (ArapFlow_SolverWait(s) != 0) return -1;
    const unsigned state = s->res[g].at_warp;
    if (g != G_EXTRA && k >= group_items(g, state)) return -1;      // (the extra outputs are judged plane by plane)
    for (int i = 0; i < MAX_PLANES; ++i)
        if (dst[i] && kPlanes[g][i].sel > 0 && !(state & (unsigned)kPlanes[g][i].sel)) return -1;
    HC(hipStreamSynchronize(s->st->stream));
    for (int i = 0; i < MAX_PLANES; ++i)
        if (dst[i])
            HC(hipMemcpyAsync(dst[i], kPlanes[g][i].dev(s, slot, k), plane_bytes(kPlanes[g][i], s->N), hipMemcpyDeviceToHost, s->copy));
    HC(hipStreamSynchronize(s->copy));
    return 0;
}

// What the Host* entry points do: pointers into the staging of the last solve call, which must have been a `download`
// solve of this slot; nullptr for a plane the slot or that solve does not have.  `out`: as `dst` above.
static int solver_host(ArapFlow_Solver* s, int g, unsigned slot, unsigned k, const void** const (&out)[MAX_PLANES])
{
    if (!s || slot >= (unsigned)s->batch || !s->a_download || slot >= s->a_n) return -1;
    if (ArapFlow_SolverWait(s) != 0) return -1;
    const ResultGroup& r = s->res[g];
    if (k >= group_items(g, r.at_dl) || !r.pin) return -1;
    const char* o = r.pin + r.stride * ((size_t)k * s->batch + slot);
    for (int i = 0; i < MAX_PLANES; ++i)
        if (out[i]) *out[i] = plane_staged(s, kPlanes[g][i], r.at_dl, slot) ? o + r.off[i] : nullptr;
    return 0;
}

int ArapFlow_SolverGetSnapshot(ArapFlow_Solver* s, unsigned slot, unsigned k, float* flow, uint8_t* rgb, uint8_t* mask,
                               float* step)
{
    if (s && slot < (unsigned)s->batch && rgb && !s->has_rgb[slot]) return -1;
    return solver_get(s, G_MID, slot, k, {flow, step, rgb, mask});
}

int ArapFlow_SolverHostSnapshot(ArapFlow_Solver* s, unsigned slot, unsigned k, const float** flow, const uint8_t** rgb,
                                const uint8_t** mask, const float** step)
{
    return solver_host(s, G_MID, slot, k, {(const void**)flow, (const void**)step, (const void**)rgb, (const void**)mask});
}

int ArapFlow_SolverGetExtraResults(ArapFlow_Solver* s, unsigned slot, float* bwd, uint8_t* occ_bwd, uint8_t* occ)
{
    return solver_get(s, G_EXTRA, slot, 0, {bwd, occ_bwd, occ});
}

int ArapFlow_SolverHostExtraResults(ArapFlow_Solver* s, unsigned slot, const float** bwd, const uint8_t** occ_bwd,
                                    const uint8_t** occ)
{
    return solver_host(s, G_EXTRA, slot, 0, {(const void**)bwd, (const void**)occ_bwd, (const void**)occ});
}

int ArapFlow_SolverSetDiag(ArapFlow_Solver* s, int on)
{
    if (!s) return -1;
    if (const int rc = ArapFlow_SolverWait(s)) return rc;
    if (on && !s->dgn) {
        HC(hipSetDevice(s->st->device));
        const size_t B = s->batch;
        s->dgn_fold_slot = align_up((size_t)s->N, 256);
        uint8_t* folds = nullptr;
        s->dgn = device_block(s->st, false, [&](Carver& part) {
            part(folds, s->dgn_fold_slot * B);
            part(s->dgn_acc, sizeof(DiagAcc) * B);
            part(s->dgn_stats, sizeof(ArapFlow_MeshStats) * B);
        });
        if (s->st->own_stream) solver_pin(s, G_DIAG);
    }
    s->res[G_DIAG].want = on ? 1 : 0;
    return 0;
}

int ArapFlow_SolverGetDiag(ArapFlow_Solver* s, unsigned slot, ArapFlow_MeshStats* stats, uint8_t* fold)
{
    return solver_get(s, G_DIAG, slot, 0, {stats, fold});
}

int ArapFlow_SolverHostDiag(ArapFlow_Solver* s, unsigned slot, const ArapFlow_MeshStats** stats, const uint8_t** fold)
{
    return solver_host(s, G_DIAG, slot, 0, {(const void**)stats, (const void**)fold});
}

int ArapFlow_SolverHostResults(ArapFlow_Solver* s, unsigned slot, const float** flow, const uint8_t** warped_rgb,
                               const uint8_t** warped_mask)
{
    return solver_host(s, G_BASE, slot, 0, {(const void**)flow, (const void**)warped_rgb, (const void**)warped_mask});
}

int ArapFlow_SolverGetResults(ArapFlow_Solver* s, unsigned slot, float* flow, uint8_t* warped_rgb,
                              uint8_t* warped_mask, float* offset, float* angle, double* final_cost)
{
    if (solver_get(s, G_BASE, slot, 0, {flow, warped_rgb, warped_mask, offset, angle}) != 0) return -1;
    plan_check_resident_error(s->plan);
    if (final_cost) *final_cost = plan_read_cost(s->plan, (int)slot, s->last_cost_index);
    return 0;
}

int ArapFlow_SolverStats(ArapFlow_Solver* s, uint64_t* pcg, uint64_t* active, uint64_t* grid)
{
    if (!s) return -1;
    if (pcg) *pcg = s->last_pcg;
    if (active) *active = s->last_active;
    if (grid) *grid = s->last_grid;
    return 0;
}

uint64_t ArapFlow_SolverResidentLaunches(ArapFlow_Solver* s) { return s ? s->plan->res_launches : 0; }
uint64_t ArapFlow_PlanResidentLaunches(Opt_Plan* plan) { return plan ? plan->res_launches : 0; }
int ArapFlow_SolverLaunchesFor(ArapFlow_Solver* s, unsigned nframes)
{
    if (!s || nframes == 0 || nframes > (unsigned)s->plan->batch) return -1;
    Opt_Plan* p = s->plan;
    const int keep = p->nb;
    p->nb = (int)nframes;                              // eligibility looks at the first nb slots
    const int sets = plan_resident_eligible(p) ? resident_deal(p->h_ntiles.data(), (int)nframes, p->knob_res_groups, nullptr, nullptr) : 0;
    p->nb = keep;
    return sets;
}
int ArapFlow_ResidentDeal(const int* active_tiles, unsigned nsolves, int* table, unsigned table_launches)
{
    if (!active_tiles || nsolves == 0) return -1;
    for (unsigned b = 0; b < nsolves; ++b)
        if (active_tiles[b] < 0 || active_tiles[b] > RES_MAX_TILES) return -1;
    std::vector<ResWg> map;
    const int sets = resident_deal(active_tiles, (int)nsolves, read_knobs().res_groups, &map, nullptr);   // (no plan: read per call)
    if (table)
        for (size_t i = 0; i < map.size() && i < (size_t)table_launches * RES_WGS; ++i) {
            table[4 * i + 0] = map[i].slot; table[4 * i + 1] = map[i].rank;
            table[4 * i + 2] = map[i].wgs; table[4 * i + 3] = map[i].gran;
        }
    return sets;
}
int ArapFlow_ResidentTiles(const uint8_t* mask_red, unsigned W, unsigned H, int aligned, int* origins, unsigned cap,
                           int* bandx0)
{
    if (!mask_red || W == 0 || H == 0) return -1;
    std::vector<int> tiles, bx;
    build_resident_tiles(mask_red, (int)W, (int)H, aligned != 0, tiles, bx, nullptr);
    if (origins)
        for (size_t i = 0; i < tiles.size() && i < cap; ++i) origins[i] = tiles[i];
    if (bandx0)
        for (size_t i = 0; i < bx.size(); ++i) bandx0[i] = bx[i];
    return (int)tiles.size();
}
int ArapFlow_SolverResidentLayout(ArapFlow_Solver* s, int* launches_per_step, int* solves_in_flight)
{
    if (!s) return -1;
    const bool res = plan_resident_eligible(s->plan) && s->plan->res_sets > 0;
    if (launches_per_step) *launches_per_step = res ? s->plan->res_sets : 0;
    if (solves_in_flight) *solves_in_flight = res ? s->plan->res_inflight : 0;
    return 0;
}
int ArapFlow_SolverResidentSums(ArapFlow_Solver* s, int* sums, unsigned cap)
{
    if (!s) return -1;
    const Opt_Plan* p = s->plan;
    if (!plan_resident_eligible(p) || p->res_sets <= 0) return 0;
    for (int k = 0; k < p->res_sets && sums && (unsigned)k < cap; ++k) sums[k] = p->res_sums[k];
    return p->res_sets;
}
int ArapFlow_ResidentFailed(Opt_State* state) { return state && state->resident_failed ? 1 : 0; }
int ArapFlow_SolverLeanStream(ArapFlow_Solver* s) { return s && plan_lean_stream(s->plan) ? 1 : 0; }
// read-only: what plan_step_recipe decided for the step whose graph the plan holds (Opt_Plan::g_recipe)
int ArapFlow_SolverStepRecipe(ArapFlow_Solver* s, int* out)
{
    if (!s || !out) return -1;
    const Opt_Plan* p = s->plan;
    const bool have = p->gexec != nullptr;
    const StepRecipe none;
    const StepRecipe& r = have ? p->g_recipe : none;
    out[0] = r.a_kern; out[1] = r.b_kern;
    for (int k = 0; k < 3; ++k) out[2 + k] = r.a_arg[k];
    out[5] = r.lag;
    return have ? 1 : 0;
}

// diagnostic (ARAPOPT_STAMPS=1): copy the [256][8] phase-time table of the LAST resident launch (table 0)
// ... or its second [512][16] table: the parts of the on-chip chain of a group sum, arrival times, placement, work
static int solver_stamp_table(ArapFlow_Solver* s, int table, uint64_t* out)
{
    if (!s || !s->plan->rd.stamps) return -1;
    HC(hipStreamSynchronize(s->st->stream));
    HC(hipMemcpy(out, s->plan->rd.stamps + table * RES_WGS * 16, RES_WGS * 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return 0;
}
int ArapFlow_SolverStamps(ArapFlow_Solver* s, uint64_t* out) { return solver_stamp_table(s, 0, out); }
int ArapFlow_SolverStampParts(ArapFlow_Solver* s, uint64_t* out) { return solver_stamp_table(s, 1, out); }

}  // extern "C"
