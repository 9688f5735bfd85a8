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
    char* pin_out = nullptr;         // [batch] x {flow float2[N], rgb u8[3N], mask u8[N]}   (allocated on first download)
    size_t pin_in_slot = 0, pin_out_slot = 0;
    bool uploads_pending = false;    // SetFrame since the last solve: the solve waits for ev_up
    bool inflight = false;           // a solve has been enqueued and not waited for
    bool retried = false;            // the last wait redid the schedule on the two-kernel path
    unsigned launches_at_enqueue = 0; // plan->res_launches when the pending solve call was enqueued
    unsigned a_n = 0, a_numIter = 0, a_nIt = 0, a_lIt = 0;
    int a_warp = 0, a_download = 0;
    // optional warp outputs (ArapFlow_SolverSetOutputs); every buffer is allocated when first asked for
    int outputs = 0;                 // ARAPFLOW_OUT_* bits for the next warps
    int warp_outputs = 0;            // ... in effect at the last warp
    int dl_outputs = 0;              // ... downloaded by the last solve call
    void* ext = nullptr;             // device: [batch] x FrameExt buffers, then the [batch] cell arrays
    std::vector<FrameExt> hext;
    unsigned* ext_cells = nullptr;
    size_t ext_cell_slot = 0;
    char* pin_ext = nullptr;         // [batch] x {bwd float2[N], occ_bwd u8[N], occ u8[N]}   (allocated on first download)
    size_t pin_ext_slot = 0;
    // in-between frames (ArapFlow_SolverSetSnapshots, DESIGN.md "In-between frames"); nothing is allocated while off
    unsigned snap_n = 0, snap_steps[ARAPFLOW_MAX_SNAPSHOTS] = {};   // the set for the next solves
    unsigned a_snap_n = 0, a_snap_steps[ARAPFLOW_MAX_SNAPSHOTS] = {};   // ... of the solve call pending or last done
    unsigned taken_n = 0;            // states the last solve call copied (they stay valid until the next one)
    unsigned warp_snap_n = 0;        // snapshots the last warp wrote outputs for
    unsigned dl_snap_n = 0;          // ... the last solve call downloaded
    void* mid = nullptr;             // device: [mid_cap][batch] x MidDev buffers, then [mid_cap][batch] WarpJobs
    unsigned mid_cap = 0;            // snapshots `mid`, `pin_mid_jobs` (and `pin_mid`, once there) are sized for
    std::vector<MidDev> hmid;        // [k * batch + slot]
    WarpJob* dmid_jobs = nullptr;
    WarpJob* pin_mid_jobs = nullptr;
    char* pin_mid = nullptr;         // [mid_cap][batch] x {flow float2[N], step float2[N], rgb u8[3N], mask u8[N]}
    size_t pin_mid_slot = 0;
    // fold diagnostics (ArapFlow_SolverSetDiag, DESIGN.md "Fold diagnostics"); nothing is allocated while off
    int diag = 0;                    // on for the next warps
    int warp_diag = 0;               // ... in effect at the last warp
    int dl_diag = 0;                 // ... downloaded by the last solve call
    void* dgn = nullptr;             // device: [batch] fold maps u8[N], then [batch] DiagAcc, then [batch] ArapFlow_MeshStats
    size_t dgn_fold_slot = 0;
    DiagAcc* dgn_acc = nullptr;
    ArapFlow_MeshStats* dgn_stats = nullptr;
    char* pin_diag = nullptr;        // [batch] x {ArapFlow_MeshStats (256 bytes), fold u8[N]}   (allocated on first download)
    size_t pin_diag_slot = 0;
};

// pinned staging of the snapshot downloads (as solver_pin_out: when first needed)
static void solver_pin_mid(ArapFlow_Solver* s)
{
    if (s->pin_mid) return;
    s->pin_mid_slot = align_up(20 * (size_t)s->N, 256);
    HC(hipHostMalloc((void**)&s->pin_mid, s->pin_mid_slot * s->mid_cap * s->batch, hipHostMallocDefault));
}
// device buffers of `n` snapshots: 8 B per vertex, snapshot and slot for the state, 20 B for the four outputs
static void solver_mid_alloc(ArapFlow_Solver* s, unsigned n)
{
    if (n <= s->mid_cap) return;
    HC(hipSetDevice(s->st->device));
    if (s->mid) HC(hipFree(s->mid));
    if (s->pin_mid_jobs) HC(hipHostFree(s->pin_mid_jobs));
    if (s->pin_mid) HC(hipHostFree(s->pin_mid));
    s->pin_mid = nullptr;
    const size_t N = s->N, B = s->batch;
    const size_t sz2 = align_up(8 * N, 256), sz3 = align_up(3 * N, 256), szb = align_up(N, 256);
    const size_t per = 3 * sz2 + sz3 + szb, jobs = align_up(sizeof(WarpJob) * n * B, 256);
    HC(hipMalloc(&s->mid, per * n * B + jobs));
    HC(hipMemsetAsync(s->mid, 0, per * n * B + jobs, s->st->stream));
    char* c = (char*)s->mid;
    auto take = [&](size_t b) { char* r = c; c += b; return r; };
    s->hmid.resize(n * B);
    for (MidDev& m : s->hmid) {
        m.state = (float2*)take(sz2); m.flow = (float2*)take(sz2); m.step = (float2*)take(sz2);
        m.rgb = (uint8_t*)take(sz3); m.mask = (uint8_t*)take(szb);
    }
    s->dmid_jobs = (WarpJob*)c;
    HC(hipHostMalloc((void**)&s->pin_mid_jobs, sizeof(WarpJob) * n * B, hipHostMallocDefault));
    HC(hipStreamSynchronize(s->st->stream));
    s->mid_cap = n;
    s->taken_n = s->warp_snap_n = s->dl_snap_n = 0;
    if (s->st->own_stream) solver_pin_mid(s);   // (as pin_out: downloads will be asked for)
}

static void solver_enqueue_warp(ArapFlow_Solver* s, unsigned nframes)
{
    Opt_State* st = s->st;
    WarpJob* jobs = s->pin_jobs;             // (pinned: see plan_gn_step on pageable sources)
    for (unsigned b = 0; b < nframes; ++b) {
        const FrameDev& f = s->hfr[b];
        WarpJob& j = jobs[b];
        j.field = f.O; j.flow_in = nullptr;
        j.rgb = s->has_rgb[b] ? f.rgb : nullptr;
        j.mask = f.mask; j.flow_out = f.flow; j.key = f.key;
        j.out_rgb = s->has_rgb[b] ? f.out_rgb : nullptr;
        j.out_mask = f.out_mask;
        const int o = s->outputs;
        const FrameExt* e = o ? &s->hext[b] : nullptr;
        j.bwd = (o & ARAPFLOW_OUT_BACKWARD) ? e->bwd : nullptr;
        j.occ_bwd = (o & ARAPFLOW_OUT_BACKWARD) ? e->occ_bwd : nullptr;
        j.occ = (o & ARAPFLOW_OUT_OCCLUSION) ? e->occ : nullptr;
        j.cell = e ? e->cell : nullptr; j.rank = e ? e->rank : nullptr; j.bin = e ? e->bin : nullptr;
        j.fold = s->diag ? (uint8_t*)s->dgn + s->dgn_fold_slot * b : nullptr;
        j.acc = s->diag ? s->dgn_acc + b : nullptr;
        j.stats = s->diag ? s->dgn_stats + b : nullptr;
    }
    HC(hipMemcpyAsync(s->djobs, jobs, sizeof(WarpJob) * nframes, hipMemcpyHostToDevice, st->stream));
    enqueue_warp(st->stream, s->djobs, nframes, s->W, s->H, s->outputs, s->ext_cells, s->ext_cell_slot * nframes);
    s->warp_outputs = s->outputs;
    if (s->diag) enqueue_warp_diag(st->stream, s->djobs, nframes, s->W, s->H, s->dgn_acc, sizeof(DiagAcc) * nframes);
    s->warp_diag = s->diag;
    // the in-between frames of the last solve: one warp pass per snapshot over the slots, on the field S_{i_k}, with the
    // step towards the next state; the slot's key image serves every pass (k_warp_resolve left it cleared)
    const unsigned n = s->taken_n;
    s->warp_snap_n = n;
    if (n == 0) return;
    WarpJob* mj = s->pin_mid_jobs;
    for (unsigned k = 0; k < n; ++k)
        for (unsigned b = 0; b < nframes; ++b) {
            const FrameDev& f = s->hfr[b];
            const MidDev& m = s->hmid[(size_t)k * s->batch + b];
            WarpJob j{};
            j.field = m.state;
            j.rgb = s->has_rgb[b] ? f.rgb : nullptr;
            j.mask = f.mask; j.flow_out = m.flow; j.key = f.key;
            j.out_rgb = s->has_rgb[b] ? m.rgb : nullptr;
            j.out_mask = m.mask;
            j.field_b = k + 1 < n ? s->hmid[(size_t)(k + 1) * s->batch + b].state : f.O;
            j.step = m.step;
            mj[(size_t)k * nframes + b] = j;
        }
    HC(hipMemcpyAsync(s->dmid_jobs, mj, sizeof(WarpJob) * n * nframes, hipMemcpyHostToDevice, st->stream));
    for (unsigned k = 0; k < n; ++k)
        enqueue_warp(st->stream, s->dmid_jobs + (size_t)k * nframes, nframes, s->W, s->H, 0, nullptr, 0, true);
}

// pinned staging of the downloads, allocated when first needed: at creation / SetOutputs in the asynchronous use
// (hipHostMalloc waits for the device, i.e. for another solver object's running solve), else at the first download
static void solver_pin_out(ArapFlow_Solver* s)
{
    if (s->pin_out) return;
    s->pin_out_slot = align_up(12 * (size_t)s->N, 256);
    HC(hipHostMalloc((void**)&s->pin_out, s->pin_out_slot * s->batch, hipHostMallocDefault));
}
static void solver_pin_ext(ArapFlow_Solver* s)
{
    if (s->pin_ext) return;
    s->pin_ext_slot = align_up(10 * (size_t)s->N, 256);
    HC(hipHostMalloc((void**)&s->pin_ext, s->pin_ext_slot * s->batch, hipHostMallocDefault));
}

static void solver_pin_diag(ArapFlow_Solver* s)
{
    if (s->pin_diag) return;
    s->pin_diag_slot = 256 + align_up((size_t)s->N, 256);
    HC(hipHostMalloc((void**)&s->pin_diag, s->pin_diag_slot * s->batch, hipHostMallocDefault));
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
                    HC(hipMemcpyAsync(s->hmid[(size_t)k * s->batch + b].state, s->hfr[b].O, sizeof(float2) * s->N,
                                      hipMemcpyDeviceToDevice, st->stream));
    }
    s->taken_n = s->a_snap_n;
    if (s->a_warp) solver_enqueue_warp(s, nframes);
    if (p->res_capable) {
        *s->pin_err = 0u;
        HC(hipMemcpyAsync(s->pin_err, p->rd.err, sizeof(unsigned), hipMemcpyDeviceToHost, st->stream));
    }
    HC(hipEventRecord(s->ev_done, st->stream));
    if (s->a_download) {
        solver_pin_out(s);
        HC(hipStreamWaitEvent(s->copy, s->ev_done, 0));
        const size_t N = s->N;
        for (unsigned b = 0; b < nframes; ++b) {
            const FrameDev& f = s->hfr[b];
            char* o = s->pin_out + s->pin_out_slot * b;
            HC(hipMemcpyAsync(o, f.flow, 8 * N, hipMemcpyDeviceToHost, s->copy));
            if (s->has_rgb[b]) HC(hipMemcpyAsync(o + 8 * N, f.out_rgb, 3 * N, hipMemcpyDeviceToHost, s->copy));
            HC(hipMemcpyAsync(o + 11 * N, f.out_mask, N, hipMemcpyDeviceToHost, s->copy));
        }
        s->dl_outputs = s->a_warp ? s->outputs : 0;
        if (s->dl_outputs) {
            solver_pin_ext(s);
            for (unsigned b = 0; b < nframes; ++b) {
                const FrameExt& e = s->hext[b];
                char* o = s->pin_ext + s->pin_ext_slot * b;
                if (s->dl_outputs & ARAPFLOW_OUT_BACKWARD) {
                    HC(hipMemcpyAsync(o, e.bwd, 8 * N, hipMemcpyDeviceToHost, s->copy));
                    HC(hipMemcpyAsync(o + 8 * N, e.occ_bwd, N, hipMemcpyDeviceToHost, s->copy));
                }
                if (s->dl_outputs & ARAPFLOW_OUT_OCCLUSION)
                    HC(hipMemcpyAsync(o + 9 * N, e.occ, N, hipMemcpyDeviceToHost, s->copy));
            }
        }
        s->dl_diag = s->a_warp ? s->diag : 0;
        if (s->dl_diag) {
            solver_pin_diag(s);
            for (unsigned b = 0; b < nframes; ++b) {
                char* o = s->pin_diag + s->pin_diag_slot * b;
                HC(hipMemcpyAsync(o, s->dgn_stats + b, sizeof(ArapFlow_MeshStats), hipMemcpyDeviceToHost, s->copy));
                HC(hipMemcpyAsync(o + 256, (uint8_t*)s->dgn + s->dgn_fold_slot * b, N, hipMemcpyDeviceToHost, s->copy));
            }
        }
        s->dl_snap_n = s->a_warp ? s->taken_n : 0;
        if (s->dl_snap_n) {
            solver_pin_mid(s);
            for (unsigned k = 0; k < s->dl_snap_n; ++k)
                for (unsigned b = 0; b < nframes; ++b) {
                    const size_t kb = (size_t)k * s->batch + b;
                    const MidDev& m = s->hmid[kb];
                    char* o = s->pin_mid + s->pin_mid_slot * kb;
                    HC(hipMemcpyAsync(o, m.flow, 8 * N, hipMemcpyDeviceToHost, s->copy));
                    HC(hipMemcpyAsync(o + 8 * N, m.step, 8 * N, hipMemcpyDeviceToHost, s->copy));
                    if (s->has_rgb[b]) HC(hipMemcpyAsync(o + 16 * N, m.rgb, 3 * N, hipMemcpyDeviceToHost, s->copy));
                    HC(hipMemcpyAsync(o + 19 * N, m.mask, N, hipMemcpyDeviceToHost, s->copy));
                }
        }
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
    const size_t sz2 = align_up(N * sizeof(float2), 256), sz1 = align_up(N * sizeof(float), 256);
    const size_t szb = align_up(N, 256), sz3 = align_up(3 * N, 256), szk = align_up(N * 8, 256);
    const size_t per = 5 * sz2 + 2 * sz1 + 2 * szb + 2 * sz3 + szk;
    const size_t tail = align_up(sizeof(FrameDev) * batch, 256) + align_up(sizeof(WarpJob) * batch, 256);
    HC(hipMalloc(&s->block, per * batch + tail));
    HC(hipMemsetAsync(s->block, 0, per * batch + tail, st->stream));
    char* c = (char*)s->block;
    auto take = [&](size_t b) { char* r = c; c += b; return r; };
    s->hfr.resize(batch);
    for (unsigned b = 0; b < batch; ++b) {
        FrameDev& f = s->hfr[b];
        f.O = (float2*)take(sz2); f.U = (float2*)take(sz2); f.C = (float2*)take(sz2);
        f.T = (float2*)take(sz2); f.flow = (float2*)take(sz2);
        f.A = (float*)take(sz1); f.M = (float*)take(sz1);
        f.mask = (uint8_t*)take(szb); f.out_mask = (uint8_t*)take(szb);
        f.rgb = (uint8_t*)take(sz3); f.out_rgb = (uint8_t*)take(sz3);
        f.key = (unsigned long long*)take(szk);
    }
    s->dfr = (FrameDev*)take(align_up(sizeof(FrameDev) * batch, 256));
    s->djobs = (WarpJob*)take(align_up(sizeof(WarpJob) * batch, 256));
    HC(hipMemcpyAsync(s->dfr, s->hfr.data(), sizeof(FrameDev) * batch, hipMemcpyHostToDevice, st->stream));
    HC(hipStreamSynchronize(st->stream));
    HC(hipStreamCreateWithFlags(&s->copy, hipStreamNonBlocking));
    HC(hipEventCreateWithFlags(&s->ev_up, hipEventDisableTiming));
    HC(hipEventCreateWithFlags(&s->ev_done, hipEventDisableTiming));
    HC(hipEventCreateWithFlags(&s->ev_dl, hipEventDisableTiming));
    s->pin_in_slot = align_up(12 * N, 256);
    HC(hipHostMalloc((void**)&s->pin_in, s->pin_in_slot * batch, hipHostMallocDefault));
    // (allocated here, not at first use: hipHostMalloc waits for the device, i.e. for another solver object's running solve)
    HC(hipHostMalloc((void**)&s->pin_jobs, sizeof(WarpJob) * batch, hipHostMallocDefault));
    HC(hipHostMalloc((void**)&s->pin_err, 64, hipHostMallocDefault));
    if (st->own_stream) solver_pin_out(s);   // the asynchronous use (ArapFlow_UseOwnStream first): downloads will be asked for
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
    if (s->pin_out) (void)hipHostFree(s->pin_out);
    if (s->pin_jobs) (void)hipHostFree(s->pin_jobs);
    if (s->pin_err) (void)hipHostFree(s->pin_err);
    if (s->pin_ext) (void)hipHostFree(s->pin_ext);
    if (s->ext) (void)hipFree(s->ext);
    if (s->mid) (void)hipFree(s->mid);
    if (s->pin_mid_jobs) (void)hipHostFree(s->pin_mid_jobs);
    if (s->pin_mid) (void)hipHostFree(s->pin_mid);
    if (s->dgn) (void)hipFree(s->dgn);
    if (s->pin_diag) (void)hipHostFree(s->pin_diag);
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
    uint8_t* smask = (uint8_t*)(stage + 8 * N);
    uint8_t* srgb = (uint8_t*)(stage + 9 * N);
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
    if (s->snap_n && s->snap_steps[s->snap_n - 1] > numIter) return -1;     // (increasing: the last is the largest)
    if (ArapFlow_SolverWait(s) != 0) return -1;
    Opt_State* st = s->st;
    HC(hipSetDevice(st->device));
    s->a_snap_n = s->snap_n;
    memcpy(s->a_snap_steps, s->snap_steps, sizeof(s->snap_steps));
    solver_mid_alloc(s, s->snap_n);                           // (the first solve that needs it; nothing with none)
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
        const size_t rank_bytes = L.bin - L.rank, bin_bytes = L.owner - L.bin;
        const size_t per = align_up(8 * N, 256) + 2 * align_up(N, 256) + rank_bytes + bin_bytes;
        s->ext_cell_slot = L.rank - L.cell;
        HC(hipMalloc(&s->ext, (per + s->ext_cell_slot) * s->batch));
        HC(hipMemsetAsync(s->ext, 0, (per + s->ext_cell_slot) * s->batch, s->st->stream));
        char* c = (char*)s->ext;
        auto take = [&](size_t b) { char* r = c; c += b; return r; };
        s->hext.resize(s->batch);
        for (int b = 0; b < s->batch; ++b) {
            FrameExt& e = s->hext[b];
            e.bwd = (float2*)take(align_up(8 * N, 256));
            e.occ_bwd = (uint8_t*)take(align_up(N, 256)); e.occ = (uint8_t*)take(align_up(N, 256));
            e.rank = (unsigned*)take(rank_bytes); e.bin = (int4*)take(bin_bytes);
        }
        s->ext_cells = (unsigned*)c;
        for (int b = 0; b < s->batch; ++b) s->hext[b].cell = (unsigned*)take(s->ext_cell_slot);
        HC(hipStreamSynchronize(s->st->stream));
        if (s->st->own_stream) solver_pin_ext(s);   // (as pin_out: downloads will be asked for)
    }
    s->outputs = which;
    return 0;
}

int ArapFlow_SolverSetSnapshots(ArapFlow_Solver* s, const unsigned* steps, unsigned n)
{
    if (!s || n > ARAPFLOW_MAX_SNAPSHOTS || (n && !steps)) return -1;
    for (unsigned k = 0; k < n; ++k)
        if (steps[k] < 1 || (k && steps[k] <= steps[k - 1])) return -1;
    if (const int rc = ArapFlow_SolverWait(s)) return rc;
    s->snap_n = n;
    for (unsigned k = 0; k < n; ++k) s->snap_steps[k] = steps[k];
    return 0;
}

int ArapFlow_SolverGetSnapshot(ArapFlow_Solver* s, unsigned slot, unsigned k, float* flow, uint8_t* rgb, uint8_t* mask,
                               float* step)
{
    if (!s || slot >= (unsigned)s->batch) return -1;
    if (ArapFlow_SolverWait(s) != 0) return -1;
    if (k >= s->warp_snap_n || (rgb && !s->has_rgb[slot])) return -1;
    HC(hipStreamSynchronize(s->st->stream));
    const MidDev& m = s->hmid[(size_t)k * s->batch + slot];
    const size_t N = s->N;
    hipStream_t cs = s->copy;
    if (flow) HC(hipMemcpyAsync(flow, m.flow, 8 * N, hipMemcpyDeviceToHost, cs));
    if (rgb) HC(hipMemcpyAsync(rgb, m.rgb, 3 * N, hipMemcpyDeviceToHost, cs));
    if (mask) HC(hipMemcpyAsync(mask, m.mask, N, hipMemcpyDeviceToHost, cs));
    if (step) HC(hipMemcpyAsync(step, m.step, 8 * N, hipMemcpyDeviceToHost, cs));
    HC(hipStreamSynchronize(cs));
    return 0;
}

int ArapFlow_SolverHostSnapshot(ArapFlow_Solver* s, unsigned slot, unsigned k, const float** flow, const uint8_t** rgb,
                                const uint8_t** mask, const float** step)
{
    if (!s || slot >= (unsigned)s->batch || !s->a_download || slot >= s->a_n) return -1;
    if (ArapFlow_SolverWait(s) != 0) return -1;
    if (k >= s->dl_snap_n || !s->pin_mid) return -1;
    const size_t N = s->N;
    const char* o = s->pin_mid + s->pin_mid_slot * ((size_t)k * s->batch + slot);
    if (flow) *flow = (const float*)o;
    if (step) *step = (const float*)(o + 8 * N);
    if (rgb) *rgb = s->has_rgb[slot] ? (const uint8_t*)(o + 16 * N) : nullptr;
    if (mask) *mask = (const uint8_t*)(o + 19 * N);
    return 0;
}

int ArapFlow_SolverGetExtraResults(ArapFlow_Solver* s, unsigned slot, float* bwd, uint8_t* occ_bwd, uint8_t* occ)
{
    if (!s || slot >= (unsigned)s->batch) return -1;
    if (ArapFlow_SolverWait(s) != 0) return -1;
    if (((bwd || occ_bwd) && !(s->warp_outputs & ARAPFLOW_OUT_BACKWARD)) ||
        (occ && !(s->warp_outputs & ARAPFLOW_OUT_OCCLUSION)))
        return -1;
    HC(hipStreamSynchronize(s->st->stream));
    const FrameExt& e = s->hext[slot];
    const size_t N = s->N;
    hipStream_t cs = s->copy;
    if (bwd) HC(hipMemcpyAsync(bwd, e.bwd, 8 * N, hipMemcpyDeviceToHost, cs));
    if (occ_bwd) HC(hipMemcpyAsync(occ_bwd, e.occ_bwd, N, hipMemcpyDeviceToHost, cs));
    if (occ) HC(hipMemcpyAsync(occ, e.occ, N, hipMemcpyDeviceToHost, cs));
    HC(hipStreamSynchronize(cs));
    return 0;
}

int ArapFlow_SolverHostExtraResults(ArapFlow_Solver* s, unsigned slot, const float** bwd, const uint8_t** occ_bwd,
                                    const uint8_t** occ)
{
    if (!s || slot >= (unsigned)s->batch || !s->a_download || slot >= s->a_n) return -1;
    if (ArapFlow_SolverWait(s) != 0) return -1;
    if (!s->dl_outputs || !s->pin_ext) return -1;
    const size_t N = s->N;
    const char* o = s->pin_ext + s->pin_ext_slot * slot;
    const bool b = s->dl_outputs & ARAPFLOW_OUT_BACKWARD, c = s->dl_outputs & ARAPFLOW_OUT_OCCLUSION;
    if (bwd) *bwd = b ? (const float*)o : nullptr;
    if (occ_bwd) *occ_bwd = b ? (const uint8_t*)(o + 8 * N) : nullptr;
    if (occ) *occ = c ? (const uint8_t*)(o + 9 * N) : nullptr;
    return 0;
}

int ArapFlow_SolverSetDiag(ArapFlow_Solver* s, int on)
{
    if (!s) return -1;
    if (const int rc = ArapFlow_SolverWait(s)) return rc;
    if (on && !s->dgn) {
        HC(hipSetDevice(s->st->device));
        const size_t B = s->batch;
        s->dgn_fold_slot = align_up((size_t)s->N, 256);
        const size_t accs = align_up(sizeof(DiagAcc) * B, 256), stats = align_up(sizeof(ArapFlow_MeshStats) * B, 256);
        HC(hipMalloc(&s->dgn, s->dgn_fold_slot * B + accs + stats));
        s->dgn_acc = (DiagAcc*)((char*)s->dgn + s->dgn_fold_slot * B);
        s->dgn_stats = (ArapFlow_MeshStats*)((char*)s->dgn_acc + accs);
        if (s->st->own_stream) solver_pin_diag(s);   // (as pin_out: downloads will be asked for)
    }
    s->diag = on ? 1 : 0;
    return 0;
}

int ArapFlow_SolverGetDiag(ArapFlow_Solver* s, unsigned slot, ArapFlow_MeshStats* stats, uint8_t* fold)
{
    if (!s || slot >= (unsigned)s->batch) return -1;
    if (ArapFlow_SolverWait(s) != 0) return -1;
    if (!s->warp_diag) return -1;
    HC(hipStreamSynchronize(s->st->stream));
    hipStream_t cs = s->copy;
    if (stats) HC(hipMemcpyAsync(stats, s->dgn_stats + slot, sizeof(ArapFlow_MeshStats), hipMemcpyDeviceToHost, cs));
    if (fold) HC(hipMemcpyAsync(fold, (uint8_t*)s->dgn + s->dgn_fold_slot * slot, (size_t)s->N, hipMemcpyDeviceToHost, cs));
    HC(hipStreamSynchronize(cs));
    return 0;
}

int ArapFlow_SolverHostDiag(ArapFlow_Solver* s, unsigned slot, const ArapFlow_MeshStats** stats, const uint8_t** fold)
{
    if (!s || slot >= (unsigned)s->batch || !s->a_download || slot >= s->a_n) return -1;
    if (ArapFlow_SolverWait(s) != 0) return -1;
    if (!s->dl_diag || !s->pin_diag) return -1;
    const char* o = s->pin_diag + s->pin_diag_slot * slot;
    if (stats) *stats = (const ArapFlow_MeshStats*)o;
    if (fold) *fold = (const uint8_t*)(o + 256);
    return 0;
}

int ArapFlow_SolverHostResults(ArapFlow_Solver* s, unsigned slot, const float** flow, const uint8_t** warped_rgb,
                               const uint8_t** warped_mask)
{
    if (!s || slot >= (unsigned)s->batch || !s->pin_out || !s->a_download || slot >= s->a_n) return -1;
    if (ArapFlow_SolverWait(s) != 0) return -1;
    const size_t N = s->N;
    const char* o = s->pin_out + s->pin_out_slot * slot;
    if (flow) *flow = (const float*)o;
    if (warped_rgb) *warped_rgb = s->has_rgb[slot] ? (const uint8_t*)(o + 8 * N) : nullptr;
    if (warped_mask) *warped_mask = (const uint8_t*)(o + 11 * N);
    return 0;
}

int ArapFlow_SolverGetResults(ArapFlow_Solver* s, unsigned slot, float* flow, uint8_t* warped_rgb,
                              uint8_t* warped_mask, float* offset, float* angle, double* final_cost)
{
    if (!s || slot >= (unsigned)s->batch) return -1;
    if (ArapFlow_SolverWait(s) != 0) return -1;
    HC(hipStreamSynchronize(s->st->stream));
    plan_check_resident_error(s->plan);
    const FrameDev& f = s->hfr[slot];
    const size_t N = s->N;
    hipStream_t cs = s->copy;
    if (flow) HC(hipMemcpyAsync(flow, f.flow, N * sizeof(float2), hipMemcpyDeviceToHost, cs));
    if (warped_rgb) HC(hipMemcpyAsync(warped_rgb, f.out_rgb, 3 * N, hipMemcpyDeviceToHost, cs));
    if (warped_mask) HC(hipMemcpyAsync(warped_mask, f.out_mask, N, hipMemcpyDeviceToHost, cs));
    if (offset) HC(hipMemcpyAsync(offset, f.O, N * sizeof(float2), hipMemcpyDeviceToHost, cs));
    if (angle) HC(hipMemcpyAsync(angle, f.A, N * sizeof(float), hipMemcpyDeviceToHost, cs));
    HC(hipStreamSynchronize(cs));
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
int ArapFlow_ResidentFailed(Opt_State* state) { return state && state->resident_failed ? 1 : 0; }
int ArapFlow_SolverLeanStream(ArapFlow_Solver* s) { return s && plan_lean_stream(s->plan) ? 1 : 0; }

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
