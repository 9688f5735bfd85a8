// host_step.h -- one Gauss-Newton step of a gaussNewtonGPU plan: the StepRecipe (what a step launches, decided once),
// the enqueue of a step from it, the graph cache keyed by it, the cost kernel, and plan_init / plan_step /
// plan_steps_batched on top.
#pragma once

static bool plan_active_tiles_majority(const Opt_Plan* p)
{
    long act = 0;
    for (int b = 0; b < p->nb; ++b) act += p->h_ntiles[b];
    const long all = (long)((p->W + RT_X - 1) / RT_X) * ((p->H + RT_Y - 1) / RT_Y);
    return 2 * act >= (long)p->nb * all;
}

// The lean streaming schedule (arap_stream.h: k_pcg_a_march2 / k_pcg_b4_r, 126 instead of 146 B per vertex and
// iteration): frame-solver plans only (nothing else reads z or an up-to-date delta between the two phases), pixel-grid
// UrShape, Gauss-Newton, 16-byte alignment of every frame's images -- and most tiles active: its phase A carries more
// loads per stage, which pays where the rows are full (1920x1080 mask == 0: 94.2 -> 86.3 ms per 4 x 400 iterations; eight
// 854x480 mask == 0 frames: 167.5 -> 138.9) and loses on sparse masks (eight DAVIS-shaped frames: 75.9 -> 80.0).
// ARAPOPT_STREAM_A=2 keeps the round-2 pair.
static bool plan_lean_stream(const Opt_Plan* p)
{
    return p->res_frames_any && p->grid_u && !p->pd.lm && p->st->tile < 0 && (p->N & 3) == 0 && !p->st->force_b8 &&
           p->st->stream_a == 0 && plan_active_tiles_majority(p);
}

// Grid of the list launches (k_gn_prep / k_gn_init / k_gn_update over the frames' active 64x4 tiles): the longest list,
// rounded up to a multiple of 64 workgroups so that batches of similar frames replay the same captured graph (a
// workgroup beyond its frame's list only reports a zero to the order-fixed sums).
static int plan_list_blocks(const Opt_Plan* p)
{
    int maxn = 1;
    for (int k = 0; k < p->nb; ++k) maxn = std::max(maxn, p->h_t64n[k]);
    return std::min((maxn + 63) / 64 * 64, p->pd.tilesX * p->pd.tilesY);
}

// 4-row blocks a workgroup of the marching phase-A kernels walks through: 5 for the round-2 pair, 7 for the lean schedule,
// whose phase A holds more loads per stage (84 VGPRs: 5 workgroups per CU) -- 30 x 39 = 1170 workgroups at 1920x1080 are
// all resident at once with 7 blocks, 1624 with 5 are not (sweep 3 / 5 / 6 / 7 / 8 / 10: 46.6 / 43.8 / 44.5 / 38.4 / 38.6 /
// 42.2 us)
constexpr int MARCH_ROWS = 5, MARCH2_ROWS = 7;

// Every decision about the next `nsteps` Gauss-Newton steps of the current batch (p->nb slots, p->sp.lIterations).
// On the resident path this deals the batch's solves to launches and workgroups first (their number and slot counts
// are part of the recipe) and uploads the tables when the deal changed.
static StepRecipe plan_step_recipe(Opt_Plan* p, int nsteps)
{
    const Opt_State* st = p->st;
    StepRecipe r;
    r.resident = plan_resident_eligible(p);
    r.L = p->sp.lIterations;
    r.nb = p->nb;
    r.nsteps = nsteps;
    if (r.resident) {
        if (plan_resident_pack(p)) plan_upload_wgmap(p);
        r.res_ns = p->res_ns;
        r.res_sums = p->res_sums;
        r.stamped = p->rd.stamps != nullptr;
        // Frame solver: the resident launch applies the step itself (X += delta, cos/sin of the new Angle:
        // ResDev::fuse_update) and the init kernel zeroes the granules, so a step is [init, resident launches] and a lone
        // k_gn_prep (flags, tile activity) runs only where no step came before (the first step after the ramp moved the
        // constraints, or after a step on another path): Opt_Plan::prep_done.
        // (not in a verbose solve: that one checks every step by itself and redoes a failed step alone, which needs the
        //  step's update left undone)
        if (p->res_frames && st->verbosity == 0) r.part = GN_STEP_FUSED;
        // ... and its per-step kernels visit the frames' active 64x4 tiles only
        if (p->res_frames && p->d_t64list != nullptr) r.list_blocks = plan_list_blocks(p);
        return r;
    }
    // phase A: direct-load kernel, an LDS-staged tile shape (ArapFlow_SetTile) or a streaming kernel
    const bool lean = plan_lean_stream(p);
    int v = st->tile;
    if (v < 0 && p->grid_u && !p->pd.lm) {
        // default for the pixel-grid UrShape (every frame-solver plan): the marching kernel of arap_stream.h -- no
        // UrShape loads, every vertex fetched once, XCD-aware strip order; 1-D launch of frames x 8 x ceil(tiles / 8)
        if (st->stream_a == 1) {
            constexpr int TX = 64, TY = 8;
            const int tX = (p->W + TX - 1) / TX, tY = (p->H + TY - 1) / TY, ch = (tX * tY + 7) / 8;
            r.a_kern = PA_GRID;
            r.a_grid = dim3((unsigned)(p->nb * 8 * ch));
            r.a_block = dim3(TX, TY, 1);
            r.a_arg[0] = tX; r.a_arg[1] = tY; r.a_arg[2] = ch;
        } else {
            const int rows = 4 * (lean ? MARCH2_ROWS : MARCH_ROWS);
            const int sX = p->pd.tilesX, cY = (p->H + rows - 1) / rows, chunk = (sX * cY + 7) / 8;
            r.a_kern = lean ? PA_MARCH2 : PA_MARCH;
            r.a_grid = dim3((unsigned)(p->nb * 8 * chunk));
            r.a_block = dim3(256);
            r.a_arg[0] = sX; r.a_arg[1] = cY; r.a_arg[2] = chunk;
        }
    } else {
        // generic UrShape: LDS-staged 64x8 tiles when most tiles are active (profiles/r01_tile_sweep_two_kernel_path.txt:
        // +14 % at full masks), direct loads for sparse masks (the staging of empty halo rows does not pay)
        if (v < 0) v = plan_active_tiles_majority(p) ? 5 : 0;
        r.a_kern = PA_DIRECT + v;
        if (v == 0) {
            r.a_grid = p->grid();
            r.a_block = p->blk();
        } else {
            const int TX = kTileShapes[v][0], TY = kTileShapes[v][1];
            r.a_grid = dim3((p->W + TX - 1) / TX, (p->H + TY - 1) / TY, p->nb);
            r.a_block = dim3(TX, TY, 1);
        }
    }
    // phase B: 16-byte accesses need every frame's images 16-byte aligned
    if ((p->N & 3) == 0 && !p->pd.lm && !st->force_b8)
        r.b_kern = lean ? PB_B4_R : (st->tile < 0 ? PB_B4_LEAN : PB_B4);       // (explicit variants: the sweep's baseline)
    else
        r.b_kern = PB_B;
    // (the lean streaming schedule leaves the last iteration's delta += alpha p to the update kernel)
    if (r.L > 0 && lean) r.lag = r.L - 1;
    return r;
}

static void launch_pcg_a(Opt_Plan* p, hipStream_t s, const StepRecipe& r, int l)
{
    const dim3 g = r.a_grid, b = r.a_block;
    const int* a = r.a_arg;
    switch (r.a_kern) {
    case PA_DIRECT: LAUNCH(p, s, "PCGStepA", k_pcg_a, g, b, 0, p->pd, l); break;
    case PA_LDS_16x16: LAUNCH(p, s, "PCGStepA", (k_pcg_a_lds<16, 16>), g, b, 0, p->pd, l); break;
    case PA_LDS_32x8: LAUNCH(p, s, "PCGStepA", (k_pcg_a_lds<32, 8>), g, b, 0, p->pd, l); break;
    case PA_LDS_64x4: LAUNCH(p, s, "PCGStepA", (k_pcg_a_lds<64, 4>), g, b, 0, p->pd, l); break;
    case PA_LDS_32x16: LAUNCH(p, s, "PCGStepA", (k_pcg_a_lds<32, 16>), g, b, 0, p->pd, l); break;
    case PA_LDS_64x8: LAUNCH(p, s, "PCGStepA", (k_pcg_a_lds<64, 8>), g, b, 0, p->pd, l); break;
    case PA_MARCH: LAUNCH(p, s, "PCGStepA", (k_pcg_a_march<MARCH_ROWS>), g, b, 0, p->pd, l, a[0], a[1], a[2]); break;
    case PA_MARCH2: LAUNCH(p, s, "PCGStepA", (k_pcg_a_march2<MARCH2_ROWS>), g, b, 0, p->pd, l, a[0], a[1], a[2]); break;
    case PA_GRID: LAUNCH(p, s, "PCGStepA", (k_pcg_a_grid<64, 8>), g, b, 0, p->pd, l, a[0], a[1], a[2]); break;
    }
}

static void launch_pcg_b(Opt_Plan* p, hipStream_t s, const StepRecipe& r, int l)
{
    const dim3 gq((p->N / 4 + 255) / 256, r.nb, 1);
    switch (r.b_kern) {
    case PB_B: LAUNCH(p, s, "PCGStepB", k_pcg_b, dim3(p->pd.tilesX, p->pd.tilesY, r.nb), p->blk(), 0, p->pd, l); break;
    case PB_B4: LAUNCH(p, s, "PCGStepB", k_pcg_b4, gq, dim3(256), 0, p->pd, l); break;
    case PB_B4_LEAN: LAUNCH(p, s, "PCGStepB", k_pcg_b4_lean, gq, dim3(256), 0, p->pd, l); break;
    case PB_B4_R: LAUNCH(p, s, "PCGStepB", k_pcg_b4_r, gq, dim3(256), 0, p->pd, l); break;
    }
}

// enqueue the kernels of one Gauss-Newton step (without the cost) on stream s, as the recipe says
// part: r.part (GN_STEP_ALL = prep, init, PCG, update;  GN_STEP_FUSED = lean init, resident launch(es) that apply the
// step themselves) or GN_STEP_PREP = the lone prep in front of fused steps
static void enqueue_gn_step(Opt_Plan* p, hipStream_t s, const StepRecipe& r, int part)
{
    const int L = r.L;
    const dim3 g(p->pd.tilesX, p->pd.tilesY, r.nb), b = p->blk();
    PlanDev pd = p->pd;
    const size_t gran_per_launch = RES_GRAN_PER_LAUNCH;                  // u64 entries
    if (r.resident) {
        // k_gn_prep zeroes slot 0 of `red` (rho_0) and the granules of every launch of this step: no memset nodes.
        // Granule tags restart at 1 in every launch (cdna guide G16 "re-initialise every call").
        pd.res_gran = p->rd.gran;
        pd.res_gran_n = (int)(gran_per_launch * r.res_ns.size());
    } else {
        // reduction slots 0 .. 2L of every active frame (contiguous because slot stride is nslots)
        HC(hipMemsetAsync(p->pd.red, 0, (size_t)r.nb * p->pd.nslots * NSHARD * sizeof(double), s));
    }
    // frame solver on the resident path: the per-step kernels visit the frames' active 64x4 tiles only
    PlanDev pdl = p->pd;
    dim3 gl = g;
    if (r.list_blocks > 0) {
        pd.t64list = pdl.t64list = p->d_t64list;
        pd.t64n = pdl.t64n = p->d_t64n;
        gl = dim3((unsigned)r.list_blocks, 1, (unsigned)r.nb);
    }
    if (part != GN_STEP_FUSED) LAUNCH(p, s, "GNPrep", k_gn_prep, gl, b, 0, pd);
    if (part == GN_STEP_PREP) return;
    // (frame solver on the resident path: no UrShape loads, no stores of what the resident kernel does not read)
    // (... and it zeroes the granules of the launches that follow: pd carries them)
    if (part == GN_STEP_FUSED) LAUNCH(p, s, "PCGInit1", k_gn_init_resf, gl, b, 0, pd);
    else LAUNCH(p, s, "PCGInit1", k_gn_init, gl, b, 0, pdl);
    if (r.resident) {
        // all L iterations in one launch, state on chip (arap_resident.h)
        ResDev rd = p->rd;
        rd.fuse_update = part == GN_STEP_FUSED ? 1 : 0;          // frame solver: the launch applies the step itself
        for (size_t set = 0; set < r.res_ns.size(); ++set) {
            rd.wgmap = p->d_wgmap + set * RES_WGS;
            rd.gran = p->rd.gran + gran_per_launch * set;
            // (the flat flavour only ever gets launches whose groups all have <= 64 workgroups: its sweep of a group's
            //  granules covers exactly that many -- plan_resident_pack refuses any other pairing)
            const ResidentKernel kern = (ResidentKernel)resident_kernel(r.stamped, r.res_ns[set], r.res_sums[set]);
            if (r.stamped)
                hipLaunchKernelGGL(kern, dim3(RES_WGS), dim3(RES_THREADS), RES_LDS_BYTES, s, p->pd, rd, L);
            else
                LAUNCH(p, s, "PCGResident", kern, dim3(RES_WGS), dim3(RES_THREADS), RES_LDS_BYTES, p->pd, rd, L);
        }
    } else {
        for (int l = 0; l < L; ++l) {
            launch_pcg_a(p, s, r, l);
            launch_pcg_b(p, s, r, l);
        }
    }
    if (part != GN_STEP_FUSED) LAUNCH(p, s, "PCGLinearUpdate", k_gn_update, gl, b, 0, pdl, r.lag);
}

// nsteps consecutive Gauss-Newton steps (one graph launch: between two graphs the GPU idles 8.6 us, inside one 0.2 us
// per kernel boundary)
static void plan_gn_step(Opt_Plan* p, int nsteps = 1)
{
    Opt_State* st = p->st;
    const StepRecipe r = plan_step_recipe(p, nsteps);
    if (r.resident) p->res_launches += (unsigned)(r.res_ns.size() * nsteps);   // launches executed (graph replays included)
    const bool fused = r.part == GN_STEP_FUSED;
    if (fused && !p->prep_done) enqueue_gn_step(p, st->stream, r, GN_STEP_PREP);
    p->prep_done = fused;
    if (!st->use_graph || st->timing) {
        for (int k = 0; k < nsteps; ++k) enqueue_gn_step(p, st->stream, r, r.part);
        return;
    }
    if (!p->gexec || !same_recipe(r, p->g_recipe)) {
        plan_drop_graph(p);
        HC(hipStreamBeginCapture(st->cap, hipStreamCaptureModeRelaxed));
        for (int k = 0; k < nsteps; ++k) enqueue_gn_step(p, st->cap, r, r.part);
        HC(hipStreamEndCapture(st->cap, &p->graph));
        HC(hipGraphInstantiate(&p->gexec, p->graph, nullptr, nullptr, 0));
        p->g_recipe = r;
    }
    HC(hipGraphLaunch(p->gexec, st->stream));
}

static void plan_cost(Opt_Plan* p, int index)
{
    LAUNCH(p, p->st->stream, "computeCost", k_cost, p->grid(), p->blk(), 0, p->pd, index);
}

// blocking read of the cost entry `index` of slot b (sum of its shards, rounded to float as the
// reference's device float, solverGPUGaussNewton.t:790-797)
static double plan_read_cost(Opt_Plan* p, int b, int index)
{
    double sh[NSHARD];
    HC(hipMemcpyAsync(sh, p->pd.costred + ((size_t)b * p->pd.ncost + index) * NSHARD, sizeof(sh),
                      hipMemcpyDeviceToHost, p->st->stream));
    HC(hipStreamSynchronize(p->st->stream));
    plan_check_resident_error(p);
    double t = 0.0;
    for (int i = 0; i < NSHARD; ++i) t += sh[i];
    return (double)(float)t;
}

// init: solverGPUGaussNewton.t:956-1007
static void plan_init(Opt_Plan* p)
{
    HC(hipSetDevice(p->st->device));
    p->sp.nIter = 0;
    p->prep_done = false;                  // the caller may have changed Mask / Constraints (the ramp does)
    plan_reserve(p, p->sp.lIterations, p->sp.nIterations + 1);
    plan_upload_slots(p);
    if (p->lazy_cost && !p->cost_wanted && p->st->verbosity == 0) return;
    HC(hipMemsetAsync(p->pd.costred, 0, (size_t)p->nb * p->pd.ncost * NSHARD * sizeof(double), p->st->stream));
    if (!p->lazy_cost || p->st->verbosity > 0 || p->sp.nIterations == 0) plan_cost(p, 0);
}

// step: solverGPUGaussNewton.t:1016-1177 (GN branch)
static int plan_step(Opt_Plan* p)
{
    if (p->sp.nIter < p->sp.nIterations) {
        plan_upload_slots(p);
        // the caller may have changed Mask / UrShape since Init or the last Step (Opt.h:58-66)
        // -- looked at before EVERY step, whatever path the step will take: grid_u (no UrShape loads in phase A of the
        // two-kernel path) is a property of the images as they are NOW, also with the resident kernel switched off,
        // paused after a timeout or absent on this device.
        if (!p->res_frames) plan_analyse_for_resident(p);
        const bool used_res = plan_resident_eligible(p);
        plan_gn_step(p);
        if (used_res && (!p->res_frames || p->st->verbosity > 0)) {
            // drop-in plan: the caller may read the unknowns right after this Step, so make sure it happened (a verbose
            // frame solve reads the costs below: same check, instead of at the end of ArapFlow_SolverSolve)
            HC(hipStreamSynchronize(p->st->stream));
            if (plan_resident_failed(p)) plan_gn_step(p);          // X untouched: redo on the two-kernel path
        }
        if (!p->lazy_cost || p->st->verbosity > 0 || (p->cost_wanted && p->sp.nIter + 1 == p->sp.nIterations))
            plan_cost(p, p->sp.nIter + 1);
        if (p->st->verbosity > 0) {
            const double a = plan_read_cost(p, 0, p->sp.nIter), b = plan_read_cost(p, 0, p->sp.nIter + 1);
            printf("cost: %f -> %f\n", a, b);
        }
        p->sp.nIter += 1;
        return 1;
    }
    if (p->st->timing && p->st->verbosity > 0) p->st->ktimer.report();
    return 0;
}

// Frame solver, quiet: all remaining Gauss-Newton steps of the ramp step as ONE graph launch (nothing on the host looks
// at a step's result before the next: the cost is wanted after the last one at most, lazy_cost).  False: not applicable,
// the caller steps one by one.
static bool plan_steps_batched(Opt_Plan* p)
{
    const int n = p->sp.nIterations - p->sp.nIter;
    if (!p->res_frames || !p->lazy_cost || p->st->verbosity > 0 || !p->st->use_graph || p->st->timing || n < 2 ||
        !plan_resident_eligible(p))
        return false;
    plan_upload_slots(p);
    plan_gn_step(p, n);
    if (p->cost_wanted) plan_cost(p, p->sp.nIterations);
    p->sp.nIter = p->sp.nIterations;
    return true;
}
