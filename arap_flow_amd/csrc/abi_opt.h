// abi_opt.h -- the Opt_* drop-in ABI of include/arap_opt.h (problem specification check, state / problem / plan
// lifecycle, Init / Step / Solve) and the small ArapFlow_* entry points on a state: setters, timers, and the one-shot
// EvalJTF / ApplyJTJ / Cost used by the parity tests.
#pragma once

// ---------------------------------------------------------------------------------------------
// Problem specification check.  The library hard-codes the energy of arap_plan.t:1-23; the file
// named in Opt_ProblemDefine is checked declaration by declaration against it.
// ---------------------------------------------------------------------------------------------
static std::string strip_spec(const std::string& src)
{
    std::string out;
    size_t i = 0;
    while (i < src.size()) {
        if (src[i] == '-' && i + 1 < src.size() && src[i + 1] == '-') {   // Lua comment
            while (i < src.size() && src[i] != '\n') ++i;
            continue;
        }
        if (!isspace((unsigned char)src[i])) out.push_back(src[i]);
        ++i;
    }
    return out;
}

static bool spec_is_arap(const std::string& stripped, std::string& why)
{
    // every structural element of the energy must be present, in this order of appearance
    static const char* need[] = {
        "Dim(\"W\",0)", "Dim(\"H\",1)",
        "Unknown(\"Offset\",opt_float2,{W,H},0)",
        "Unknown(\"Angle\",opt_float,{W,H},1)",
        "Array(\"UrShape\",opt_float2,{W,H},2)",
        "Array(\"Constraints\",opt_float2,{W,H},3)",
        "Array(\"Mask\",opt_float,{W,H},4)",
        "Param(\"w_fitSqrt\",float,5)",
        "Param(\"w_regSqrt\",float,6)",
        "UsePreconditioner(true)",
        "Exclude(Not(eq(Mask(0,0),0)))",
        "Stencil{{1,0},{-1,0},{0,1},{0,-1}}",
        "w_regSqrt*((Offset(0,0)-Offset(x,y))-Rotate2D(Angle(0,0),(UrShape(0,0)-UrShape(x,y))))",
        "InBounds(x,y)*eq(Mask(x,y),0)*eq(Mask(0,0),0)",
        "Energy(Select(valid,e_reg,0))",
        "(Offset(0,0)-Constraints(0,0))",
        "All(greatereq(Constraints(0,0),0))",
        "Energy(w_fitSqrt*Select(valid,e_fit,0.0))",
    };
    size_t pos = 0;
    for (const char* n : need) {
        size_t f = stripped.find(n, pos);
        if (f == std::string::npos) { why = std::string("missing or out of order: ") + n; return false; }
        pos = f + strlen(n);
    }
    // and nothing else that adds energy terms or unknowns
    size_t cnt = 0, at = 0;
    while ((at = stripped.find("Energy(", at)) != std::string::npos) { ++cnt; at += 7; }
    if (cnt != 2) { why = "expected exactly two Energy() terms"; return false; }
    cnt = 0; at = 0;
    while ((at = stripped.find("Unknown(", at)) != std::string::npos) { ++cnt; at += 8; }
    if (cnt != 2) { why = "expected exactly two Unknown() declarations"; return false; }
    return true;
}

static void slot_from_params(Slot& s, void** pp)
{
    // plan-declared indices: arap_plan.t:2-8 ; scalars are HOST pointers (util.t:664-692)
    s.O = (float2*)pp[0];
    s.A = (float*)pp[1];
    s.U = (const float2*)pp[2];
    s.C = (const float2*)pp[3];
    s.M = (const float*)pp[4];
    s.wf = *(const float*)pp[5];
    s.wr = *(const float*)pp[6];
}

// ---------------------------------------------------------------------------------------------
// C ABI, part 1
// ---------------------------------------------------------------------------------------------
extern "C" {

Opt_State* Opt_NewState(Opt_InitializationParameters params)
{
    if (params.doublePrecision) {
        fprintf(stderr, "arapopt: doublePrecision is not supported (float32 only, as the application uses)\n");
        return nullptr;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        fprintf(stderr, "arapopt: no HIP device available; this library has no CPU fallback\n");
        return nullptr;
    }
    Opt_State* st = new Opt_State();
    st->verbosity = params.verbosityLevel;
    st->timing = params.collectPerKernelTimingInfo;
    HC(hipGetDevice(&st->device));
    HC(hipStreamCreateWithFlags(&st->cap, hipStreamNonBlocking));
    HC(hipEventCreate(&st->t0));
    HC(hipEventCreate(&st->t1));
    const Knobs knobs = read_knobs();
    st->use_graph = !knobs.no_graph;
    st->tile = knobs.tile;                 // experiments: phase-A variant
    st->force_b8 = knobs.b8;               // experiments: 8-byte form of phase B
    st->stream_a = knobs.stream_a;
    st->mscore_plain = knobs.mscore_plain;
    st->aug_bytes = knobs.aug_bytes;
    return st;
}

void ArapFlow_FreeState(Opt_State* st)
{
    if (!st) return;
    (void)hipStreamDestroy(st->cap);
    if (st->own_stream) (void)hipStreamDestroy(st->own_stream);
    (void)hipEventDestroy(st->t0);
    (void)hipEventDestroy(st->t1);
    st->ktimer.clear();
    if (st->diag) (void)hipFree(st->diag);
    if (st->tex) (void)hipFree(st->tex);
    if (st->light) (void)hipFree(st->light);
    if (st->aug) (void)hipFree(st->aug);
    if (st->clip) (void)hipFree(st->clip);
    delete st;
}

Opt_Problem* Opt_ProblemDefine(Opt_State* state, const char* filename, const char* solverkind)
{
    if (!state || !filename || !solverkind) return nullptr;
    const int kind = strcmp(solverkind, "gaussNewtonGPU") == 0 ? 0 : (strcmp(solverkind, "LMGPU") == 0 ? 1 : -1);
    if (kind < 0) {                                                       // asserted at o.t:122
        fprintf(stderr, "arapopt: unknown solver kind '%s' (expected gaussNewtonGPU or LMGPU)\n", solverkind);
        return nullptr;
    }
    if (strcmp(filename, "builtin:arap") != 0) {
        FILE* f = fopen(filename, "rb");
        if (!f) {
            fprintf(stderr, "arapopt: cannot open problem specification '%s'\n", filename);
            return nullptr;
        }
        std::string src;
        char buf[4096];
        size_t n;
        while ((n = fread(buf, 1, sizeof(buf), f)) > 0) src.append(buf, n);
        fclose(f);
        std::string why;
        if (!spec_is_arap(strip_spec(src), why)) {
            fprintf(stderr,
                    "arapopt: '%s' is not the ARAP image-warping energy this library implements (%s)\n",
                    filename, why.c_str());
            return nullptr;
        }
    }
    Opt_Problem* pr = new Opt_Problem();
    pr->kind = kind;
    if (state->verbosity > 1) printf("arapopt: problem '%s' (%s) accepted\n", filename, solverkind);
    return pr;
}

void Opt_ProblemDelete(Opt_State*, Opt_Problem* problem) { delete problem; }

Opt_Plan* Opt_ProblemPlan(Opt_State* state, Opt_Problem* problem, unsigned int* dimensions)
{
    if (!state || !problem || !dimensions) return nullptr;
    const unsigned W = dimensions[0], H = dimensions[1];
    if (W == 0 || H == 0 || (uint64_t)W * H > (1ull << 30)) {
        fprintf(stderr, "arapopt: bad dimensions %u x %u\n", W, H);
        return nullptr;
    }
    Opt_Plan* p = plan_create(state, (int)W, (int)H, 1);
    p->kind = problem->kind;
    if (p->kind == 0) plan_enable_resident(p);
    return p;
}

void Opt_PlanFree(Opt_State*, Opt_Plan* plan) { plan_free(plan); }

void Opt_SetSolverParameter(Opt_State*, Opt_Plan* plan, const char* name, void* value)
{
    if (!plan || !name || !value) return;
    SolverParameters& sp = plan->sp;
#define SETI(f) if (strcmp(name, #f) == 0) { sp.f = *(int*)value; return; }
#define SETF(f) if (strcmp(name, #f) == 0) { sp.f = *(float*)value; return; }
    if (strcmp(name, "residual_reset_period") == 0 && *(int*)value < 1) {    // the host loop takes (l + 1) modulo it
        if (plan->st->verbosity > 0)
            printf("Warning: residual_reset_period %d is below 1, keeping %d\n", *(int*)value, sp.residual_reset_period);
        return;
    }
    SETI(nIterations) SETI(lIterations) SETI(residual_reset_period)
    SETF(min_relative_decrease) SETF(min_trust_region_radius) SETF(max_trust_region_radius)
    SETF(q_tolerance) SETF(function_tolerance) SETF(trust_region_radius) SETF(radius_decrease_factor)
    SETF(min_lm_diagonal) SETF(max_lm_diagonal)
#undef SETI
#undef SETF
    if (plan->st->verbosity > 0) printf("Warning: tried to set nonexistent solver parameter %s\n", name);
}

void Opt_ProblemInit(Opt_State* state, Opt_Plan* plan, void** problemparams)
{
    if (state && state->res_cooldown > 0) --state->res_cooldown;
    plan->nb = 1;
    slot_from_params(plan->hslots[0], problemparams);
    if (plan->kind == 1) plan_init_lm(plan); else plan_init(plan);
}

int Opt_ProblemStep(Opt_State*, Opt_Plan* plan, void** problemparams)
{
    slot_from_params(plan->hslots[0], problemparams);
    return plan->kind == 1 ? plan_step_lm(plan) : plan_step(plan);
}

void Opt_ProblemSolve(Opt_State* state, Opt_Plan* plan, void** problemparams)
{
    Opt_ProblemInit(state, plan, problemparams);
    while (Opt_ProblemStep(state, plan, problemparams) != 0) {}
}

double Opt_ProblemCurrentCost(Opt_State*, Opt_Plan* plan)
{
    if (plan->kind == 1) return (double)(float)plan->lm_prev_cost;
    return plan_read_cost(plan, 0, plan->sp.nIter);
}

// ---------------------------------------------------------------------------------------------
// C ABI, part 2
// ---------------------------------------------------------------------------------------------
const char* ArapFlow_Version(void) { return ARAPOPT_VERSION; }

int ArapFlow_LMState(Opt_Plan* plan, float* radius, float* decrease, int* pcg_iterations_last_step, int* outcome_last_step)
{
    if (!plan || plan->kind != 1) return -1;
    if (radius) *radius = plan->lm_radius;
    if (decrease) *decrease = plan->lm_decrease;
    if (pcg_iterations_last_step) *pcg_iterations_last_step = plan->lm_last_pcg;
    if (outcome_last_step) *outcome_last_step = plan->lm_last_outcome;
    return 0;
}

void ArapFlow_SetResident(Opt_State* state, int on)
{
    state->use_resident = on != 0;
    if (on) { state->res_cooldown = 0; state->res_backoff = 8; }     // an explicit "on" also ends a pause after a timeout
}

int ArapFlow_SetTile(Opt_State* state, int tile_x, int tile_y)
{
    if (tile_x < 0 && tile_y < 0) { state->tile = -1; return 0; }         // automatic (default)
    const int v = tile_shape_index(tile_x, tile_y);
    if (v >= 0) state->tile = v;
    return v >= 0 ? 0 : -1;
}

void ArapFlow_SetKernelTiming(Opt_State* state, int on)
{
    HC(hipStreamSynchronize(state->stream));
    state->ktimer.clear();
    state->timing = on ? 1 : 0;
}

int ArapFlow_KernelTime(Opt_State* state, const char* kernel_name, double* total_ms, uint64_t* launches)
{
    double tot = 0.0;
    uint64_t n = 0;
    for (auto& r : state->ktimer.recs) {
        if (r.name != kernel_name) continue;
        float ms = 0.f;
        HC(hipEventSynchronize(r.b));
        HC(hipEventElapsedTime(&ms, r.a, r.b));
        tot += ms;
        ++n;
    }
    if (total_ms) *total_ms = tot;
    if (launches) *launches = n;
    return n ? 0 : -1;
}

void ArapFlow_SetStream(Opt_State* state, void* hip_stream) { state->stream = (hipStream_t)hip_stream; }

int ArapFlow_UseOwnStream(Opt_State* state)
{
    if (!state) return -1;
    if (!state->own_stream) HC(hipStreamCreateWithFlags(&state->own_stream, hipStreamNonBlocking));
    state->stream = state->own_stream;
    return 0;
}

void ArapFlow_TimerBegin(Opt_State* state) { HC(hipEventRecord(state->t0, state->stream)); }

float ArapFlow_TimerEnd(Opt_State* state)
{
    float ms = 0.f;
    HC(hipEventRecord(state->t1, state->stream));
    HC(hipEventSynchronize(state->t1));
    HC(hipEventElapsedTime(&ms, state->t0, state->t1));
    return ms;
}

static Opt_Plan* temp_plan(Opt_State* st, unsigned W, unsigned H, const void* O, const void* A, const void* U,
                           const void* C, const void* M, float wf, float wr)
{
    Opt_Plan* p = plan_create(st, (int)W, (int)H, 1);
    Slot& s = p->hslots[0];
    s.O = (float2*)O; s.A = (float*)A; s.U = (const float2*)U; s.C = (const float2*)C; s.M = (const float*)M;
    s.wf = wf; s.wr = wr;
    p->nb = 1;
    plan_reserve(p, 1, 1);
    plan_upload_slots(p);
    HC(hipMemsetAsync(p->pd.red, 0, (size_t)p->pd.nslots * NSHARD * sizeof(double), st->stream));
    HC(hipMemsetAsync(p->pd.costred, 0, (size_t)p->pd.ncost * NSHARD * sizeof(double), st->stream));
    return p;
}

int ArapFlow_EvalJTF(Opt_State* st, unsigned W, unsigned H, const void* O, const void* A, const void* U,
                     const void* C, const void* M, float wf, float wr, void* gO, void* gA, void* dO, void* dA)
{
    Opt_Plan* p = temp_plan(st, W, H, O, A, U, C, M, wf, wr);
    hipLaunchKernelGGL(k_gn_prep, p->grid(), p->blk(), 0, st->stream, p->pd);
    hipLaunchKernelGGL(k_gn_init, p->grid(), p->blk(), 0, st->stream, p->pd);
    hipLaunchKernelGGL(k_export_jtf, p->grid(), p->blk(), 0, st->stream, p->pd, (float2*)gO, (float*)gA,
                       (float2*)dO, (float*)dA);
    hipError_t e = hipStreamSynchronize(st->stream);
    if (e == hipSuccess) e = hipGetLastError();
    plan_free(p);
    return (int)e;
}

int ArapFlow_ApplyJTJ(Opt_State* st, unsigned W, unsigned H, const void* A, const void* U, const void* C,
                      const void* M, float wf, float wr, const void* pO, const void* pA, void* outO, void* outA)
{
    Opt_Plan* p = temp_plan(st, W, H, nullptr, A, U, C, M, wf, wr);
    const size_t N = (size_t)W * H;
    hipLaunchKernelGGL(k_gn_prep, p->grid(), p->blk(), 0, st->stream, p->pd);
    HC(hipMemcpyAsync(p->pd.pO0, pO, N * sizeof(float2), hipMemcpyDeviceToDevice, st->stream));
    HC(hipMemcpyAsync(p->pd.pA0, pA, N * sizeof(float), hipMemcpyDeviceToDevice, st->stream));
    hipLaunchKernelGGL(k_pcg_a, p->grid(), p->blk(), 0, st->stream, p->pd, 0);
    HC(hipMemcpyAsync(outO, p->pd.ApO, N * sizeof(float2), hipMemcpyDeviceToDevice, st->stream));
    HC(hipMemcpyAsync(outA, p->pd.ApA, N * sizeof(float), hipMemcpyDeviceToDevice, st->stream));
    hipError_t e = hipStreamSynchronize(st->stream);
    if (e == hipSuccess) e = hipGetLastError();
    plan_free(p);
    return (int)e;
}

int ArapFlow_Cost(Opt_State* st, unsigned W, unsigned H, const void* O, const void* A, const void* U,
                  const void* C, const void* M, float wf, float wr, double* cost_host)
{
    Opt_Plan* p = temp_plan(st, W, H, O, A, U, C, M, wf, wr);
    hipLaunchKernelGGL(k_cost, p->grid(), p->blk(), 0, st->stream, p->pd, 0);
    *cost_host = plan_read_cost(p, 0, 0);
    hipError_t e = hipGetLastError();
    plan_free(p);
    return (int)e;
}

}  // extern "C"
