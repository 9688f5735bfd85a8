// host_lm.h -- host loop of the "LMGPU" solver kind (device side: arap_lm.h).
#pragma once

// ---------------------------------------------------------------------------------------------
// "LMGPU": host loop of the Levenberg-Marquardt branch (solverGPUGaussNewton.t:1016-1177 with UsesLambda).
// Like the reference it is host driven: Q is read back after every PCG iteration for the zeta test (:1093-1102)
// and the costs after every step (:1119-1157); no graph, one frame (Opt_* plans only).
// ---------------------------------------------------------------------------------------------
static void plan_lm_alloc(Opt_Plan* p)
{
    if (p->lm_block) return;
    const size_t N = (size_t)p->N;
    p->lm_block = device_block(p->st, true, [&](Carver& part) {
        for (float2** f : {&p->pd.bO, &p->pd.CtCO, &p->pd.SSqO, &p->pd.AdO, &p->prevO}) part(*f, N * sizeof(float2));
        for (float** f : {&p->pd.bA, &p->pd.CtCA, &p->pd.SSqA, &p->pd.AdA, &p->prevA}) part(*f, N * sizeof(float));
    });
}

static double plan_read_shards(Opt_Plan* p, const double* dev)
{
    double sh[NSHARD];
    HC(hipMemcpyAsync(sh, dev, sizeof(sh), hipMemcpyDeviceToHost, p->st->stream));
    HC(hipStreamSynchronize(p->st->stream));
    double t = 0.0;
    for (int i = 0; i < NSHARD; ++i) t += sh[i];
    return t;
}

static void plan_init_lm(Opt_Plan* p)
{
    HC(hipSetDevice(p->st->device));
    plan_lm_alloc(p);
    p->sp.nIter = 0;
    p->pd.lm = 1;
    plan_reserve(p, p->sp.lIterations, 2);
    if (p->sp.lIterations + 2 > p->lm_lcap || !p->pd.lmred) {
        HC(hipStreamSynchronize(p->st->stream));
        if (p->pd.lmred) HC(hipFree(p->pd.lmred));
        p->lm_lcap = p->sp.lIterations + 2;
        HC(hipMalloc(&p->pd.lmred, (size_t)p->lm_lcap * NSHARD * sizeof(double)));
    }
    plan_upload_slots(p);
    p->lm_radius = p->sp.trust_region_radius;                 // init copies the solver parameters (:996-1001)
    p->lm_decrease = p->sp.radius_decrease_factor;
    p->lm_done = false;
    p->lm_last_pcg = 0;
    p->lm_last_outcome = -1;
    HC(hipMemsetAsync(p->pd.costred, 0, (size_t)p->pd.ncost * NSHARD * sizeof(double), p->st->stream));
    hipLaunchKernelGGL(k_cost, p->grid(), p->blk(), 0, p->st->stream, p->pd, 0);
    p->lm_prev_cost = plan_read_cost(p, 0, 0);
}

static int plan_step_lm(Opt_Plan* p)
{
    Opt_State* st = p->st;
    hipStream_t s = st->stream;
    const SolverParameters& sp = p->sp;
    if (p->lm_done || sp.nIter >= sp.nIterations) return 0;
    plan_upload_slots(p);
    const dim3 g = p->grid(), b = p->blk();
    const int L = sp.lIterations;
    const size_t N = (size_t)p->N;
    HC(hipMemsetAsync(p->pd.red, 0, (size_t)p->pd.nslots * NSHARD * sizeof(double), s));
    HC(hipMemsetAsync(p->pd.lmred, 0, (size_t)p->lm_lcap * NSHARD * sizeof(double), s));
    hipLaunchKernelGGL(k_gn_prep, g, b, 0, s, p->pd);
    hipLaunchKernelGGL(k_gn_init, g, b, 0, s, p->pd);
    HC(hipMemsetAsync(p->pd.red, 0, NSHARD * sizeof(double), s));            // scanAlphaNumerator again (:1041)
    hipLaunchKernelGGL(k_lm_prepare, g, b, 0, s, p->pd, p->lm_radius, sp.min_lm_diagonal, sp.max_lm_diagonal,
                       sp.nIter == 0 ? 1 : 0);
    float Q0 = (float)plan_read_shards(p, p->pd.lmred);
    p->lm_last_pcg = 0;
    for (int l = 0; l < L; ++l) {
        hipLaunchKernelGGL(k_pcg_a, g, b, 0, s, p->pd, l);
        if (((l + 1) % sp.residual_reset_period) == 0) {
            hipLaunchKernelGGL(k_lm_step2a, g, b, 0, s, p->pd, l);
            hipLaunchKernelGGL(k_lm_apply, g, b, 0, s, p->pd, (const float2*)p->pd.deltaO, (const float*)p->pd.deltaA,
                               p->pd.AdO, p->pd.AdA);
            hipLaunchKernelGGL(k_lm_step2b, g, b, 0, s, p->pd, l);
        } else {
            hipLaunchKernelGGL(k_pcg_b, g, b, 0, s, p->pd, l);
        }
        const float Q1 = (float)plan_read_shards(p, p->pd.lmred + (size_t)(l + 1) * NSHARD);
        const float zeta = (float)(l + 1) * (Q1 - Q0) / Q1;
        p->lm_last_pcg = l + 1;
        if (zeta < sp.q_tolerance) break;
        Q0 = Q1;
    }
    hipLaunchKernelGGL(k_lm_model_cost, g, b, 0, s, p->pd, p->lm_lcap - 1);
    const float model_cost = (float)plan_read_shards(p, p->pd.lmred + (size_t)(p->lm_lcap - 1) * NSHARD);
    const float model_cost_change = (float)p->lm_prev_cost - model_cost;
    const Slot& sl = p->hslots[0];
    HC(hipMemcpyAsync(p->prevO, sl.O, N * sizeof(float2), hipMemcpyDeviceToDevice, s));   // savePreviousUnknowns
    HC(hipMemcpyAsync(p->prevA, sl.A, N * sizeof(float), hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(k_gn_update, g, b, 0, s, p->pd, -1);
    HC(hipMemsetAsync(p->pd.costred + NSHARD, 0, NSHARD * sizeof(double), s));
    hipLaunchKernelGGL(k_cost, g, b, 0, s, p->pd, 1);
    const double newCost = plan_read_cost(p, 0, 1);
    const float cost_change = (float)p->lm_prev_cost - (float)newCost;
    const float relative_decrease = cost_change / model_cost_change;
    if (cost_change >= 0 && relative_decrease > sp.min_relative_decrease) {
        if (cost_change <= (float)p->lm_prev_cost * sp.function_tolerance) {
            if (st->verbosity > 0) printf("\nFunction tolerance reached, exiting\n");
            p->lm_done = true;
            p->lm_last_outcome = ARAPFLOW_LM_FUNCTION_TOLERANCE;
            return 0;
        }
        const double step_quality = relative_decrease;
        const double tmp_factor = 1.0 - pow(2.0 * step_quality - 1.0, 3.0);
        p->lm_radius = (float)((double)p->lm_radius / fmax(1.0 / 3.0, tmp_factor));
        p->lm_radius = (float)fmin((double)p->lm_radius, (double)sp.max_trust_region_radius);
        p->lm_decrease = 2.0f;
        p->lm_prev_cost = newCost;
        p->lm_last_outcome = ARAPFLOW_LM_ACCEPTED;
    } else {
        HC(hipMemcpyAsync(sl.O, p->prevO, N * sizeof(float2), hipMemcpyDeviceToDevice, s));   // revertUpdate
        HC(hipMemcpyAsync(sl.A, p->prevA, N * sizeof(float), hipMemcpyDeviceToDevice, s));
        p->lm_radius = p->lm_radius / p->lm_decrease;
        p->lm_decrease = 2.0f * p->lm_decrease;
        if (p->lm_radius <= sp.min_trust_region_radius) {
            if (st->verbosity > 0) printf("\nTrust_region_radius is less than the min, exiting\n");
            p->lm_done = true;
            p->lm_last_outcome = ARAPFLOW_LM_MIN_RADIUS;
            return 0;
        }
        p->lm_last_outcome = ARAPFLOW_LM_REJECTED;
    }
    if (st->verbosity > 0) printf("cost: %f (trust_region_radius %g)\n", p->lm_prev_cost, p->lm_radius);
    p->sp.nIter += 1;
    return 1;
}
