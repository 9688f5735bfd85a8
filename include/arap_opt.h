/*
 * arap_opt.h -- C ABI of libarapopt.so, the MI355X-native (HIP, gfx950) replacement for the ARAP
 * hot path of lhoangan/arap_flow.
 *
 * Part 1 re-declares, with identical names, argument order and meaning, the ten entry points of the
 * reference's Opt C API (reference: ARAP/API/release/include/Opt.h:35-71, implemented by the
 * thunks of ARAP/API/src/createwrapper.t:124-220 around ARAP/API/src/o.t:2521-2558).  A program
 * written against the reference's Opt.h (ARAP/shared/OptSolver.h:43-91) links against this library
 * unchanged -- see INTEGRATION.md.
 *
 * Part 2 (ArapFlow_*) are additions that have no counterpart symbol in the reference: they move the
 * work the reference does on the host around each Opt_ProblemSolve (constraint ramp, reset, flow
 * extraction, triangle rasteriser: ARAP/deformation/src/CombinedSolver.h:199-366,
 * ARAP/warping/src/main.cpp:110-225) onto the GPU and batch independent frames.
 *
 * Plain C: pointers and sizes only.  Device pointers are HIP device pointers.
 */
#ifndef ARAP_OPT_H
#define ARAP_OPT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * Part 1: the reference's Opt API
 * ---------------------------------------------------------------------------------------------- */

typedef struct Opt_State Opt_State;     /* Opt.h:3 */
typedef struct Opt_Plan Opt_Plan;       /* Opt.h:4 */
typedef struct Opt_Problem Opt_Problem; /* Opt.h:5 */

/* Opt.h:10-30.  Passed BY VALUE to Opt_NewState.
 *   doublePrecision            must be 0 (the application never sets it: OptSolver.h:49); a non-zero
 *                              value makes Opt_NewState print an error and return NULL.
 *   verbosityLevel             0 silent, >=1 per-GN-step cost lines ("cost: a -> b",
 *                              solverGPUGaussNewton.t:1160).
 *   collectPerKernelTimingInfo non-zero: hipEvent brackets around every launch, table printed when
 *                              the solve ends (util.t:451-511).
 *   threadsPerBlock            ignored (the tile shape is fixed by the kernels). */
struct Opt_InitializationParameters {
    int doublePrecision;
    int verbosityLevel;
    int collectPerKernelTimingInfo;
    int threadsPerBlock;
};
typedef struct Opt_InitializationParameters Opt_InitializationParameters;

/* Opt.h:35.  New independent context on the current HIP device.  Never freed by the reference;
 * ArapFlow_FreeState below is the addition that frees it. */
Opt_State* Opt_NewState(Opt_InitializationParameters params);

/* Opt.h:40-41.  `filename` is the problem specification.  This library implements exactly one
 * energy, the one of the reference's arap_plan.t:1-23; the file is read, stripped of comments and
 * white space, and its declarations are checked against that energy.  Anything else prints a
 * diagnostic and returns NULL (the reference returns NULL from Opt_ProblemPlan when compilation
 * fails, o.t:861-881).  The literal name "builtin:arap" selects the energy without a file.
 * `solverkind`: "gaussNewtonGPU" (what the application uses, CombinedSolverBase.h:75-77) or "LMGPU" (the
 * Levenberg-Marquardt branch of the same solver, solverGPUGaussNewton.t:615-680,1038-1157: trust region, CtC,
 * model cost, revert); anything else: diagnostic + NULL (asserted at o.t:122). */
Opt_Problem* Opt_ProblemDefine(Opt_State* state, const char* filename, const char* solverkind);
void Opt_ProblemDelete(Opt_State* state, Opt_Problem* problem);

/* Opt.h:46-47.  dimensions[0] = W, dimensions[1] = H (Dim("W",0), Dim("H",1), arap_plan.t:1).
 * Allocates the solver state (solverGPUGaussNewton.t:1254-1284). */
Opt_Plan* Opt_ProblemPlan(Opt_State* state, Opt_Problem* problem, unsigned int* dimensions);
void Opt_PlanFree(Opt_State* state, Opt_Plan* plan);

/* Opt.h:51.  `value` points to an int for "nIterations", "lIterations", "residual_reset_period"
 * and to a float for the nine LM parameters (solverGPUGaussNewton.t:148-163), which only "LMGPU" plans read.
 * Unknown names print a warning (:1220).  A "residual_reset_period" below 1 is not stored (the step takes the PCG
 * iteration number modulo it): the plan keeps its previous value, with a warning when verbose. */
void Opt_SetSolverParameter(Opt_State* state, Opt_Plan* plan, const char* name, void* value);

/* Opt.h:56-66.  problemparams is indexed by the plan's declared indices (arap_plan.t:2-8,
 * unpacked as in util.t:664-692):
 *   [0] float2* device  Offset      in/out   [1] float*  device  Angle  in/out
 *   [2] float2* device  UrShape     in       [3] float2* device  Constraints in
 *   [4] float*  device  Mask        in       [5] float*  HOST    w_fitSqrt
 *   [6] float*  HOST    w_regSqrt
 * Images are W*H, row major, x fastest, no padding (o.t:376-387).  The array is re-read on every
 * Init and every Step (solverGPUGaussNewton.t:960,1026).
 * Opt_ProblemSolve = Init, then Step until it returns 0 (o.t:2548-2551).
 * Opt_ProblemStep: one Gauss-Newton iteration = PCGInit1, lIterations PCG iterations, update,
 * cost (:1016-1177); returns 0 once nIterations steps have been taken. */
void Opt_ProblemSolve(Opt_State* state, Opt_Plan* plan, void** problemparams);
void Opt_ProblemInit(Opt_State* state, Opt_Plan* plan, void** problemparams);
int Opt_ProblemStep(Opt_State* state, Opt_Plan* plan, void** problemparams);

/* Opt.h:71.  Cost after the last completed Init/Step, float upconverted to double
 * (solverGPUGaussNewton.t:1179-1182).  Synchronises the plan's stream. */
double Opt_ProblemCurrentCost(Opt_State* state, Opt_Plan* plan);

/* ------------------------------------------------------------------------------------------------
 * Part 2: additions (no reference symbol)
 * ---------------------------------------------------------------------------------------------- */

/* Library identification: "arapopt <version> gfx950". */
const char* ArapFlow_Version(void);

void ArapFlow_FreeState(Opt_State* state);

/* All work of `state` is enqueued on this HIP stream (hipStream_t as void*; NULL = the null
 * stream, which is what the reference uses: util.t:828). */
void ArapFlow_SetStream(Opt_State* state, void* hip_stream);
/* The same with a non-blocking stream the library creates and owns: what a host program that overlaps uploads and
 * downloads with solves wants (the null stream synchronises with every blocking stream of the process). */
int ArapFlow_UseOwnStream(Opt_State* state);

/* hipEvent stopwatch on the state's stream, for callers that have no HIP binding of their own
 * (bench.py).  Begin records an event; End records a second one, synchronises on it and returns
 * the elapsed milliseconds. */
void ArapFlow_TimerBegin(Opt_State* state);
float ArapFlow_TimerEnd(Opt_State* state);

/* Per-kernel hipEvent timing (the reference's collectPerKernelTimingInfo, Opt.h:23-25, util.t:414-511)
 * switched at run time.  While on, every kernel launch is bracketed by two events on the stream and
 * hipGraph replay is disabled.  ArapFlow_KernelTime sums the records of the kernel named
 * `kernel_name` ("GNPrep", "PCGInit1", "PCGStepA", "PCGStepB", "PCGLinearUpdate", "computeCost")
 * since timing was switched on; returns -1 if there is none. */
void ArapFlow_SetKernelTiming(Opt_State* state, int on);
int ArapFlow_KernelTime(Opt_State* state, const char* kernel_name, double* total_ms, uint64_t* launches);

/* Kernel-level entry points on raw device images, used by the parity tests (tier T1).  All pointers
 * are device pointers; vectors are split like the unknowns: an Offset-shaped float2 image and an
 * Angle-shaped float image.  wf/wr = w_fitSqrt/w_regSqrt.  Synchronous.
 *   ArapFlow_EvalJTF : gradient J^T F and diag(J^T J) of o.t:2129-2172
 *   ArapFlow_ApplyJTJ: (J^T J P) of o.t:2029-2089
 *   ArapFlow_Cost    : o.t:2375-2385
 * Return 0 on success, a HIP error code otherwise. */
int ArapFlow_EvalJTF(Opt_State* state, unsigned W, unsigned H, const void* Offset, const void* Angle,
                     const void* UrShape, const void* Constraints, const void* Mask, float wf, float wr,
                     void* gO, void* gA, void* dO, void* dA);
int ArapFlow_ApplyJTJ(Opt_State* state, unsigned W, unsigned H, const void* Angle, const void* UrShape,
                      const void* Constraints, const void* Mask, float wf, float wr, const void* pO,
                      const void* pA, void* outO, void* outA);
int ArapFlow_Cost(Opt_State* state, unsigned W, unsigned H, const void* Offset, const void* Angle,
                  const void* UrShape, const void* Constraints, const void* Mask, float wf, float wr,
                  double* cost_host);

/* Batched frame solver: the device-resident counterpart of the reference's CombinedSolver
 * (ARAP/deformation/src/CombinedSolver.h:99-390) driven as in ARAP/deformation/src/main.cpp:140-160.
 * One object serves frames of one size; `batch` frames are solved concurrently, one set of PCG
 * scalars per frame.  Frames are independent: no exchange between slots. */
typedef struct ArapFlow_Solver ArapFlow_Solver;

ArapFlow_Solver* ArapFlow_SolverCreate(Opt_State* state, unsigned W, unsigned H, unsigned batch);
void ArapFlow_SolverFree(ArapFlow_Solver* s);

/* addImage (CombinedSolver.h:139-170) for slot `slot`.  HOST pointers:
 *   rgb       uint8[H][W][3] or NULL (no warp wanted)
 *   mask_red  uint8[H][W]    red channel of the mask PNG: 0 = deformable object (CombinedSolver.h:213)
 *   cons      int32[ncons][4] = x1 y1 x2 y2 rows of the constraint file (main.cpp:26-50), file order
 *   add_border_pins  non-zero: append (x,y,x,y) for every border pixel (main.cpp:130-136)
 * The host buffers are staged into pinned memory before the call returns (they may be reused at once); the copies
 * to the device run on the solver's own copy stream and the next solve waits for them.  If a solve of this solver is
 * still in flight the call waits for it first.  Returns 0, or -1 on bad arguments. */
int ArapFlow_SolverSetFrame(ArapFlow_Solver* s, unsigned slot, const uint8_t* rgb, const uint8_t* mask_red,
                            const int32_t* cons, unsigned ncons, int add_border_pins);

/* solveAll (CombinedSolverBase.h:23-31,99-120) for slots [0, nframes): reset (CombinedSolver.h:207-221),
 * then for i < numIter: constraints ramped to alpha = (i+1)/numIter (:199-201,223-242) and one
 * Opt_ProblemSolve with nIterations/lIterations, unknowns carried over.  The application's values
 * are 19, 8, 400 (main.cpp:215-221).  Returns when the solve has finished. */
int ArapFlow_SolverSolve(ArapFlow_Solver* s, unsigned nframes, unsigned numIter, unsigned nIterations,
                         unsigned lIterations);

/* Pipelined form of the three calls around a solve, for hosts that keep the GPU busy (arap_deform --serve): enqueue
 * the whole schedule of slots [0, nframes) on the state's stream -- behind this solver's pending SetFrame uploads,
 * which travel on the solver's own copy stream from pinned staging -- then, if `warp`, the flow emission + rasteriser,
 * then, if `download`, the copy of every slot's flow / warped RGB / warped mask into pinned host buffers owned by the
 * solver (again on the copy stream), and return WITHOUT waiting.  With two solver objects a host uploads batch k+1
 * and reads back batch k-1 while batch k is being solved.  ArapFlow_SolverWait blocks until everything enqueued for
 * this solver is done (and, if a resident launch gave up, redoes the schedule on the two-kernel path first); every
 * other call on a solver with work in flight waits by itself.  ArapFlow_SolverSolve = SolveAsync(.., 0, 0) + Wait.
 * ArapFlow_SolverHostResults returns pointers into the pinned buffers of a `download` solve (valid until the next
 * solve of this solver; warped_rgb NULL if the slot has no RGB).  Return 0, -1 on bad arguments. */
int ArapFlow_SolverSolveAsync(ArapFlow_Solver* s, unsigned nframes, unsigned numIter, unsigned nIterations,
                              unsigned lIterations, int warp, int download);
int ArapFlow_SolverWait(ArapFlow_Solver* s);
int ArapFlow_SolverHostResults(ArapFlow_Solver* s, unsigned slot, const float** flow, const uint8_t** warped_rgb,
                               const uint8_t** warped_mask);

/* Optional outputs of the warp (DESIGN.md "Backward flow and occlusion"; all off by default, and then no extra kernel
 * runs).  ArapFlow_SolverSetOutputs(s, which) selects them, with `which` an OR of
 *   ARAPFLOW_OUT_BACKWARD   backward flow float[H][W][2] (frame 2 -> frame 1; 0 where nothing is drawn) and the
 *                           backward occlusion uint8[H][W] (255 = frame-2 object pixel left uncovered: revealed)
 *   ARAPFLOW_OUT_OCCLUSION  forward occlusion uint8[H][W] (255 = frame-1 pixel not visible in frame 2)
 * for every later ArapFlow_SolverWarp and SolveAsync(.., warp = 1, ..).  The device buffers (about 34 bytes per pixel
 * and slot, output and scratch) are allocated at the first call that turns an output on.  Returns 0, -1 on bad
 * arguments.
 * ArapFlow_SolverGetExtraResults: synchronise and copy one slot's outputs of the last warp to HOST buffers (any may be
 * NULL); -1 if a requested output was off at that warp.
 * ArapFlow_SolverHostExtraResults: pointers into the solver's pinned buffers filled by a `download` solve (valid until
 * the next solve of this solver; NULL for an output that was off); -1 if that solve downloaded none. */
#define ARAPFLOW_OUT_BACKWARD 1
#define ARAPFLOW_OUT_OCCLUSION 2
int ArapFlow_SolverSetOutputs(ArapFlow_Solver* s, int which);
int ArapFlow_SolverGetExtraResults(ArapFlow_Solver* s, unsigned slot, float* bwd, uint8_t* occ_bwd, uint8_t* occ);
int ArapFlow_SolverHostExtraResults(ArapFlow_Solver* s, unsigned slot, const float** bwd, const uint8_t** occ_bwd,
                                    const uint8_t** occ);

/* In-between frames from the constraint ramp (DESIGN.md "In-between frames"; off by default, and then nothing is
 * allocated, copied or launched).  After ramp step i (1 <= i <= numIter) the slot's Offset is the state S_i: a converged
 * deformation towards the fraction i / numIter of every handle's displacement; S_numIter is the final result.
 * ArapFlow_SolverSetSnapshots(s, steps, n) selects n <= ARAPFLOW_MAX_SNAPSHOTS strictly increasing step indices >= 1
 * for every later solve (n = 0: off); -1 on bad arguments.  A solve whose numIter is below the largest index returns
 * -1 before anything is enqueued.  Every later solve copies the states S_{i_k} of its slots as the ramp passes them,
 * and every warp after it (ArapFlow_SolverWarp, SolveAsync(.., warp = 1, ..)) then writes per snapshot k and slot
 *   flow  float[H][W][2]   S_{i_k} - grid (frame-1 domain), the expression of the final flow
 *   rgb   uint8[H][W][3], mask uint8[H][W]   the rasteriser on the field S_{i_k}: the in-between frame t_k
 *   step  float[H][W][2]   flow from t_k to the next state (S_{i_(k+1)}; the final one after the last snapshot), in the
 *                          domain of t_k; 0 where nothing is drawn
 * so flow_1, step_1 .. step_n chain frame 1 -> t_1 -> .. -> t_n -> frame 2.  The optional outputs of
 * ArapFlow_SolverSetOutputs apply to the final warp only.  Device memory (28 bytes per vertex, snapshot and slot) is
 * allocated by the first solve that needs it.
 * ArapFlow_SolverGetSnapshot: synchronise and copy snapshot k (0-based, in the order given) of one slot to HOST
 * buffers, any may be NULL; -1 if the last warp wrote no such snapshot (or rgb is asked of a slot without RGB).
 * ArapFlow_SolverHostSnapshot: pointers into the solver's pinned buffers filled by a `download` solve (valid until the
 * next solve of this solver; rgb NULL if the slot has no RGB); -1 if that solve downloaded no such snapshot. */
#define ARAPFLOW_MAX_SNAPSHOTS 8
int ArapFlow_SolverSetSnapshots(ArapFlow_Solver* s, const unsigned* steps, unsigned n);
int ArapFlow_SolverGetSnapshot(ArapFlow_Solver* s, unsigned slot, unsigned k, float* flow, uint8_t* rgb, uint8_t* mask,
                               float* step);
int ArapFlow_SolverHostSnapshot(ArapFlow_Solver* s, unsigned slot, unsigned k, const float** flow, const uint8_t** rgb,
                                const uint8_t** mask, const float** step);

/* copyResultToCPU + warpField (CombinedSolver.h:280-366) on the device for slots [0, nframes):
 * flow = Offset - grid, and the forward triangle rasterisation of rgb and mask with the solved
 * Offset as warp field.  Asynchronous. */
int ArapFlow_SolverWarp(ArapFlow_Solver* s, unsigned nframes);

/* Synchronise and copy one slot's results to HOST buffers (any may be NULL):
 *   flow float[H][W][2], warped_rgb uint8[H][W][3], warped_mask uint8[H][W] (255 = object),
 *   offset float[H][W][2], angle float[H][W], final_cost = Opt_ProblemCurrentCost of the last solve. */
int ArapFlow_SolverGetResults(ArapFlow_Solver* s, unsigned slot, float* flow, uint8_t* warped_rgb,
                              uint8_t* warped_mask, float* offset, float* angle, double* final_cost);

/* Counters of the last ArapFlow_SolverSolve (for the bench): number of PCG iterations executed per
 * frame and number of active (Mask == 0) vertices summed over the solved slots. */
int ArapFlow_SolverStats(ArapFlow_Solver* s, uint64_t* pcg_iterations_per_frame, uint64_t* active_vertices,
                         uint64_t* grid_vertices);

/* The frame solver runs the PCG loop of a Gauss-Newton step either as two kernels per iteration
 * replayed from a hipGraph, or -- when every frame's active 64x4 tiles fit on chip -- as ONE resident
 * launch that keeps the PCG state in registers/LDS.  Both perform the same float32
 * operations; results are identical.  ArapFlow_SetResident(state, 0) forces the two-kernel path;
 * ArapFlow_SolverResidentLaunches counts resident launches since the solver was created. */
void ArapFlow_SetResident(Opt_State* state, int on);
/* Phase-A kernel of the two-kernel path: (0,0) = neighbours read through L1/L2, or an LDS-staged tile of (16,16),
 * (32,8), (64,4), (32,16) or (64,8) vertices -- BASELINE config 5's tile sweep; (-1,-1) = automatic (default: 64x8
 * when most tiles are active, direct otherwise).  Same arithmetic, identical results.  -1 for any other shape. */
int ArapFlow_SetTile(Opt_State* state, int tile_x, int tile_y);
uint64_t ArapFlow_SolverResidentLaunches(ArapFlow_Solver* s);
/* How the last solve's frames were dealt to resident launches: launches per Gauss-Newton step and the largest
 * number of solves in flight in one launch (every solve gets a group of the launch's 512 workgroups sized by its
 * active-tile count; small solves share an XCD).  Both 0 when the two-kernel path ran.  Returns 0, -1 on NULL. */
int ArapFlow_SolverResidentLayout(ArapFlow_Solver* s, int* launches_per_step, int* solves_in_flight);
/* Which group-sum flavour of the resident kernel each launch of a Gauss-Newton step of the last solve took: 1 = the
 * kernel that carries only the flat sum (every group dealt to the launch has <= 64 workgroups), 0 = the kernel that
 * carries all three (ARAPOPT_RES_SUMS=any, read when the state's plans are created, forces it).  Same arithmetic, identical
 * results.  Writes min(launches, cap) entries; returns the launches per step (0: the two-kernel path ran), -1 on NULL. */
int ArapFlow_SolverResidentSums(ArapFlow_Solver* s, int* sums, unsigned cap);
/* Resident launches per Gauss-Newton step that a solve of slots [0, nframes) would take with the frames set so far
 * (0: the two-kernel path would run, -1: bad arguments).  Every launch costs about the same time however full it
 * is, so a host that wants the best throughput adds frames to a batch while this stays 1 (arap_deform does). */
int ArapFlow_SolverLaunchesFor(ArapFlow_Solver* s, unsigned nframes);
/* The deal itself, as a pure host function (no device needed): given the active 64x4-tile counts of `nsolves` solves
 * (each <= 4608) it returns the number of resident launches and, when `table` is given, writes for each of the first
 * `table_launches` launches the 512 workgroup entries {solve or -1, rank in its group, group size, granule offset}
 * (int[table_launches][512][4]).  -1 on bad arguments. */
int ArapFlow_ResidentDeal(const int* active_tiles, unsigned nsolves, int* table, unsigned table_launches);
/* The resident kernel's work list of one solve, as a pure host function (no device needed): 32x8 tiles in bands of 8
 * rows; inside a band the tiles start at the band's first active vertex (`aligned` != 0; else at x = 0) and follow each
 * other every 32 columns; tiles without an active vertex (mask_red == 0) are left out.  Writes up to `cap` tile origins
 * (x0 + W * y0, band by band) and the ceil(H / 8) band start columns; returns the number of tiles, -1 on bad arguments. */
int ArapFlow_ResidentTiles(const uint8_t* mask_red, unsigned W, unsigned H, int aligned, int* origins, unsigned cap,
                           int* bandx0);
/* The drop-in path (Opt_ProblemInit/Step/Solve) takes the resident kernel too when the caller's UrShape is the
 * pixel grid on every active vertex (what the application passes, CombinedSolver.h:207-221) and the active tiles
 * fit.  Mask and UrShape are looked at before EVERY step (the reference re-reads its parameters at every step and
 * lets the caller change them in between, Opt.h:58-66): new contents or swapped buffers are honoured.  Counts the
 * resident launches executed for this plan. */
uint64_t ArapFlow_PlanResidentLaunches(Opt_Plan* plan);
/* Trust-region state of an "LMGPU" plan after the last Init / Step (read-only; any pointer may be NULL): the radius and
 * the radius decrease factor the next step starts from, the PCG iterations the last step attempted since Init ran
 * before its zeta break (0 before the first step) and how that step ended (-1 before the first step).  A Step that
 * returns 0 because nIterations steps have been taken attempts nothing and leaves all four as they were.
 * Returns 0, or -1 for a NULL or Gauss-Newton plan. */
enum { ARAPFLOW_LM_ACCEPTED = 0, ARAPFLOW_LM_REJECTED = 1, ARAPFLOW_LM_FUNCTION_TOLERANCE = 2, ARAPFLOW_LM_MIN_RADIUS = 3 };
int ArapFlow_LMState(Opt_Plan* plan, float* radius, float* decrease, int* pcg_iterations_last_step, int* outcome_last_step);
/* The resident kernel needs its 512 workgroups co-resident.  If a launch gives up at a bounded group wait (e.g.
 * another process is using the GPU), the step's update is skipped on the device, the work is redone on the
 * two-kernel path (same results) and the resident path pauses for the next 8 solve calls (doubling with every
 * further timeout, up to 1024; a checked success resets it).  Returns 1 once any launch of this state has given up. */
int ArapFlow_ResidentFailed(Opt_State* state);
/* 1 if the batch of the last solve call, where it runs kernel per phase (solves the resident kernel cannot hold, or a
 * pause after a timeout), takes the lean streaming schedule (arap_stream.h: k_pcg_a_march2 / k_pcg_b4_r: 85 + 41 bytes
 * per vertex and iteration instead of 57 + 89), which it does when most of its tiles are active. */
int ArapFlow_SolverLeanStream(ArapFlow_Solver* s);
/* Which kernels the last Gauss-Newton step this solver enqueued as a graph was made of (read-only; for tests that must
 * know they reached the kernel pair they were written for).  out[6] = {phase A, phase B, a0, a1, a2, lag}:
 *   phase A: 0 none (a resident step), 1 k_pcg_a, 2..6 k_pcg_a_lds<16x16, 32x8, 64x4, 32x16, 64x8>, 7 k_pcg_a_march<5>,
 *            8 k_pcg_a_march2<7>, 9 k_pcg_a_grid<64,8>;   phase B: 0 none, 1 k_pcg_b, 2 k_pcg_b4, 3 k_pcg_b4_lean, 4 k_pcg_b4_r;
 *   a0, a1, a2: strips (march) or 64x8 tiles (grid) in x, chunks or tiles in y, workgroups per XCD and frame;
 *   lag: the PCG iteration whose delta += alpha p is left to the update kernel (lean schedule: lIterations - 1), else -1.
 * Returns 1, 0 when the solver holds no step graph (nothing solved yet, ARAPOPT_NO_GRAPH=1, kernel timing: out is
 * {0, 0, 0, 0, 0, -1}), -1 on bad arguments. */
int ArapFlow_SolverStepRecipe(ArapFlow_Solver* s, int* out);
/* Diagnostic only (env ARAPOPT_STAMPS=1 selects an instrumented build of the resident kernel): copies
 * out[512][16] = per workgroup {phase A, wait 1, phase B, wait 2, update} summed 100 MHz ticks of the
 * last resident launch, tiles per workgroup, halo cells.  Returns -1 when stamps are off. */
int ArapFlow_SolverStamps(ArapFlow_Solver* s, uint64_t* out);
/* Diagnostic only, same build: out[512][16] = per workgroup the parts of the on-chip chain of its group sums (block sum:
 * wave tree, LDS + barrier, final level; lane tree, broadcast: shader clocks of wave 0), the summed publish times of the
 * two sums of an iteration (100 MHz), HW_ID | XCC id << 32, tiles, halo cells, border-export granules, rank | group size
 * << 16 | batch slot << 32, PCG iterations of the launch.  Returns -1 when stamps are off. */
int ArapFlow_SolverStampParts(ArapFlow_Solver* s, uint64_t* out);

/* warp_image (ARAP/warping/src/main.cpp:145-225) on DEVICE buffers: rgb uint8[H][W][3], mask_red
 * uint8[H][W], flow float[H][W][2] -> out_rgb uint8[H][W][3], out_mask uint8[H][W].
 * `scratch` is a 256-byte aligned device buffer of ArapFlow_WarpScratchBytes(W,H) bytes (64-bit keys and the job the
 * kernels read live in it).  Asynchronous on the state's stream.  Returns 0 or a HIP error code.
 * For every ArapFlow_* call on caller-owned device memory: `scratch` owes 256 bytes of alignment, every other buffer its
 * element type's (8 for float[..][2] data and the 64-bit tables, 4 for float planes and ArapFlow_MeshStats, 2 for 16-bit
 * distances, 1 for bytes) unless the call states otherwise; a call writes nothing outside the bytes stated for a buffer,
 * expects nothing of the contents of `scratch`, and enqueues all of its work on the state's stream. */
uint64_t ArapFlow_WarpScratchBytes(unsigned W, unsigned H);
int ArapFlow_Warp(Opt_State* state, unsigned W, unsigned H, const void* rgb, const void* mask_red,
                  const void* flow, void* out_rgb, void* out_mask, void* scratch);

/* ArapFlow_Warp plus the optional outputs on DEVICE buffers, each NULL when not wanted: out_bwd float[H][W][2],
 * out_occ_bwd uint8[H][W], out_occ uint8[H][W] (see ArapFlow_SolverSetOutputs).  `scratch` is a 256-byte aligned
 * device buffer of ArapFlow_WarpExScratchBytes(W,H) bytes.  With all three NULL this is ArapFlow_Warp.  Asynchronous
 * on the state's stream.  Returns 0, -1 on bad arguments, or a HIP error code. */
uint64_t ArapFlow_WarpExScratchBytes(unsigned W, unsigned H);
int ArapFlow_WarpEx(Opt_State* state, unsigned W, unsigned H, const void* rgb, const void* mask_red,
                    const void* flow, void* out_rgb, void* out_mask, void* out_bwd, void* out_occ_bwd, void* out_occ,
                    void* scratch);

/* The warp of flow_a plus the flow from that warped frame to a second state (DESIGN.md "In-between frames"), on
 * DEVICE buffers: flow_a, flow_b float[H][W][2] are two deformations of the same frame as flows (positions
 * (float)x + flow.x, (float)y + flow.y, as in ArapFlow_Warp).  out_rgb / out_mask: ArapFlow_Warp's of flow_a (out_rgb
 * and rgb may be NULL).  out_step float[H][W][2]: per pixel q of the warped frame, with the triangle drawn there, the
 * point of state b interpolated with the rasteriser's barycentrics of state a, minus q; 0 where nothing is drawn.  With
 * flow_b = 0 it is ArapFlow_WarpEx's backward flow bit for bit.  The call allocates its own scratch and returns when
 * the outputs are written.  Returns 0, -1 on bad arguments, or a HIP error code. */
int ArapFlow_WarpStep(Opt_State* state, unsigned W, unsigned H, const void* rgb, const void* mask_red,
                      const void* flow_a, const void* flow_b, void* out_rgb, void* out_mask, void* out_step);

/* Layered warp (DESIGN.md "Layered warp"): ONE rasteriser pass over the n layers of a frame -- the --multseg segments in
 * list order, the higher index on top -- on DEVICE buffers: rgb uint8[H][W][3] shared by all layers (or NULL: no
 * out_rgb), masks_red uint8[n][H][W] (0 = object), flows float[n][H][W][2].  Outputs, each NULL when not wanted:
 * the composite out_rgb / out_mask / out_bwd / out_occ_bwd (bit for bit what the host merge of n ArapFlow_WarpEx calls
 * gives) and out_occ, the forward occlusion ACROSS layers, which n separate calls cannot give: a frame-1 pixel is
 * occluded when it leaves the frame or a triangle of a higher layer, or a later triangle of its own layer, is drawn over
 * its landing point; lower layers never occlude.  With n = 1 every output equals ArapFlow_WarpEx's.
 * `scratch`: 256-byte aligned device buffer of ArapFlow_WarpLayersScratchBytes(W, H, n) bytes.  Asynchronous on the
 * state's stream.  Returns 0; -1 on bad arguments: n = 0, n > 255, no output at all, out_rgb without rgb,
 * W * H >= 2^31, or out_occ with W * H > 2^24 (the field widths of the keys and of a binned vertex); else a HIP error
 * code. */
uint64_t ArapFlow_WarpLayersScratchBytes(unsigned W, unsigned H, unsigned n);
int ArapFlow_WarpLayers(Opt_State* state, unsigned W, unsigned H, unsigned n, const void* rgb, const void* masks_red,
                        const void* flows, void* out_rgb, void* out_mask, void* out_bwd, void* out_occ_bwd,
                        void* out_occ, void* scratch);

/* Layered in-between frames (DESIGN.md "Layered in-between frames"): the layered warp of a state a of all n layers, the
 * flow from that composite frame to a second state b and the forward occlusion of that link, on DEVICE buffers laid out
 * as in ArapFlow_WarpLayers; flows_a, flows_b float[n][H][W][2] are the layers' two states as flows.  Outputs, each
 * NULL when not wanted: out_rgb / out_mask, ArapFlow_WarpLayers' of flows_a; out_step float[H][W][2], per covered pixel
 * q of the composite the point d(q) of state b of the winner's layer, interpolated with the rasteriser's barycentrics
 * of state a, minus q, and 0 where nothing is drawn (n = 1: ArapFlow_WarpStep's out_step; flows_b = 0:
 * ArapFlow_WarpLayers' out_bwd); out_occ uint8[H][W], 255 where what pixel q shows is hidden in the next frame: d(q)
 * leaves the frame, or a triangle of a higher layer, or a triangle of the same layer later than every triangle that
 * shares a corner with the winner, is drawn over d(q) in state b; for an uncovered q, where state b draws anything at
 * q.  Lower layers never occlude.  With out_step == out_occ == NULL the call does ArapFlow_WarpLayers' work for RGB
 * and mask.
 * `scratch`: 256-byte aligned device buffer of ArapFlow_WarpLayersStepScratchBytes(W, H, n) bytes (48 per pixel).
 * Asynchronous on the state's stream.  Returns 0; -1 on bad arguments: n = 0, n > 255, no output at all, out_rgb
 * without rgb, W * H >= 2^31, or out_occ with W * H > 2^24; else a HIP error code. */
uint64_t ArapFlow_WarpLayersStepScratchBytes(unsigned W, unsigned H, unsigned n);
int ArapFlow_WarpLayersStep(Opt_State* state, unsigned W, unsigned H, unsigned n, const void* rgb,
                            const void* masks_red, const void* flows_a, const void* flows_b, void* out_rgb,
                            void* out_mask, void* out_step, void* out_occ, void* scratch);

/* Point tracks through a sequence (DESIGN.md "Point tracks"): where P caller-given sub-pixel points of frame 1 are in
 * each of T states of the n layers of a frame, and whether they can be seen there, on DEVICE buffers: masks_red as in
 * ArapFlow_WarpLayers, flows float[T][n][H][W][2] the states of the layers as flows, points float[P][2] in frame-1
 * coordinates.  A point's owner is the topmost (layer, triangle) of frame 1 that holds it; out_pos float[T][P][2] is
 * the point carried by its owner into state s with the owner's barycentrics (a point of the background, or outside
 * the frame, stays where it is); out_occ uint8[T][P] is 255 where the point leaves the frame in state s, or a triangle
 * of a higher layer, or a triangle of the owner's layer later than every triangle that shares a corner with the owner,
 * is drawn over it there -- ArapFlow_WarpLayersStep's rule; a point outside the frame (or NaN) is 255 in every state.
 * With the points the W * H integer pixels in index order, out_occ of state s is the out_occ of
 * ArapFlow_WarpLayersStep(flows_a = 0, flows_b = flows[s]) and out_pos - pixel its out_step on covered pixels.
 * Either output may be NULL, not both.  P may exceed W * H.
 * `scratch`: 256-byte aligned device buffer of ArapFlow_TrackPointsScratchBytes(W, H, T, P) bytes (per state
 * 4 (W * H + 1) + 37 P, and 32 P once; 0 for sizes the call refuses).  Touches no key image.  Asynchronous on the
 * state's stream.  Returns 0; -1, and nothing is launched, on bad arguments: a null state, input or scratch, both
 * outputs NULL, n = 0, n > 255, W * H = 0 or >= 2^31, P = 0 or > 2^24, T = 0 or > ARAPFLOW_MAX_SNAPSHOTS + 1; else a HIP
 * error code. */
uint64_t ArapFlow_TrackPointsScratchBytes(unsigned W, unsigned H, unsigned T, unsigned P);
int ArapFlow_TrackPoints(Opt_State* state, unsigned W, unsigned H, unsigned n, const void* masks_red, unsigned T,
                         const void* flows, unsigned P, const void* points, void* out_pos, void* out_occ,
                         void* scratch);

/* Moving background (DESIGN.md "Moving background"): the point maps between two frames whose background is sampled
 * through the affine maps M1, M2 (six floats (a, b, c, d, e, f): pixel (x, y) shows the background point
 * (a x + b y + c, d x + e y + f)).  G = M2^-1 o M1 (frame 1 -> frame 2) and Ginv = M1^-1 o M2, derived in double and
 * rounded once to float; bit-equal M1 and M2 give the exact identity for both.  Host only.  Returns 0, or -1 on a null
 * pointer, a non-finite coefficient or a linear part with zero determinant. */
int ArapFlow_BackgroundMaps(const float M1[6], const float M2[6], float G[6], float Ginv[6]);

/* Full-frame RGB, flow and occlusion behind the objects of a warped pair, on DEVICE buffers (M1, M2: host).  bg
 * uint8[bgH][bgW][3] is the background picture; frame 1 has its object where mask_red uint8[H][W] is 0, frame 2 where
 * cover2 uint8[H][W] (a warp's out_mask) is not 0.  Outputs, each NULL when not wanted -- an output that is NULL is not
 * computed and its input not read:
 *   out_rgb1 / out_rgb2 uint8[H][W][3]   rgb1 / rgb2 on the object, else the bilinear sample (clamp to edge) of bg at
 *                                        M1 (x, y) / M2 (x, y)
 *   flow_full float[H][W][2]             `flow` on the frame-1 object, else G (x, y) - (x, y)
 *   occ_full uint8[H][W]                 `occ` on the frame-1 object, else 255 where G (x, y) leaves the frame or cover2
 *                                        is set at its nearest pixel
 *   bwd_full float[H][W][2]              `bwd` on the frame-2 object, else Ginv (x, y) - (x, y)
 *   occ_bwd_full uint8[H][W]             `occ_bwd` on the frame-2 object, else 255 where Ginv (x, y) leaves the frame or
 *                                        mask_red is 0 at its nearest pixel
 * No output may alias an input.  Needs no scratch.  Asynchronous on the state's stream.  Returns 0; -1 on bad arguments:
 * a null state, bg, mask_red or cover2, a zero size, W * H >= 2^31, an output whose input (rgb1, rgb2, flow, occ, bwd,
 * occ_bwd in the order above) is NULL, no output at all, or maps ArapFlow_BackgroundMaps refuses; else a HIP error code. */
int ArapFlow_Background(Opt_State* state, unsigned W, unsigned H, const void* bg, unsigned bgW, unsigned bgH,
                        const float M1[6], const float M2[6], const void* rgb1, const void* mask_red, const void* rgb2,
                        const void* cover2, const void* flow, const void* occ, const void* bwd, const void* occ_bwd,
                        void* out_rgb1, void* out_rgb2, void* flow_full, void* occ_full, void* bwd_full,
                        void* occ_bwd_full);

/* Moving background over a sequence of frames (DESIGN.md "Moving background over in-between frames"): frame 1, the
 * in-between frames t_1 .. t_n of a pair and frame 2 are nframes = n + 2 frames F_0 .. F_{nframes-1}, joined by
 * nframes - 1 links F_f -> F_{f+1}; one launch does ArapFlow_Background's frame-1 work for every link.  maps
 * float[nframes][6] (host) are the sampling maps of the frames; the point map of link f is the G of
 * ArapFlow_BackgroundMaps(maps[f], maps[f+1]).  F_0 has its object where mask_red is 0, F_f (f >= 1) where covers[f]
 * (a warp's out_mask) is not 0.  The other arguments are HOST arrays of DEVICE pointers (a NULL array: every entry
 * NULL), buffers as in ArapFlow_Background:
 *   covers[nframes]       entry 0 unused
 *   rgbs[nframes]         the frames' object-side RGB
 *   flows[nframes-1]      the object-side flow of link f, in the domain of F_f
 *   occs[nframes-1]       the object-side occlusion of link f
 *   out_rgbs[nframes]     rgbs[f] on the object of F_f, else the bilinear sample of bg at maps[f] (x, y)
 *   out_flows[nframes-1]  flows[f] on the object of F_f, else G_f (x, y) - (x, y)
 *   out_occs[nframes-1]   occs[f] on the object of F_f, else 255 where G_f (x, y) leaves the frame or covers[f+1] is
 *                         set at its nearest pixel
 * An output entry that is NULL is not computed and its input not read.  With nframes = 2 the outputs are
 * ArapFlow_Background's out_rgb1, flow_full, occ_full and out_rgb2, bit for bit.  No output may alias an input.  Needs
 * no scratch.  Asynchronous on the state's stream.  Returns 0; -1, and nothing is launched, on bad arguments: a null
 * state, bg, maps, mask_red, covers or covers[f] for f >= 1, nframes outside 2 .. ARAPFLOW_MAX_SNAPSHOTS + 2, a zero
 * size, W * H >= 2^31, an output whose object-side input is NULL, no output at all, or two consecutive maps that
 * ArapFlow_BackgroundMaps refuses; else a HIP error code. */
int ArapFlow_BackgroundSeq(Opt_State* state, unsigned W, unsigned H, const void* bg, unsigned bgW, unsigned bgH,
                           unsigned nframes, const float* maps, const void* mask_red, const void* const* covers,
                           const void* const* rgbs, const void* const* flows, const void* const* occs,
                           void* const* out_rgbs, void* const* out_flows, void* const* out_occs);

/* Random textures (DESIGN.md "Random textures"): one procedural texture per layer of a frame, for the random-texture twin
 * of a pair.  A layer's texture is a pure function of the pixel, the layer's seed and these few parameters:
 *   kind        one of ARAPFLOW_TEX_*
 *   seed        of the layer's hash; any value
 *   m           six floats (a, b, c, d, e, f), pixel -> texture point as in ArapFlow_BackgroundMaps: pixel (x, y) shows
 *               the point (u, v) = (a x + b y + c, d x + e y + f); one texture cell is one unit of (u, v)
 *   p0, p1      BRICK: the mortar's width as a fraction of a cell, the shift of odd rows in cells; WAVE: the amplitude of
 *               the noise that bends the bands, in cells, and the profile (p1 < 0.5: saw, else triangle); else unused
 *   c0, c1, c2  the palette, RGB: CHECKER c0 / c1; BRICK c0 / c1 bricks, c2 mortar; VORONOI and WAVE between c0 and c1;
 *               NOISE the ramp c0 -> c1 -> c2
 *   reserved    not read */
enum { ARAPFLOW_TEX_CHECKER = 0, ARAPFLOW_TEX_BRICK = 1, ARAPFLOW_TEX_VORONOI = 2, ARAPFLOW_TEX_NOISE = 3,
       ARAPFLOW_TEX_WAVE = 4 };
typedef struct ArapFlow_TexLayer {
    uint32_t kind, seed;
    float m[6];
    float p0, p1;
    uint8_t c0[3], c1[3], c2[3], reserved[3];
} ArapFlow_TexLayer;

/* Retexture the objects of a frame, on DEVICE buffers (layers: HOST, n entries): rgb uint8[H][W][3], masks_red
 * uint8[n][H][W] (0 = object, the layers of ArapFlow_WarpLayers in the same order; NULL: every pixel belongs to layer 0)
 * -> out_rgb uint8[H][W][3].  A pixel belongs to the HIGHEST layer index whose mask is 0 there -- the layered warp's
 * stacking order -- and gets that layer's texture colour; a pixel of no layer gets rgb's bytes.  The result is a function
 * of the arguments alone: two runs give identical bytes, and a layer's pixels do not depend on the other layers'
 * descriptions.  Warping out_rgb with the frame's solved flows (ArapFlow_Warp / WarpLayers) gives the twin's second
 * frame; the flows are shared.  Needs no scratch beyond the layer table (52 bytes a layer), which the state allocates at
 * the first call and the call copies before it returns.  Asynchronous on the state's stream.  Returns 0; -1, and nothing
 * is launched or written, on bad arguments: a null state, rgb, layers or out_rgb, n = 0 or n > 255, a zero size,
 * W * H >= 2^31, an unknown kind, a non-finite map coefficient or parameter, or out_rgb overlapping rgb or masks_red;
 * else a HIP error code. */
int ArapFlow_Texture(Opt_State* state, unsigned W, unsigned H, unsigned n, const void* rgb, const void* masks_red,
                     const ArapFlow_TexLayer* layers, void* out_rgb);

/* Motion blur (DESIGN.md "Motion blur"): a frame exposed over a window of time, as the integer mean of `samples` layered
 * warps of the same mesh at `samples` moments of the window.  The layers are ArapFlow_WarpLayersStep's: masks_red
 * uint8[n][H][W] (0 = object), two states as flows, flows_a and flows_b float32[n][H][W][2], a shared rgb; flows_a == NULL
 * means all zero and gives the same bytes as an array of zeros.
 *   times    t_k = centre + shutter * ((k + 0.5) / samples - 0.5), k = 0 .. samples - 1, computed in double from the float32
 *            centre and shutter and rounded once to float32; samples = 1 gives t_0 = centre.  t may leave [0, 1]: a frame
 *            exposed around 0 extrapolates the motion backwards for the first half of its window.
 *   sample   the flow field f = u * a + t * b with u = 1.0f - t, float32, one IEEE operation per operator; sample k is, by
 *            definition, what ArapFlow_WarpLayers writes as out_rgb / out_mask for flows = f.
 *   bg       optional: a picture uint8[bgH][bgW][3] and two sampling maps Ma, Mb (six floats each, as in
 *            ArapFlow_Background).  Sample k sees the picture through u * Ma[i] + t * Mb[i] per coefficient (float32, on the
 *            host) -- through Ma itself when Ma and Mb are bit-equal -- and a pixel the sample leaves uncovered contributes
 *            that sample of the picture (ArapFlow_Background's bilinear sample).  Without bg it contributes 0 (out_rgb is
 *            then premultiplied colour).
 *   outputs  with sum the integer sum of a channel over the samples and cnt the number of samples that cover the pixel:
 *            out_rgb = (2 sum + samples) / (2 samples), out_alpha = (2 * 255 * cnt + samples) / (2 samples), integer
 *            division (round half up).  Either may be NULL, not both.  No float is added across samples: two runs give
 *            identical bytes.
 * ArapFlow_BlurSchedule is the one place the times and maps are derived (host only, needs no device; the device call
 * uses it): times[samples], maps[samples][6] or NULL (Ma and Mb are then not read).  Returns 0, or -1: times NULL, samples
 * = 0 or > ARAPFLOW_MAX_BLUR_SAMPLES, a non-finite centre, a non-finite or negative shutter, maps without Ma and Mb or
 * with a non-finite coefficient.
 * ArapFlow_BlurLayers works on DEVICE buffers (Ma, Mb: HOST).  Samples are rasterised ARAPFLOW_BLUR_CHUNK at a time, each
 * into a key image of its own, and summed per pixel in registers; no image per sample exists.  `scratch`: 256-byte aligned
 * device buffer of ArapFlow_BlurLayersScratchBytes(W, H, n, samples) bytes -- per pixel 8 * min(samples, ARAPFLOW_BLUR_CHUNK)
 * for the keys and 8 more for the carried sums when samples > ARAPFLOW_BLUR_CHUNK; 0 for sizes the call refuses.  The call
 * clears what it needs of it.  Asynchronous on the state's stream.  Returns 0; -1, and nothing is launched or written, on
 * bad arguments: a null state, rgb, masks_red, flows_b or scratch, both outputs NULL, n = 0 or n > 255, W * H = 0 or
 * >= 2^31, samples = 0 or > ARAPFLOW_MAX_BLUR_SAMPLES, a non-finite or negative shutter, a non-finite centre, bg without
 * both maps or with a zero picture size or a non-finite coefficient, an output overlapping an input; else a HIP error
 * code. */
#define ARAPFLOW_MAX_BLUR_SAMPLES 32
#define ARAPFLOW_BLUR_CHUNK 8
int ArapFlow_BlurSchedule(float centre, float shutter, unsigned samples, const float Ma[6], const float Mb[6], float* times,
                          float* maps);
uint64_t ArapFlow_BlurLayersScratchBytes(unsigned W, unsigned H, unsigned n, unsigned samples);
int ArapFlow_BlurLayers(Opt_State* state, unsigned W, unsigned H, unsigned n, const void* rgb, const void* masks_red,
                        const void* flows_a, const void* flows_b, float centre, float shutter, unsigned samples,
                        const void* bg, unsigned bgW, unsigned bgH, const float Ma[6], const float Mb[6], void* out_rgb,
                        void* out_alpha, void* scratch);

/* Relit frames (DESIGN.md "Relit frames"): a finished frame (objects over their background) under one soft shadow of the
 * objects on the background, a tone curve, a smooth illumination field, a vignette and sensor noise.  The geometry is
 * untouched, so a relit pair shares the clean pair's flow, occlusion and track files.  One frame's description (HOST):
 *   seed            of the frame's hash (ArapFlow_Texture's h); any value
 *   m               six floats, pixel -> field point (u, v) = (a x + b y + c, d x + e y + f) as in ArapFlow_TexLayer; one
 *                   value-noise cell of the illumination field per unit
 *   amp             >= 0: amplitude of the illumination field
 *   vig             0 .. 1: depth of the vignette at the frame's corner
 *   gain[3], gamma  > 0, finite: the tone curve per channel
 *   sh_dx, sh_dy    |.| <= ARAPFLOW_LIGHT_MAX_SHIFT: where the shadow falls relative to the object, in pixels
 *   sh_r            0 .. ARAPFLOW_LIGHT_MAX_R: radius of the penumbra (a box of 2 sh_r + 1 pixels a side)
 *   sh_g            0 .. 256: depth of the shadow in 256ths; 0 = no shadow
 *   sigma0, sigma1  >= 0: standard deviation of the noise in grey levels, the constant part and the part per grey level
 * Every float finite.  Derived on the host, in one place (ArapFlow_LightTables, needs no device; the device call uses it):
 *   lut[c][i] = floor(255 * min(max(gain[c] * pow(i / 255, gamma), 0), 1) + 0.5), in double with the C library's pow;
 *               gamma = 1, gain = 1 is the identity table
 *   geom      = (cx, cy, inv_r2) = ((W - 1) / 2, (H - 1) / 2, 1 / (cx^2 + cy^2)), in double, each rounded once to float32;
 *               inv_r2 = 0 when W = H = 1
 * Per pixel (x, y), channel c, input byte v0, with obj(p) the cover predicate at pixel p -- cover[p] != 0, or == 0 with
 * cover_is_mask (the solver's convention); false for every p outside the frame -- and every float operator one IEEE
 * float32 operation in the order of the parentheses (no fused multiply-add but inside vn, ArapFlow_Texture's value noise):
 *   shadow   only if sh_g > 0 and !obj(x, y), else v1 = v0:  a = #{(i, j): |i| <= r, |j| <= r, obj(x - sh_dx + i, y - sh_dy
 *            + j)}, A = (2 r + 1)^2, v1 = (v0 * (256 A - sh_g * a) + 128 A) / (256 A), integer division (below 2^32)
 *   tone     v2 = lut[c][v1]
 *   shading  L = 1.0f + amp * (2.0f * vn(seed, u, v, 0) - 1.0f),
 *            V = 1.0f - vig * min(((fx - cx) * (fx - cx) + (fy - cy) * (fy - cy)) * inv_r2, 1.0f),  fx = (float)x, fy = (float)y
 *            v3 = (float)v2 * (L * V)
 *   noise    n = (((r0 + r1) + (r2 + r3)) - 2.0f) * 1.7320508f, r_j = r01(h(seed, x, y, 1 + 4 c + j)): zero mean, unit variance
 *            v4 = v3 + (sigma0 + sigma1 * v3) * n
 *   out      (uint8)(min(max(v4, 0.0f), 255.0f) + 0.5f)
 * The neutral description (amp = vig = 0, gain = gamma = 1, sh_g = 0, sigma0 = sigma1 = 0) returns the input bytes; the
 * output is a function of the arguments alone; an object pixel does not depend on the cover beyond its own bit.
 * ArapFlow_LightTables returns 0, or -1: a null pointer, a zero size, W * H >= 2^31, a field outside its range or
 * non-finite.
 * ArapFlow_Relight works on DEVICE buffers (frame: HOST): rgb uint8[H][W][3], cover uint8[H][W] (may be NULL when sh_g = 0,
 * and is then not read) -> out_rgb uint8[H][W][3].  Needs no scratch beyond the 768-byte table, which the state allocates
 * at the first call and the call copies before it returns.  Asynchronous on the state's stream.  Returns 0; -1, and
 * nothing is launched or written, on bad arguments: a null state, rgb, frame or out_rgb, a zero size, W * H >= 2^31, a
 * field outside its range or non-finite, sh_g > 0 without a cover, out_rgb overlapping rgb or cover; else a HIP error
 * code. */
#define ARAPFLOW_LIGHT_MAX_R 16
#define ARAPFLOW_LIGHT_MAX_SHIFT 64
typedef struct ArapFlow_LightFrame {
    uint32_t seed;
    float m[6];
    float amp, vig;
    float gain[3], gamma;
    int32_t sh_dx, sh_dy, sh_r, sh_g;
    float sigma0, sigma1;
} ArapFlow_LightFrame;
int ArapFlow_LightTables(const ArapFlow_LightFrame* frame, unsigned W, unsigned H, uint8_t lut[3][256], float geom[3]);
int ArapFlow_Relight(Opt_State* state, unsigned W, unsigned H, const void* rgb, const void* cover, int cover_is_mask,
                     const ArapFlow_LightFrame* frame, void* out_rgb);

/* Segment maps (DESIGN.md "Segment maps"): the object index maps of both frames of a pair, the motion boundaries of its
 * forward and backward flow, and the squared distance to the nearest boundary.  The layers are ArapFlow_WarpLayers':
 * masks_red uint8[n][H][W] (0 = object), flows float32[n][H][W][2], the higher index on top.
 *   idx1   uint8[H][W]: the owner of the frame-1 pixel (the largest l with masks_red[l] == 0) + 1; 0: no layer owns it.
 *   idx2   uint8[H][W]: the layer of the layered rasteriser's winner at the frame-2 pixel + 1; 0: nothing drawn there.
 *          idx2 != 0 exactly where ArapFlow_WarpLayers' out_mask != 0.
 *   F1, B2 the full flows, no outputs: F1(p) = flows[owner][p] on an owned pixel, B2(q) = ArapFlow_WarpLayers' out_bwd on
 *          a covered one; elsewhere the moving background's flow_full / bwd_full expression of ArapFlow_Background for
 *          the cameras M1, M2 (HOST, six floats each), or exactly (0, 0) when both are NULL.  Bit-equal M1 and M2 give the
 *          bytes of the static call.
 *   mb1    uint8[H][W]: 255 where F1 jumps against a 4-neighbour q inside the frame, !(dx * dx + dy * dy <= tau * tau)
 *          with (dx, dy) = F1(p) - F1(q), every operator one float32 operation, tau * tau formed once; else 0.  A
 *          non-finite difference is a jump; both sides of a jump are marked.  mb2: the same on B2.
 *   dist1  uint16[H][W]: the exact squared Euclidean distance in pixels to the nearest pixel with mb1 = 255 if that is
 *          <= radius^2, else 65535 (also in a frame without boundary).  dist2: the same on mb2.
 * Any output may be NULL, not all six; a pass no output needs is not launched: without idx2, mb2 and dist2 nothing is
 * rasterised, without dist1 and dist2 no distance pass runs.  Integer atomics of the rasteriser only, no float
 * reduction: two runs give identical bytes.  `scratch`: 256-byte aligned device buffer of
 * ArapFlow_SegMapsScratchBytes(W, H, n) bytes -- per pixel 8 (key image) + 8 (full flow) + 1 (boundary map) + 1 (column
 * distance) = 18, however many layers, plus a few hundred bytes; 0 for sizes the call refuses.  The call clears what it
 * needs of it.  Asynchronous on the state's stream.  Returns 0; -1, and nothing is launched or written, on bad arguments:
 * a null state, masks_red, flows or scratch, all six outputs NULL, n = 0 or n > 255, W * H = 0 or >= 2^31, exactly one of
 * M1 / M2, maps ArapFlow_BackgroundMaps refuses, a negative or non-finite tau, radius > ARAPFLOW_SEG_MAX_RADIUS, an
 * output overlapping an input, the scratch or another output; else a HIP error code. */
#define ARAPFLOW_SEG_MAX_RADIUS 254
uint64_t ArapFlow_SegMapsScratchBytes(unsigned W, unsigned H, unsigned n);
int ArapFlow_SegMaps(Opt_State* state, unsigned W, unsigned H, unsigned n, const void* masks_red, const void* flows,
                     const float M1[6], const float M2[6], float tau, unsigned radius, void* idx1, void* idx2, void* mb1,
                     void* mb2, void* dist1, void* dist2, void* scratch);

/* Flow scoring (DESIGN.md "Flow scoring"): the error table of an estimated flow against n pairs of one size, on DEVICE
 * buffers.  gt, est float32[n][H][W][2], the ground truth and the estimate; occ uint8[n][H][W], non-zero = occluded (every
 * occlusion map here); dist uint16[n][H][W], ArapFlow_SegMaps' squared distance with 65535 = none within the radius;
 * skip uint8[n][H][W], non-zero = the pixel is left out (a fold map is one); each of the three may be NULL.  Per pixel,
 * every operator one float32 operation, sqrtf correctly rounded:
 *   du = est.x - gt.x;  dv = est.y - gt.y;  e2 = du * du + dv * dv;  e = sqrtf(e2);  g2 = gt.x * gt.x + gt.y * gt.y
 *   ec = (e <= 4096.f) ? e : 4096.f                      (NaN and +inf land on the cap)
 *   q  = (uint32)(ec * 4096.f + 0.5f)                    (truncation: the end-point error in units of 2^-12 px, <= 2^24)
 * A pixel with skip != 0 is counted in row 9, field 0, and nowhere else; otherwise one with !(g2 < inf), a non-finite
 * ground truth, in row 9, field 1, and nowhere else; every other pixel is counted: in row 0 and in at most one row of each
 * group
 *   row 0 all
 *   row 1 noc      occ given and occ == 0             row 2 occ      occ given and occ != 0
 *   row 3 d0-10    dist given and dist < 100          row 4 d10-60   dist given and 100 <= dist < 3600
 *   row 5 d60-140  dist given and 3600 <= dist < 19600
 *   row 6 s0-10    g2 < 100.f       row 7 s10-40   100.f <= g2 < 1600.f       row 8 s40+   g2 >= 1600.f
 * The fields of a row, each uint64:
 *   0 count   1 sum: the sum of q   2 n1: !(e2 <= 1.f)   3 n3: !(e2 <= 9.f)   4 n5: !(e2 <= 25.f)
 *   5 fl: !(e2 <= 9.f) && !(e2 <= 0.0025f * g2), KITTI's Fl outlier   6 nonfinite: !(e2 < inf)   7 max: the largest q
 * so the mean end-point error of a class is sum / 4096 / count, to 2^-13 px.  A class whose plane is NULL stays zero.
 *   table  uint64[n][ARAPFLOW_SCORE_ROWS][ARAPFLOW_SCORE_FIELDS]; the call clears it itself.
 *   err    float32[n][H][W] or NULL: e as computed on a counted pixel, -1.f on every other.
 * Integer atomics only, no float reduction: two runs give identical bytes.  One launch whatever n; the flows are read 16
 * bytes at a time where gt, est and err are 16-byte, dist 8-byte, occ and skip 4-byte aligned (a pair whose W * H is odd
 * included), one pixel at a time otherwise.  Needs no scratch.  Asynchronous on the state's stream.  Returns 0; -1, and
 * nothing is launched or written, on bad arguments: a null state, gt, est or table, n = 0, W * H = 0, n * W * H >= 2^31,
 * an output overlapping an input or the other output; else a HIP error code. */
#define ARAPFLOW_SCORE_ROWS 10
#define ARAPFLOW_SCORE_FIELDS 8
int ArapFlow_FlowScore(Opt_State* state, unsigned W, unsigned H, unsigned n, const void* gt, const void* est,
                       const void* occ, const void* dist, const void* skip, void* table, void* err);

/* Track scoring (DESIGN.md "Track scoring"): the TAP-Vid table of estimated point tracks against the tracks of a track
 * file, on DEVICE buffers in a track file's layout.  gt_pos, est_pos float32[F][P][2]; gt_occ, est_occ uint8[F][P],
 * non-zero = hidden.  Frame 0 is the query frame and is not scored.  Point k is valid iff gt_occ[0][k] == 0:
 *   table[0][0][0] = the number of valid points, table[0][0][1] = the number of invalid ones, the rest of frame 0 is zero,
 * and an invalid point is counted nowhere else.  For a valid point k and a frame f >= 1, every operator one float32
 * operation, sqrtf correctly rounded:
 *   dx = (est.x - gt.x) * sx;  dy = (est.y - gt.y) * sy;  e2 = dx * dx + dy * dy;  e = sqrtf(e2)
 *   ec = (e <= 4096.f) ? e : 4096.f                      (NaN and +inf land on the cap)
 *   q  = (uint32)(ec * 4096.f + 0.5f)                    (truncation: the error in units of 2^-12 px, <= 2^24)
 *   gv = gt_occ[f][k] == 0;  ev = est_occ[f][k] == 0;  in_x = gv && (e2 < x * x)   for x = 1, 2, 4, 8, 16
 * The point-frame is counted in
 *   class 0 all         always
 *   class 1 tracked     gv, and the ground truth is visible in every frame 1 .. f-1
 *   class 2 reappeared  gv, and the ground truth is hidden in some frame 1 .. f-1
 * The fields of a class, each uint64:
 *   0 count   1 gt_vis: gv   2 est_vis: ev   3 agree: gv == ev   4..8 within_x: in_x   9..13 tp_x: in_x && ev
 *   14 sum: the sum of q over gv   15 max: the largest q over gv
 * so per class and frame OA = agree / count, delta_x = within_x / gt_vis, J_x = tp_x / (gt_vis + est_vis - tp_x), and the
 * mean error of the visible points is sum / 4096 / gt_vis.
 *   table  uint64[F][ARAPFLOW_TSCORE_CLASSES][ARAPFLOW_TSCORE_FIELDS]; the call clears it itself.
 * Integer atomics only, no float reduction: two runs give identical bytes.  One launch, no scratch, asynchronous on the
 * state's stream.  Returns 0; -1, and nothing is launched or written, on bad arguments: a null state, buffer or table,
 * P = 0 or P > 2^24, F < 2 or F > ARAPFLOW_TSCORE_MAX_FRAMES, sx or sy not finite or <= 0, the table overlapping an input;
 * else a HIP error code. */
#define ARAPFLOW_TSCORE_MAX_FRAMES 64
#define ARAPFLOW_TSCORE_CLASSES 3
#define ARAPFLOW_TSCORE_FIELDS 16
int ArapFlow_TrackScore(Opt_State* state, unsigned F, unsigned P, const void* gt_pos, const void* gt_occ,
                        const void* est_pos, const void* est_occ, float sx, float sy, void* table);

/* Flow chaining (DESIGN.md "Track scoring"): estimated tracks from per-link flow estimates, on DEVICE buffers.  flows
 * float32[L][H][W][2], link j the estimated flow from sequence frame j to j + 1 on the integer pixels of frame j; bwd the
 * same shape or NULL, link j the estimated flow from frame j + 1 back to j; points float32[P][2] in frame 0.  With
 * in_frame(a): 0 <= a.x <= W - 1 && 0 <= a.y <= H - 1 (false on NaN) and the bilinear sample, per component,
 *   S(A, a):  x0 = (int)floorf(a.x); y0 = (int)floorf(a.y); x1 = min(x0 + 1, W - 1); y1 = min(y0 + 1, H - 1)
 *             fx = a.x - (float)x0;  fy = a.y - (float)y0
 *             top = fmaf(fx, A[y0][x1] - A[y0][x0], A[y0][x0]);  bot = fmaf(fx, A[y1][x1] - A[y1][x0], A[y1][x0])
 *             v   = fmaf(fy, bot - top, top)
 * a point p is chained as
 *   pos[0] = p;  lost = !in_frame(p);  occ[0] = lost ? 255 : 0
 *   link j, lost:  pos[j+1] = pos[j];  occ[j+1] = 255
 *   otherwise:     f = S(flows[j], pos[j]);  b = (pos[j].x + f.x, pos[j].y + f.y);  pos[j+1] = b
 *                  !in_frame(b):  lost = true, occ[j+1] = 255      (for good; decided before any floorf of b)
 *                  else occ[j+1] = 0, and with bwd:  g = S(bwd[j], b);  s = f + g
 *                       d2 = s.x * s.x + s.y * s.y;  m2 = (f.x * f.x + f.y * f.y) + (g.x * g.x + g.y * g.y)
 *                       occ[j+1] = !(d2 <= fmaf(0.01f, m2, 0.5f)) ? 255 : 0      (forward-backward check; per link)
 *   out_pos float32[L + 1][P][2], out_occ uint8[L + 1][P]: a track file's planes, ArapFlow_TrackScore's est_pos, est_occ.
 * One launch, no scratch, asynchronous on the state's stream.  Returns 0; -1, and nothing is launched, on bad arguments:
 * a null state, flows, points or output, L = 0 or L >= ARAPFLOW_TSCORE_MAX_FRAMES, P = 0 or P > 2^24, W * H = 0 or
 * >= 2^31, an output overlapping an input or the other output; else a HIP error code. */
int ArapFlow_ChainFlows(Opt_State* state, unsigned W, unsigned H, unsigned L, const void* flows, const void* bwd,
                        unsigned P, const void* points, void* out_pos, void* out_occ);

/* Frame scoring (DESIGN.md "Frame scoring"): the PSNR / integer-SSIM table of n estimated frames against n reference
 * frames of one size, on DEVICE buffers.  ref, est uint8[n][H][W][3]; occ uint8[n][H][W], non-zero = occluded; dist
 * uint16[n][H][W], ArapFlow_SegMaps' squared distance with 65535 = none; skip uint8[n][H][W], non-zero = left out; obj
 * uint8[n][H][W], a mask in the solver's convention, 0 = object, non-zero = background; each of the four may be NULL.
 *   pixel:   d_c = |ref_c - est_c|;  sse = d_0^2 + d_1^2 + d_2^2;  sad = d_0 + d_1 + d_2;  mx = max(d_0, d_1, d_2)
 *   luma:    Y = (77 R + 150 G + 29 B + 128) >> 8
 *   window:  every 8 x 8 window wholly in the frame, stride 1: (W - 7)(H - 7) of them, none when W < 8 or H < 8.  With
 *            a = Y(ref), b = Y(est) over its 64 pixels, in integers (each below 2^31 in magnitude, B signed):
 *              s1 = sum a;  s2 = sum b;  ss = sum (a * a + b * b);  s12 = sum a * b
 *              vars = 64 * ss - s1 * s1 - s2 * s2;  covar = 64 * s12 - s1 * s2
 *              A = 2 * s1 * s2 + 416;  B = 2 * covar + 235963;  C = s1 * s1 + s2 * s2 + 416;  D = vars + 235963
 *            then, every operator one float32 operation, the division correctly rounded:
 *              s = ((float)A * (float)B) / ((float)C * (float)D);  t = max(s + 1.0f, 0.0f)
 *              q = (uint32)(t * 1048576.f + 0.5f)                 (truncation; 2^21 for identical windows, never more)
 *            The anchor of the window with top-left (x, y) is the pixel (x + 3, y + 3); a window belongs to the rows its
 *            anchor belongs to.
 * A pixel with skip != 0 is counted in row 8, field 0, and nowhere else; a window whose anchor has skip != 0 in row 8,
 * field 1, and nowhere else (its 64 pixels are whatever they are).  Every other pixel or anchor is counted in
 *   row 0 all
 *   row 1 noc      occ given and occ == 0             row 2 occ      occ given and occ != 0
 *   row 3 d0-10    dist given and dist < 100          row 4 d10-60   dist given and 100 <= dist < 3600
 *   row 5 d60-140  dist given and 3600 <= dist < 19600
 *   row 6 obj      obj given and obj == 0             row 7 bg       obj given and obj != 0
 * The fields of a row 0..7, each uint64:
 *   0 count: pixels   1 sse   2 sad   3 max: the largest mx   4 windows   5 ssim_sum: the sum of q
 *   6 ssim_worst: the largest 2^21 - q
 * A row whose plane is NULL stays zero.  Tables pool by adding every field but 3 and 6, which take the maximum.
 *   table  uint64[n][ARAPFLOW_FSCORE_ROWS][ARAPFLOW_FSCORE_FIELDS]; the call clears it itself.
 *   ssim   float32[n][H][W] or NULL: s as computed at the anchor of a counted window, -2.f at every other pixel.
 * Integer atomics only, no float reduction: two runs give identical bytes.  One launch whatever n; the frames are read 16
 * bytes at a time where ref and est are 16-byte aligned (whatever W * H), byte by byte otherwise.  Needs no scratch.
 * Asynchronous on the state's stream.  Returns 0; -1, and nothing is launched or written, on bad arguments: a null state,
 * ref, est or table, n = 0, W * H = 0, n * W * H >= 2^31, an output overlapping an input or the other output; else a HIP
 * error code. */
#define ARAPFLOW_FSCORE_ROWS 9
#define ARAPFLOW_FSCORE_FIELDS 7
int ArapFlow_FrameScore(Opt_State* state, unsigned W, unsigned H, unsigned n, const void* ref, const void* est,
                        const void* occ, const void* dist, const void* skip, const void* obj, void* table, void* ssim);

/* Map scoring (DESIGN.md "Map scoring"): the scorers of the fourth kind of ground truth, the maps -- DAVIS J (region
 * similarity) and F (boundary accuracy) per object of estimated label maps, and the precision / recall histogram of
 * estimated occlusion or motion-boundary maps -- over n maps of one size, on DEVICE buffers, in integers only.
 *   gt, est  uint8[n][H][W];  skip uint8[n][H][W] or NULL, non-zero = the pixel is left out;  a pixel with skip == 0 (or
 *            no skip plane) is "counted".  radius 0 .. ARAPFLOW_SEG_MAX_RADIUS.
 * Boundary match of two pixel sets A (from gt) and B (from est): the skipped pixels are removed from both (they are
 * neither counted nor targets); a = |A|, b = |B|; a_hit = the number of p in A for which some q in B has
 * (p.x - q.x)^2 + (p.y - q.y)^2 <= radius^2; b_hit the same with the roles swapped.  With radius 0 a hit is the same
 * pixel.  (The DAVIS toolkit's f_measure: dilation by disk(radius), then intersection; no thinning.)
 * bmap(m) of a binary map m, the toolkit's seg2bmap at equal size: for x < W-1, y < H-1:
 *   b = m[y][x] != m[y][x+1] | m[y][x] != m[y+1][x] | m[y][x] != m[y+1][x+1];  last row, x < W-1: m[y][x] != m[y][x+1];
 *   last column, y < H-1: m[y][x] != m[y+1][x];  the bottom-right pixel: 0.  It is formed on the whole mask, skipped
 *   pixels included; the match then removes them (the toolkit's handling of void pixels).
 *
 * ArapFlow_LabelScore: gt, est are label maps (ArapFlow_SegMaps' idx1 / idx2: 0 = no object), 1 <= L <= 255 labels are
 * scored.  table uint64[n][L + 1][ARAPFLOW_LSCORE_FIELDS], cleared by the call:
 *   row 0:            0 counted pixels  1 skipped pixels  2 counted with gt == est  3 counted with gt > L
 *                     4 counted with est > L  5..7 zero
 *   row k, 1..L:      0 gt: counted with gt == k  1 est: counted with est == k  2 inter: counted with both
 *                     3 gt_b, 4 est_b, 5 gt_hit, 6 est_hit: a, b, a_hit, b_hit of the boundary match of
 *                     A = bmap(gt == k), B = bmap(est == k)   7 zero
 * ArapFlow_MapScore: gt is binary (non-zero = positive), est a score 0..255 (a hard map written 0 / 255 is one).
 *   hist   uint64[n][2][256], cleared by the call: hist[c][v] = the counted pixels with (gt != 0) == c and est == v; the
 *          skipped pixels are W * H minus its sum.
 *   m, thr 0 <= m <= ARAPFLOW_MSCORE_MAX_THR thresholds, a HOST array, each 1..255; for threshold j the boundary match
 *          of A = {gt != 0}, B = {est >= thr[j]} goes to match uint64[n][m][4] as (a, b, a_hit, b_hit), cleared by the
 *          call.  With m = 0 thr, match and scratch may be NULL and neither a set nor a distance pass is launched.
 * scratch: ArapFlow_MapScoreScratchBytes(W, H) bytes (7 a pixel, 256-byte aligned, whatever n, L and m; 0 for sizes the
 * calls refuse), 256-byte aligned; it serves both calls.
 * Integer atomics only: two runs give identical bytes and tables add exactly.  Asynchronous on the state's stream.
 * Return 0; -1, and nothing is launched or written, on bad arguments: a null state, gt, est, table or hist, n = 0,
 * W * H = 0, n * W * H >= 2^31, L = 0 or L > 255, radius > ARAPFLOW_SEG_MAX_RADIUS, m > ARAPFLOW_MSCORE_MAX_THR, a
 * threshold of 0 or above 255, m > 0 with a null thr, match or scratch, a label call with a null scratch, an output
 * (the scratch is one) overlapping an input or another output; else a HIP error code. */
#define ARAPFLOW_LSCORE_FIELDS 8
#define ARAPFLOW_MSCORE_MAX_THR 8
uint64_t ArapFlow_MapScoreScratchBytes(unsigned W, unsigned H);
int ArapFlow_LabelScore(Opt_State* state, unsigned W, unsigned H, unsigned n, unsigned L, unsigned radius, const void* gt,
                        const void* est, const void* skip, void* table, void* scratch);
int ArapFlow_MapScore(Opt_State* state, unsigned W, unsigned H, unsigned n, const void* gt, const void* est,
                      const void* skip, unsigned m, const unsigned* thr, unsigned radius, void* hist, void* match,
                      void* scratch);

/* Frames from flows (DESIGN.md "Frames from flows"): the in-between frames of a pair at K times from an estimated flow,
 * by flow splatting (Baker et al., IJCV 2011, section 3.3.2: splat the flow to time t, fill small holes, fetch both frames
 * along the flow with an occlusion test, blend), in integers wherever a result is stored.  On DEVICE buffers, but for
 * `times`.
 *   A, B   uint8[H][W][3], frame 1 and frame 2;  fwd float32[H][W][2], the estimated flow A -> B on A's pixels;
 *   bwd    the same shape or NULL, the estimated flow B -> A on B's pixels;
 *   times  float32[K], a HOST array, 1 <= K <= ARAPFLOW_INTERP_MAX_TIMES, each finite and 0 < t < 1.
 * N = W * H < 2^31.  in_frame(p): 0 <= p.x <= W - 1 and 0 <= p.y <= H - 1, false on NaN; S(F, a): the bilinear flow
 * sample of ArapFlow_ChainFlows.  A flow value is valid when both components are finite and below 1e9 in magnitude.
 * s = 1.0f - t; tq = (int)(t * 256.f + 0.5f); every fmaf below is one fused operation, every other operator one float32
 * operation; nearest(v, hi) = min((int)floorf(v + .5f), hi) (the clamp acts only beyond 2^23).
 * Step 1, splat.  One 64-bit key per pixel and time, cleared to all ones, updated with a minimum.
 *   Side A, pixel x = (i, j) with u = fwd[j][i] valid:  e = (i + u.x, j + u.y);  cost = 766 when !in_frame(e), else
 *   cost = sum_c |A[x][c] - B[q][c]| with q = (nearest(e.x, W - 1), nearest(e.y, H - 1)); the cost does not depend on t.
 *   For each time: p = (fmaf(t, u.x, (float)i), fmaf(t, u.y, (float)j)); nothing is written when !in_frame(p); else
 *   r = (nearest(p.x, W - 1), nearest(p.y, H - 1)) and key[k][r] = min(key[k][r], cost << 32 | 0 << 31 | (j * W + i)).
 *   Side B, only with bwd, pixel y = (i, j) with g = bwd[j][i] valid: the cost the same way, |B[y][c] - A[q][c]| at
 *   e = y + g;  p = (fmaf(s, g.x, (float)i), fmaf(s, g.y, (float)j));  the key carries a 1 in bit 31 and stands for the
 *   flow u = -g.
 *   The winner is the lowest cost; on equal cost side A wins, within a side the lowest source index.
 * Step 2, hole fill.  A pixel without a key takes the key of the nearest keyed pixel of its own row at distance
 *   d = 1 .. ARAPFLOW_INTERP_FILL, the left one at equal d; if there is none the pixel is a hole.
 * Step 3, colour at pixel r = (x, y).  The integer bilinear colour sample C(I, a), a inside the frame:
 *   x0 = floorf(a.x), x1 = min(x0 + 1, W - 1), wx = (int)((a.x - x0) * 256.f + .5f), the same in y;
 *   C_c = (256-wx)(256-wy) I[y0][x0][c] + wx (256-wy) I[y0][x1][c] + (256-wx) wy I[y1][x0][c] + wx wy I[y1][x1][c].
 *   A hole: out_c = ((256 - tq) * A[r][c] + tq * B[r][c] + 128) >> 8, src = 255.
 *   Any other pixel, u the flow its key stands for (fwd[index], or -bwd[index] with bit 31):
 *     a0 = (fmaf(-t, u.x, (float)x), fmaf(-t, u.y, (float)y));  b1 = (fmaf(s, u.x, (float)x), fmaf(s, u.y, (float)y))
 *     okA = in_frame(a0) and, with f0 = S(fwd, a0), d = f0 - u:
 *           d.x * d.x + d.y * d.y <= fmaf(0.01f, (f0.x * f0.x + f0.y * f0.y) + (u.x * u.x + u.y * u.y), 0.5f)
 *     okB = in_frame(b1) and, where bwd is given, with g1 = S(bwd, b1), d = u + g1:
 *           d.x * d.x + d.y * d.y <= fmaf(0.01f, (u.x * u.x + u.y * u.y) + (g1.x * g1.x + g1.y * g1.y), 0.5f)
 *     (both tests false on NaN)
 *     both:     out_c = ((256 - tq) * C_c(A, a0) + tq * C_c(B, b1) + 2^23) >> 24        (fits 32 bits)
 *     one:      out_c = (C_c + 32768) >> 16 of that side
 *     neither:  the hole formula
 *     src = 0 both, 1 A only, 2 B only, 3 neither, plus 4 when the key came from the hole fill.
 *   out      uint8[K][H][W][3]
 *   src      uint8[K][H][W] or NULL
 *   scratch  a 256-byte aligned device buffer of ArapFlow_InterpScratchBytes(W, H, K) bytes, the caller's: the K * N
 *            64-bit keys, rounded up to 256 bytes (0 for sizes the call refuses)
 * Two kernels behind one clear of the keys, each launched once for all K times; the only atomics are the 64-bit integer
 * minima on the keys, so two runs give identical bytes.  Nothing is launched or allocated unless the call is made.
 * Asynchronous on the state's stream.  Returns 0; -1, and nothing is launched or written, on bad arguments: a null state,
 * A, B, fwd, times, out or scratch, K = 0 or K > 32, a time that is not finite or not in (0, 1), W * H = 0 or >= 2^31,
 * K * W * H >= 2^31, an output or the scratch overlapping an input or each other; else a HIP error code. */
#define ARAPFLOW_INTERP_MAX_TIMES 32
#define ARAPFLOW_INTERP_FILL 16
uint64_t ArapFlow_InterpScratchBytes(unsigned W, unsigned H, unsigned K);
int ArapFlow_InterpFrames(Opt_State* state, unsigned W, unsigned H, const void* A, const void* B, const void* fwd,
                          const void* bwd, unsigned K, const float* times, void* out, void* src, void* scratch);

/* Fold diagnostics (DESIGN.md "Fold diagnostics"; off by default, and then nothing is allocated or launched): how much
 * of a warped mesh inverted or went non-finite, and which frame-1 pixels carry a flow value that is no valid
 * correspondence.  With P(v) the warp position of vertex v (the solved Offset, or (x, y) + flow) and the rasterised
 * triangles t = 2u (p00, p01, p10), t = 2u + 1 (p10, p01, p11) of every quad whose four corners are object,
 *   det(t) = (e1.x * e2.y) - (e1.y * e2.x),  e1 = P(c1) - P(c0),  e2 = P(c2) - P(c0)      (float32, uncontracted)
 * is +1 on the pixel grid.  A triangle is non-finite iff det is not finite, folded iff det is finite and <= 0.
 *   vertices, outside   object vertices; those of them whose P is not inside [0, W-1] x [0, H-1] (NaN counts)
 *   triangles           rasterised triangles;  folded, nonfinite: as above;  reserved: 0
 *   det_min, det_max    over the finite dets, in the total order of the IEEE bit patterns (-0 < +0); +inf / -inf when
 *                       there is none
 *   disp2_max           max of (dx * dx) + (dy * dy), dx = P.x - (float)x, dy = P.y - (float)y, over the object
 *                       vertices whose P has two finite coordinates; 0 when there is none
 * The fold map uint8[H][W] (frame-1 domain) is 255 where the vertex is object and a corner of a folded or non-finite
 * rasterised triangle, else 0.  Counts, flags and order-independent extrema only: two runs give identical bytes. */
typedef struct ArapFlow_MeshStats {
    uint32_t vertices, outside, triangles, folded, nonfinite, reserved;
    float det_min, det_max, disp2_max;
} ArapFlow_MeshStats;

/* The diagnostics of a flow on DEVICE buffers: mask_red uint8[H][W], flow float[H][W][2] -> out_fold uint8[H][W],
 * out_stats one ArapFlow_MeshStats (a DEVICE pointer too), each NULL when not wanted.  Needs no scratch beyond a few
 * hundred bytes the state allocates at the first call.  Asynchronous on the state's stream.  Returns 0; -1 on bad
 * arguments: a null state, mask_red or flow, both outputs NULL, a zero size or W * H >= 2^31; else a HIP error code. */
int ArapFlow_WarpDiag(Opt_State* state, unsigned W, unsigned H, const void* mask_red, const void* flow, void* out_fold,
                      ArapFlow_MeshStats* out_stats);

/* The same for the frame solver: ArapFlow_SolverSetDiag(s, on) makes every later warp (ArapFlow_SolverWarp,
 * SolveAsync(.., warp = 1, ..)) compute the statistics and the fold map of its slots' solved fields; the redo after a
 * resident time-out re-runs them with the warp.  Device memory (one byte per vertex and slot, plus the statistics) is
 * allocated by the first call that turns them on.  Returns 0, -1 on a null solver.
 * ArapFlow_SolverGetDiag: synchronise and copy one slot's diagnostics of the last warp to HOST buffers (either may be
 * NULL); -1 if that warp computed none.
 * ArapFlow_SolverHostDiag: pointers into the solver's pinned buffers filled by a `download` solve (valid until the next
 * solve of this solver); -1 if that solve downloaded none. */
int ArapFlow_SolverSetDiag(ArapFlow_Solver* s, int on);
int ArapFlow_SolverGetDiag(ArapFlow_Solver* s, unsigned slot, ArapFlow_MeshStats* stats, uint8_t* fold);
int ArapFlow_SolverHostDiag(ArapFlow_Solver* s, unsigned slot, const ArapFlow_MeshStats** stats, const uint8_t** fold);

/* Training batches (DESIGN.md "Training batches"; the numpy twin is tests/aug_ref.py): B pairs of one source size W x H,
 * each under its own geometric and photometric augmentation, cropped to w x h, normalised and laid out planar, in one
 * launch.  DEVICE inputs, stacked like ArapFlow_FlowScore's pairs:
 *   rgb1, rgb2   uint8[B][H][W][3]
 *   flow         float[B][H][W][2], on frame 1's pixels
 *   skip         uint8[B][H][W] or NULL: non-zero = no ground truth at that pixel
 * DEVICE outputs, each NULL when not wanted (then it is not computed, and inputs only it needs are not read and may be
 * NULL: img1 needs rgb1, img2 needs rgb2, out_flow and valid need flow):
 *   img1, img2   float[B][3][h][w]
 *   out_flow     float[B][2][h][w]
 *   valid        uint8[B][h][w], 0 or 255
 * Per sample a HOST ArapFlow_AugSample; per call scale[3], bias[3] (the normalisation) and tau >= 0 or +inf.
 * Every float operator below is one IEEE float32 operation in the order of the parentheses; there is no fused
 * multiply-add anywhere.  (float)x, (float)y: the output pixel's coordinates converted first.
 *   q_k = ((a * x + b * y) + c, (d * x + e * y) + f), (a .. f) = T_k: the source point of frame k that output pixel
 *         (x, y) shows
 *   Tables (ArapFlow_AugmentTables, a pure host function; the device call uses the same code):
 *     P2 = the inverse of T2 as a map, in IEEE double: det = a e - b d,
 *          P2 = (e / det, -b / det, (b f - e c) / det, -d / det, a / det, (d c - a f) / det), each rounded once to float
 *     lut[k][c][i] = (float)((255 * min(max(gain_k[c] * pow(i / 255, gamma_k), 0), 1)) * scale[c] + bias[c]), in double
 *          with the C library's pow, rounded once.  Neutral (gain = gamma = scale = 1, bias = 0): lut[i] == i.
 *   Taps of a point q in a W x H plane:  inside = q.x >= 0 && q.x <= W-1 && q.y >= 0 && q.y <= H-1 (false on NaN);
 *     bx = fminf(fmaxf(q.x, 0), (float)(W-1));  x0 = min((int)floorf(bx), W-1);  x1 = min(x0 + 1, W-1);
 *     fx = bx - (float)x0;  the same in y.  Tap ij is the pixel (x_j, y_i).
 *   mix(c00, c01, c10, c11) = top + fy * (bot - top),  top = c00 + fx * (c01 - c00),  bot = c10 + fx * (c11 - c10)
 *   Images:  img_k[c][y][x] = mix of lut[k][c][byte] at the four taps of q_k (not rounded); img2 is then fill[c] where
 *     (x, y) lies in any of the sample's rectangles erase[i] = (x0, y0, x1, y1), half-open, output pixels.
 *   Flow, at the taps of q1:  tap 01 is used iff fx > 0, tap 10 iff fy > 0, tap 11 iff both, tap 00 always.  An unused
 *     tap is replaced by tap 00 (it is not read).  A tap is bad iff its skip byte is non-zero or a flow component is not
 *     finite; a bad tap's value is (0, 0) in what follows.
 *       u      = mix of the four values, per component
 *       spread = max over the taps of max(|f.x - f00.x|, |f.y - f00.y|)
 *       out.x  = (((P2.a * q1.x + P2.b * q1.y) + P2.c) - (float)x) + (P2.a * u.x + P2.b * u.y);  out.y with d, e, f
 *       valid  = inside(q1) && no tap bad && spread <= tau && out.x and out.y finite
 *     Where !valid: out_flow = (0, 0), valid = 0; else valid = 255.  spread <= tau is the motion-boundary guard.
 * One kernel, one launch (grid.z = B), no atomics, no scratch: two runs give identical bytes.  The per-sample table
 * lives in device memory the state owns (allocated at the first call, grown with B) and is copied stream-ordered
 * before the call returns.  Nothing is allocated or launched unless the call is made.
 * ArapFlow_AugmentTables returns 0; -1 on a null pointer, a non-finite coefficient of T1 or T2, det(T2) == 0 in double,
 * or a gain or gamma that is not finite and > 0.  (n_erase, the rectangles and fill are not read.)
 * ArapFlow_AugmentPairs is asynchronous on the state's stream.  Returns 0; -1, and nothing is launched or written, on: a
 * null state, samples, scale or bias, a null input that an asked output needs, every output NULL, a zero size, W * H >= 2^31 or
 * B * w * h >= 2^31, B > ARAPFLOW_AUG_MAX_BATCH, a sample that ArapFlow_AugmentTables refuses or whose n_erase exceeds
 * ARAPFLOW_AUG_MAX_ERASE, tau NaN or negative, an output overlapping an input it reads or another output; else a HIP
 * error code. */
#define ARAPFLOW_AUG_MAX_BATCH 64
#define ARAPFLOW_AUG_MAX_ERASE 4
typedef struct ArapFlow_AugSample {
    float T1[6], T2[6];
    float gain1[3], gamma1, gain2[3], gamma2;
    uint32_t n_erase;
    int32_t erase[ARAPFLOW_AUG_MAX_ERASE][4];
    float fill[3];
} ArapFlow_AugSample;
int ArapFlow_AugmentTables(const ArapFlow_AugSample* sample, const float scale[3], const float bias[3], float P2[6],
                           float lut[2][3][256]);
int ArapFlow_AugmentPairs(Opt_State* state, unsigned W, unsigned H, unsigned w, unsigned h, unsigned B, const void* rgb1,
                          const void* rgb2, const void* flow, const void* skip, const ArapFlow_AugSample* samples,
                          const float scale[3], const float bias[3], float tau, void* img1, void* img2, void* out_flow,
                          void* valid);

/* Training clips (DESIGN.md "Training clips"; the numpy twin is tests/clip_ref.py): B clips of one source size W x H, each
 * of T frames, L flow links and P tracked points, every frame under its own augmentation, cropped to w x h, normalised
 * and laid out planar, in at most two launches.  Notation and arithmetic are those of "Training batches" above: q, the
 * taps, mix, the used / bad-tap rule and the spread guard are reused word for word (the kernels call the same device
 * functions), every float operator is one IEEE float32 operation in the order of the parentheses, no fused multiply-add.
 * Shapes: W * H < 2^31; B * T * w * h < 2^31; 1 <= B <= ARAPFLOW_AUG_MAX_BATCH; 1 <= T <= ARAPFLOW_CLIP_MAX_FRAMES and
 * B * T <= 256; 0 <= L <= ARAPFLOW_CLIP_MAX_LINKS and B * L * w * h < 2^31; 0 <= P and B * T * P < 2^31.
 * DEVICE inputs:
 *   frames   uint8[B][T][H][W][3]
 *   flows    float[B][L][H][W][2]: link l is a flow on the pixels of frame links[l][0] towards frame links[l][1]
 *   skip     uint8[B][L][H][W] or NULL: non-zero = no ground truth at that pixel of that link
 *   pos      float[B][T][P][2]: a point's position in each source frame
 *   occ      uint8[B][T][P]: 255 (non-zero) = hidden in that frame
 * HOST inputs: links int32[L][2], one table per call, 0 <= i, j < T and i != j, repeats allowed; samples
 * ArapFlow_ClipFrame[B][T]; scale[3], bias[3], tau as in ArapFlow_AugmentPairs.
 * DEVICE outputs, each NULL when not wanted (then it is not computed; an input that only unasked outputs need is not read,
 * may be NULL and takes no part in the checks: video needs frames; out_flows and valid need links and flows; tracks needs
 * pos; vis needs pos and occ):
 *   video      float[B][T][3][h][w]
 *   out_flows  float[B][L][2][h][w]
 *   valid      uint8[B][L][h][w], 0 or 255
 *   tracks     float[B][T][P][2]
 *   vis        uint8[B][T][P], 0 or 255
 * A frame's description, ArapFlow_ClipFrame (120 bytes): T, output pixel -> source point of this frame; gain, gamma, the
 * tone curve; fill and n_erase <= ARAPFLOW_AUG_MAX_ERASE rectangles erase[i] = (x0, y0, x1, y1), half-open, output pixels.
 *   Tables (ArapFlow_ClipTables, a pure host function; the device call uses the same code, and ArapFlow_AugmentTables is
 *     made of the same per-frame pieces): P = the inverse of T as a map and lut[c][i], by the expressions given for P2
 *     and lut[k] above.
 *   Video:  video[b][t] = img of "Training batches" with T = T_{b,t} and that frame's lut, then fill[c] where (x, y) lies
 *     in any of that frame's rectangles.  Any frame may carry rectangles.
 *   Links:  for link l = (i, j), out_flows[b][l] and valid[b][l] are the pair definition's out_flow and valid with
 *     T1 := T_{b,i}, P2 := P_{b,j} and the flow and skip planes [b][l].  Rectangles do not touch valid.
 *   Tracks: p = pos[b][t][k], P = P_{b,t}:
 *     o      = ((P.a * p.x + P.b * p.y) + P.c, (P.d * p.x + P.e * p.y) + P.f)
 *     fin    = |o.x| <= FLT_MAX && |o.y| <= FLT_MAX (false on NaN); where it is false, o = (0, 0)
 *     in     = fin && o.x >= 0 && o.x <= (float)(w - 1) && o.y >= 0 && o.y <= (float)(h - 1)
 *     erased (only where in): rx = (int)floorf(o.x + 0.5f), ry alike; (rx, ry) lies in any rectangle of frame (b, t)
 *     tracks = o, always (a hidden point keeps its position);  vis = (occ == 0 && in && !erased) ? 255 : 0
 * Two kernels at the most: k_augment_clip (grid (tiles, T + L, B): a block is a 64 x 16 tile of one frame or one link)
 * when video, out_flows or valid is asked, k_clip_tracks (grid (ceil(P / 256), T, B)) when tracks or vis is.  No
 * atomics, no scratch: two runs give identical bytes.  The per-frame table and the link table live in device memory the
 * state owns (allocated at the first call, grown with B * T) and are copied stream-ordered, in one copy, before the call
 * returns.
 * ArapFlow_ClipTables returns 0; -1 on a null pointer, a non-finite coefficient of T, det(T) == 0 in double, or a gain
 * or gamma that is not finite and > 0.  (n_erase, the rectangles and fill are not read.)
 * ArapFlow_AugmentClips is asynchronous on the state's stream.  Returns 0; -1, and nothing is launched or written, on: a
 * null state, samples, scale or bias; every output NULL; a zero W, H, w, h, B or T; a limit above exceeded; out_flows or
 * valid asked with L == 0 or null links; tracks or vis asked with P == 0; a null input that an asked output needs; a
 * link out of range or with i == j (where a link output is asked); a frame that ArapFlow_ClipTables refuses or whose
 * n_erase exceeds ARAPFLOW_AUG_MAX_ERASE; tau NaN or negative; an output overlapping an input it reads or another
 * output; else a HIP error code. */
#define ARAPFLOW_CLIP_MAX_FRAMES 16
#define ARAPFLOW_CLIP_MAX_LINKS 32
typedef struct ArapFlow_ClipFrame {
    float T[6];
    float gain[3], gamma;
    float fill[3];
    uint32_t n_erase;
    int32_t erase[ARAPFLOW_AUG_MAX_ERASE][4];
} ArapFlow_ClipFrame;
int ArapFlow_ClipTables(const ArapFlow_ClipFrame* frame, const float scale[3], const float bias[3], float P[6],
                        float lut[3][256]);
int ArapFlow_AugmentClips(Opt_State* state, unsigned W, unsigned H, unsigned w, unsigned h, unsigned B, unsigned T,
                          unsigned L, unsigned P, const void* frames, const int32_t* links, const void* flows,
                          const void* skip, const void* pos, const void* occ, const ArapFlow_ClipFrame* samples,
                          const float scale[3], const float bias[3], float tau, void* video, void* out_flows, void* valid,
                          void* tracks, void* vis);

#ifdef __cplusplus
}
#endif
#endif /* ARAP_OPT_H */
