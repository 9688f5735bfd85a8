// arapopt.hip -- libarapopt.so: host side of the MI355X-native ARAP solver + the C ABI of
// include/arap_opt.h.  Built for gfx950 only (see arap_flow_amd/build.py).
//
// Host-side structure mirrors the reference's plan lifecycle:
//   Opt_NewState/ProblemDefine/ProblemPlan   createwrapper.t:124-220, o.t:2521-2558
//   init / step / cost / setSolverParameter  solverGPUGaussNewton.t:956-1007, 1016-1177, 1179-1221
// but one Gauss-Newton step is a single hipGraph launch (2 + 2*lIterations + 1 kernel nodes and one
// memset node) with every PCG scalar kept in device memory: no per-iteration memset/memcpy calls,
// no host round trip inside a solve (the reference issues ~4 tiny API calls per PCG iteration,
// solverGPUGaussNewton.t:1058-1091, and a blocking read-back per step, :790-797).
//
// This file is the single translation unit (kernel symbols must be visible where they are launched); the code
// lives in the headers below, device first, then host in dependency order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/arap_opt.h"
#include "arap_kernels.h"
#include "arap_resident.h"
#include "arap_lm.h"
#include "arap_tiled.h"
#include "arap_stream.h"
#include "arap_warp.h"
#include "arap_occ.h"
#include "arap_layers.h"
#include "arap_mid.h"
#include "arap_layers_step.h"
#include "arap_track.h"
#include "arap_bg.h"
#include "arap_tex.h"
#include "arap_blur.h"
#include "arap_light.h"
#include "arap_seg.h"
#include "arap_score.h"
#include "arap_tscore.h"
#include "arap_chain.h"
#include "arap_fscore.h"
#include "arap_mscore.h"
#include "arap_interp.h"
#include "arap_diag.h"
#include "arap_frame.h"
#include "arap_aug.h"
#include "arap_clip.h"

using namespace arap;

#define ARAPOPT_VERSION "arapopt 0.1.0 gfx950"

#include "host_plan.h"       // state, plan, knobs, timed launches
#include "host_resident.h"   // resident path: tile lists, deal of solves to workgroups, failure and back-off
#include "host_step.h"       // StepRecipe, one Gauss-Newton step, its graph cache, init / step
#include "host_lm.h"         // "LMGPU" host loop
#include "abi_opt.h"         // Opt_* drop-in ABI and the small ArapFlow_* entry points
#include "abi_warp.h"        // warp scratch layout, ArapFlow_Warp*
#include "abi_seg.h"         // ArapFlow_SegMaps
#include "abi_score.h"       // ArapFlow_FlowScore
#include "abi_tscore.h"      // ArapFlow_TrackScore, ArapFlow_ChainFlows
#include "abi_fscore.h"      // ArapFlow_FrameScore
#include "abi_mscore.h"      // ArapFlow_LabelScore, ArapFlow_MapScore
#include "abi_interp.h"      // ArapFlow_InterpFrames
#include "abi_solver.h"      // ArapFlow_Solver*
#include "abi_aug.h"         // ArapFlow_AugmentTables, ArapFlow_AugmentPairs
#include "abi_clip.h"        // ArapFlow_ClipTables, ArapFlow_AugmentClips
