"""ctypes binding of libarapopt.so (include/arap_opt.h).

There is no CPU fallback: if the HIP library is missing or no GPU is present, loading/creating a
state raises.  Nothing here imports the oracle.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ARAPOPT_LIB") or os.path.join(_HERE, "lib", "libarapopt.so")     # (ARAPOPT_LIB: kernel experiments)


class Opt_InitializationParameters(C.Structure):
    """Opt.h:10-30"""
    _fields_ = [("doublePrecision", C.c_int), ("verbosityLevel", C.c_int),
                ("collectPerKernelTimingInfo", C.c_int), ("threadsPerBlock", C.c_int)]


class MeshStats(C.Structure):
    """ArapFlow_MeshStats (DESIGN.md "Fold diagnostics")"""
    _fields_ = [("vertices", C.c_uint32), ("outside", C.c_uint32), ("triangles", C.c_uint32), ("folded", C.c_uint32),
                ("nonfinite", C.c_uint32), ("reserved", C.c_uint32), ("det_min", C.c_float), ("det_max", C.c_float),
                ("disp2_max", C.c_float)]


class TexLayer(C.Structure):
    """ArapFlow_TexLayer (DESIGN.md "Random textures")"""
    _fields_ = [("kind", C.c_uint32), ("seed", C.c_uint32), ("m", C.c_float * 6), ("p0", C.c_float), ("p1", C.c_float),
                ("c0", C.c_uint8 * 3), ("c1", C.c_uint8 * 3), ("c2", C.c_uint8 * 3), ("reserved", C.c_uint8 * 3)]


class LightFrame(C.Structure):
    """ArapFlow_LightFrame (DESIGN.md "Relit frames")"""
    _fields_ = [("seed", C.c_uint32), ("m", C.c_float * 6), ("amp", C.c_float), ("vig", C.c_float), ("gain", C.c_float * 3),
                ("gamma", C.c_float), ("sh_dx", C.c_int32), ("sh_dy", C.c_int32), ("sh_r", C.c_int32), ("sh_g", C.c_int32),
                ("sigma0", C.c_float), ("sigma1", C.c_float)]


class AugSample(C.Structure):
    """ArapFlow_AugSample (DESIGN.md "Training batches")"""
    _fields_ = [("T1", C.c_float * 6), ("T2", C.c_float * 6), ("gain1", C.c_float * 3), ("gamma1", C.c_float),
                ("gain2", C.c_float * 3), ("gamma2", C.c_float), ("n_erase", C.c_uint32), ("erase", (C.c_int32 * 4) * 4),
                ("fill", C.c_float * 3)]


class ClipFrame(C.Structure):
    """ArapFlow_ClipFrame (DESIGN.md "Training clips")"""
    _fields_ = [("T", C.c_float * 6), ("gain", C.c_float * 3), ("gamma", C.c_float), ("fill", C.c_float * 3),
                ("n_erase", C.c_uint32), ("erase", (C.c_int32 * 4) * 4)]


TEX_KINDS = ("checker", "brick", "voronoi", "noise", "wave")      # ARAPFLOW_TEX_*: a kind's number is its index here

MESH_STATS_KEYS = tuple(k for k, _ in MeshStats._fields_ if k != "reserved")     # the order of a diag file's lines


# every symbol include/arap_opt.h declares: (name, restype, argtypes)
_VP, _U, _I = C.c_void_p, C.c_uint, C.c_int
SYMBOLS = [
    ("Opt_NewState", _VP, [Opt_InitializationParameters]),
    ("Opt_ProblemDefine", _VP, [_VP, C.c_char_p, C.c_char_p]),
    ("Opt_ProblemDelete", None, [_VP, _VP]),
    ("Opt_ProblemPlan", _VP, [_VP, _VP, C.POINTER(C.c_uint)]),
    ("Opt_PlanFree", None, [_VP, _VP]),
    ("Opt_SetSolverParameter", None, [_VP, _VP, C.c_char_p, _VP]),
    ("Opt_ProblemSolve", None, [_VP, _VP, C.POINTER(_VP)]),
    ("Opt_ProblemInit", None, [_VP, _VP, C.POINTER(_VP)]),
    ("Opt_ProblemStep", _I, [_VP, _VP, C.POINTER(_VP)]),
    ("Opt_ProblemCurrentCost", C.c_double, [_VP, _VP]),
    ("ArapFlow_Version", C.c_char_p, []),
    ("ArapFlow_FreeState", None, [_VP]),
    ("ArapFlow_SetStream", None, [_VP, _VP]),
    ("ArapFlow_UseOwnStream", _I, [_VP]),
    ("ArapFlow_TimerBegin", None, [_VP]),
    ("ArapFlow_TimerEnd", C.c_float, [_VP]),
    ("ArapFlow_SetKernelTiming", None, [_VP, _I]),
    ("ArapFlow_KernelTime", _I, [_VP, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    ("ArapFlow_EvalJTF", _I, [_VP, _U, _U, _VP, _VP, _VP, _VP, _VP, C.c_float, C.c_float, _VP, _VP, _VP, _VP]),
    ("ArapFlow_ApplyJTJ", _I, [_VP, _U, _U, _VP, _VP, _VP, _VP, C.c_float, C.c_float, _VP, _VP, _VP, _VP]),
    ("ArapFlow_Cost", _I, [_VP, _U, _U, _VP, _VP, _VP, _VP, _VP, C.c_float, C.c_float, C.POINTER(C.c_double)]),
    ("ArapFlow_SolverCreate", _VP, [_VP, _U, _U, _U]),
    ("ArapFlow_SolverFree", None, [_VP]),
    ("ArapFlow_SolverSetFrame", _I, [_VP, _U, _VP, _VP, _VP, _U, _I]),
    ("ArapFlow_SolverSolve", _I, [_VP, _U, _U, _U, _U]),
    ("ArapFlow_SolverSolveAsync", _I, [_VP, _U, _U, _U, _U, _I, _I]),
    ("ArapFlow_SolverWait", _I, [_VP]),
    ("ArapFlow_SolverHostResults", _I, [_VP, _U, C.POINTER(_VP), C.POINTER(_VP), C.POINTER(_VP)]),
    ("ArapFlow_SolverWarp", _I, [_VP, _U]),
    ("ArapFlow_SolverGetResults", _I, [_VP, _U, _VP, _VP, _VP, _VP, _VP, C.POINTER(C.c_double)]),
    ("ArapFlow_SolverStats", _I, [_VP, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("ArapFlow_SetResident", None, [_VP, _I]),
    ("ArapFlow_SetTile", _I, [_VP, _I, _I]),
    ("ArapFlow_SolverResidentLaunches", C.c_uint64, [_VP]),
    ("ArapFlow_PlanResidentLaunches", C.c_uint64, [_VP]),
    ("ArapFlow_LMState", _I, [_VP, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("ArapFlow_SolverLaunchesFor", _I, [_VP, C.c_uint]),
    ("ArapFlow_ResidentDeal", _I, [C.POINTER(C.c_int), C.c_uint, C.POINTER(C.c_int), C.c_uint]),
    ("ArapFlow_ResidentTiles", _I, [_VP, _U, _U, _I, C.POINTER(C.c_int), _U, C.POINTER(C.c_int)]),
    ("ArapFlow_SolverResidentLayout", _I, [_VP, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("ArapFlow_SolverResidentSums", _I, [_VP, C.POINTER(C.c_int), C.c_uint]),
    ("ArapFlow_SolverLeanStream", _I, [_VP]),
    ("ArapFlow_SolverStepRecipe", _I, [_VP, C.POINTER(C.c_int)]),
    ("ArapFlow_ResidentFailed", _I, [_VP]),
    ("ArapFlow_SolverStamps", _I, [_VP, _VP]),
    ("ArapFlow_SolverStampParts", _I, [_VP, _VP]),
    ("ArapFlow_WarpScratchBytes", C.c_uint64, [_U, _U]),
    ("ArapFlow_Warp", _I, [_VP, _U, _U, _VP, _VP, _VP, _VP, _VP, _VP]),
    ("ArapFlow_SolverSetOutputs", _I, [_VP, _I]),
    ("ArapFlow_SolverGetExtraResults", _I, [_VP, _U, _VP, _VP, _VP]),
    ("ArapFlow_SolverHostExtraResults", _I, [_VP, _U, C.POINTER(_VP), C.POINTER(_VP), C.POINTER(_VP)]),
    ("ArapFlow_WarpExScratchBytes", C.c_uint64, [_U, _U]),
    ("ArapFlow_WarpEx", _I, [_VP, _U, _U, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    ("ArapFlow_SolverSetSnapshots", _I, [_VP, C.POINTER(C.c_uint), _U]),
    ("ArapFlow_SolverGetSnapshot", _I, [_VP, _U, _U, _VP, _VP, _VP, _VP]),
    ("ArapFlow_SolverHostSnapshot", _I, [_VP, _U, _U, C.POINTER(_VP), C.POINTER(_VP), C.POINTER(_VP), C.POINTER(_VP)]),
    ("ArapFlow_WarpStep", _I, [_VP, _U, _U, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    ("ArapFlow_WarpLayersScratchBytes", C.c_uint64, [_U, _U, _U]),
    ("ArapFlow_WarpLayers", _I, [_VP, _U, _U, _U, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    ("ArapFlow_WarpLayersStepScratchBytes", C.c_uint64, [_U, _U, _U]),
    ("ArapFlow_WarpLayersStep", _I, [_VP, _U, _U, _U, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    ("ArapFlow_TrackPointsScratchBytes", C.c_uint64, [_U, _U, _U, _U]),
    ("ArapFlow_TrackPoints", _I, [_VP, _U, _U, _U, _VP, _U, _VP, _U, _VP, _VP, _VP, _VP]),
    ("ArapFlow_BackgroundMaps", _I, [C.POINTER(C.c_float)] * 4),
    ("ArapFlow_Background", _I, [_VP, _U, _U, _VP, _U, _U, C.POINTER(C.c_float), C.POINTER(C.c_float)] + [_VP] * 14),
    ("ArapFlow_BackgroundSeq", _I, [_VP, _U, _U, _VP, _U, _U, _U, C.POINTER(C.c_float), _VP] + [C.POINTER(_VP)] * 7),
    ("ArapFlow_Texture", _I, [_VP, _U, _U, _U, _VP, _VP, C.POINTER(TexLayer), _VP]),
    ("ArapFlow_BlurSchedule", _I, [C.c_float, C.c_float, _U] + [C.POINTER(C.c_float)] * 4),
    ("ArapFlow_BlurLayersScratchBytes", C.c_uint64, [_U, _U, _U, _U]),
    ("ArapFlow_BlurLayers", _I, [_VP, _U, _U, _U, _VP, _VP, _VP, _VP, C.c_float, C.c_float, _U, _VP, _U, _U,
                                 C.POINTER(C.c_float), C.POINTER(C.c_float), _VP, _VP, _VP]),
    ("ArapFlow_LightTables", _I, [C.POINTER(LightFrame), _U, _U, C.POINTER(C.c_uint8), C.POINTER(C.c_float)]),
    ("ArapFlow_Relight", _I, [_VP, _U, _U, _VP, _VP, _I, C.POINTER(LightFrame), _VP]),
    ("ArapFlow_SegMapsScratchBytes", C.c_uint64, [_U, _U, _U]),
    ("ArapFlow_SegMaps", _I, [_VP, _U, _U, _U, _VP, _VP, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, _U] + [_VP] * 7),
    ("ArapFlow_FlowScore", _I, [_VP, _U, _U, _U] + [_VP] * 7),
    ("ArapFlow_TrackScore", _I, [_VP, _U, _U] + [_VP] * 4 + [C.c_float, C.c_float, _VP]),
    ("ArapFlow_ChainFlows", _I, [_VP, _U, _U, _U, _VP, _VP, _U, _VP, _VP, _VP]),
    ("ArapFlow_FrameScore", _I, [_VP, _U, _U, _U] + [_VP] * 8),
    ("ArapFlow_MapScoreScratchBytes", C.c_uint64, [_U, _U]),
    ("ArapFlow_LabelScore", _I, [_VP, _U, _U, _U, _U, _U] + [_VP] * 5),
    ("ArapFlow_MapScore", _I, [_VP, _U, _U, _U, _VP, _VP, _VP, _U, C.POINTER(C.c_uint), _U, _VP, _VP, _VP]),
    ("ArapFlow_InterpScratchBytes", C.c_uint64, [_U, _U, _U]),
    ("ArapFlow_InterpFrames", _I, [_VP, _U, _U] + [_VP] * 4 + [_U, C.POINTER(C.c_float)] + [_VP] * 3),
    ("ArapFlow_WarpDiag", _I, [_VP, _U, _U, _VP, _VP, _VP, _VP]),
    ("ArapFlow_SolverSetDiag", _I, [_VP, _I]),
    ("ArapFlow_SolverGetDiag", _I, [_VP, _U, C.POINTER(MeshStats), _VP]),
    ("ArapFlow_SolverHostDiag", _I, [_VP, _U, C.POINTER(C.POINTER(MeshStats)), C.POINTER(_VP)]),
    ("ArapFlow_AugmentTables", _I, [C.POINTER(AugSample)] + [C.POINTER(C.c_float)] * 4),
    ("ArapFlow_AugmentPairs", _I, [_VP, _U, _U, _U, _U, _U] + [_VP] * 4 + [C.POINTER(AugSample)] + [C.POINTER(C.c_float)] * 2 +
     [C.c_float] + [_VP] * 4),
    ("ArapFlow_ClipTables", _I, [C.POINTER(ClipFrame)] + [C.POINTER(C.c_float)] * 4),
    ("ArapFlow_AugmentClips", _I, [_VP] + [_U] * 8 + [_VP, C.POINTER(C.c_int32)] + [_VP] * 4 + [C.POINTER(ClipFrame)] +
     [C.POINTER(C.c_float)] * 2 + [C.c_float] + [_VP] * 5),
]

OUT_BACKWARD, OUT_OCCLUSION = 1, 2      # ARAPFLOW_OUT_* of include/arap_opt.h
MAX_SNAPSHOTS = 8                       # ARAPFLOW_MAX_SNAPSHOTS
MAX_BLUR_SAMPLES, BLUR_CHUNK = 32, 8    # ARAPFLOW_MAX_BLUR_SAMPLES, ARAPFLOW_BLUR_CHUNK
SEG_MAX_RADIUS = 254                    # ARAPFLOW_SEG_MAX_RADIUS
SCORE_ROWS, SCORE_FIELDS = 10, 8         # ARAPFLOW_SCORE_ROWS, ARAPFLOW_SCORE_FIELDS
TSCORE_MAX_FRAMES, TSCORE_CLASSES, TSCORE_FIELDS = 64, 3, 16    # ARAPFLOW_TSCORE_MAX_FRAMES, _CLASSES, _FIELDS
FSCORE_ROWS, FSCORE_FIELDS = 9, 7         # ARAPFLOW_FSCORE_ROWS, ARAPFLOW_FSCORE_FIELDS
LSCORE_FIELDS, MSCORE_MAX_THR = 8, 8      # ARAPFLOW_LSCORE_FIELDS, ARAPFLOW_MSCORE_MAX_THR
INTERP_MAX_TIMES, INTERP_FILL = 32, 16     # ARAPFLOW_INTERP_MAX_TIMES, ARAPFLOW_INTERP_FILL
LIGHT_MAX_R, LIGHT_MAX_SHIFT = 16, 64   # ARAPFLOW_LIGHT_MAX_R, ARAPFLOW_LIGHT_MAX_SHIFT
AUG_MAX_BATCH, AUG_MAX_ERASE = 64, 4    # ARAPFLOW_AUG_MAX_BATCH, ARAPFLOW_AUG_MAX_ERASE
CLIP_MAX_FRAMES, CLIP_MAX_LINKS, CLIP_MAX_UNITS = 16, 32, 256   # ARAPFLOW_CLIP_MAX_FRAMES, ARAPFLOW_CLIP_MAX_LINKS; B * T <= 256

_LIB = None


def load():
    """Load libarapopt.so and type every exported entry point.  Raises if it was not built."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libarapopt.so not built (%s): run `python -m arap_flow_amd.build` or "
                "__graft_entry__.build(); there is no CPU fallback" % LIB_PATH)
        # One HIP runtime per process: libarapopt.so links /opt/rocm's libamdhip64, torch (which owns the device
        # buffers in the tests and the bench) bundles its own copy.  Whichever is loaded first serves both, but if
        # this library came first and torch second, HIP reports no device to this library.  Load torch first.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            fn = getattr(lib, name)     # AttributeError if a declared symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _LIB = lib
    return _LIB
