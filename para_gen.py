#!/usr/bin/env python3
"""para_gen -- Python 3 twin of the reference's dataset generator CLI (para_gen.py:341-653), same flags.

  python para_gen.py --input IN --output OUT --gpu 0 1 .. 7 [--fd k] [--size W H] [--multseg] [--resume]
                     [--bwd_flow] [--occ | --multseg --occ_layers] [--mid K | --multseg --mid_layers K]
                     [--bg_dir DIR [--bg_motion [STRENGTH] [--mid_bg]]] [--diag] [--max_fold FRAC] [--retex]
                     [--bg_dir DIR --blur SHUTTER [SAMPLES]]
                     [--bg_dir DIR --relight [STRENGTH]]
                     [--seg [TAU [RADIUS]]]
                     [--tracks P]
                     [--arap_bin BIN] [--dm_bin BIN | --matches DIR] [--narap N] [--jobs J]

Pipeline per frame pair (para_gen.py:384-567): scan IN/orgRGB/**/N.jpg + IN/orgMasks/**/N.png, pair frame n with
n+fd, resize/crop, match, filter matches into constraints, composite a random background, write the inverted
mask (one, or one per segment with --multseg), hand list-file lines to whichever GPU has room (one worker process
per GPU, HIP_VISIBLE_DEVICES per worker, no collective), flatten segments, composite the background into the
warped frame, write OUT/all_files.list.

What differs from the reference, and why (a GPU solves ~20 of these frames per second; the reference's loop prepares
pairs serially and forks one ARAP child per hand-out, which would leave the GPU idle > 90 % of the time):
  * The front end (resize, match filter, masks, PNG writes) and the back end (flatten, background) run in --jobs worker
    processes; the parent only schedules.  Output files are the same.
  * One persistent ARAP worker per GPU id (`arap_deform --serve`, started before the first pair is prepared) is fed
    list-file lines over a pipe and reports every finished solve; it batches what has accumulated whenever its GPU
    would otherwise idle.  --narap is the most lines a GPU holds at a time (the reference's dead flag, para_gen.py:628,
    put to work): lines go to whichever GPU has room, as the reference's GPU queue does (para_gen.py:441-445,560-567).
    A foreign --arap_bin (argv contract of arap_deform only) is run once per hand-out of up to --narap lines instead.
  * A worker that exits non-zero fails the run at once (the reference hangs: its GPU id never returns to the queue).
  * DeepMatching (para_gen.py:227-240) is an external binary that is not part of the reference tree.  Pass --dm_bin
    PATH (called exactly as the reference does), --dm_bin builtin (this repo's GPU implementation of the published
    algorithm, libarapmatch.so: every pair is matched first, then the ARAP workers start -- the two must not share a
    GPU at the same time) or --matches DIR holding precomputed `x1 y1 x2 y2 ...` lines at DIR/<seq>/<frame>.txt.
  * --bg_dir replaces the hard-coded 'data/naturedata' (para_gen.py:16); without it frames keep a black
    background.
  * --bg_motion (needs --bg_dir) moves the background between the two frames (DESIGN.md "Moving background"): frame 1 is
    composited as before; the warped frame's background, the full-frame flow OUT/FlowFull and, with --occ / --occ_layers
    / --bwd_flow, OUT/OccFull, OUT/FlowBwdFull, OUT/OccBwdFull come from one `bg` line per pair, handed to the pair's
    worker once its solves (and flatten / layers line) are done.
  * --mid_bg (needs --bg_motion and --mid K or --multseg --mid_layers K) moves the camera through the in-between frames
    too (DESIGN.md "Moving background over in-between frames"): the frame after ramp step i gets the camera at the
    fraction i / 19 of the pair's motion, the pair's bg line names the snapshots (mid=), their cameras (mm=) and
    OUT/MidFull/<seq>/<frame> (mid_out=), and one sequence pass of the worker writes there every in-between frame over
    the moving background and every link's full-frame flow (with --mid_layers K --occ_layers: and occlusion).  OUT/Mid
    keeps the object-side files.
  * --diag writes the fold diagnostics of every pair (DESIGN.md "Fold diagnostics"): OUT/Diag/<seq>/<frame>.txt, the mesh
    statistics of the solve, and OUT/Fold/<seq>/<frame>.png, 255 where the frame-1 flow value is no valid correspondence;
    with --multseg the segments' files are merged.  --max_fold FRAC (implies --diag) keeps a pair out of all_files.list
    and all_files_ext.list when a triangle went non-finite or more than FRAC of them folded, and names it in
    OUT/rejected.list instead (`rgb1 rgb2 flow folded triangles nonfinite`); its files stay.  The lists are decided from
    the Diag files on disk (write_lists), so a --resume run writes the same ones.
  * --tracks P (needs --mid K or --multseg --mid_layers K) writes long-range point tracks (DESIGN.md "Point tracks"):
    P query points of frame 1 (pipeline.sample_track_points, from the pair's own generator), their sub-pixel position
    and an occluded flag in frame 1, the K in-between frames and frame 2, as OUT/Tracks/<seq>/<frame>.trk
    (arap_flow_amd/trk.py), from one `trk` line per pair once the states' flow files exist.  The background is taken
    as static, so --bg_motion is refused.
  * --retex writes the random-texture twin of every kept pair (DESIGN.md "Random textures"; the reference's D15OM beside
    its D15RM): OUT/inpRGB_tex/<seq>/<frame>.png, frame 1 with a procedural texture on every object (with --multseg one per
    segment), and OUT/wRGB_tex/<seq>/<frame>.png, its warp with the pair's already solved flows, from one `tex` line per
    pair, handed to a worker once the pair's solves (and layers line) are done and before the segments are merged.  The
    twin costs no solve and shares the pair's Flow file: OUT/all_files_tex.list names `inpRGB_tex wRGB_tex Flow`.  With
    --bg_dir the twin gets the pair's background; with --bg_motion its warped frame goes through a second bg line with the
    same maps.  The textures are drawn from a random.Random seeded with the pair's id, so a rerun reproduces them.
  * --blur SHUTTER [SAMPLES] writes the motion-blurred variant of every kept pair (DESIGN.md "Motion blur"):
    OUT/inpRGB_blur/<seq>/<frame>.png, frame 1 exposed around t = 0, and OUT/wRGB_blur/<seq>/<frame>.png, frame 2 exposed
    around t = 1, each the integer mean of SAMPLES (default 9) renders of the pair's solved mesh over a window of SHUTTER
    (in units of the pair's motion) over the pair's background -- with --bg_motion through the camera of every moment --
    from one `blur` line per pair, handed to a worker once the pair's solves (and layers line) are done and before the
    segments are merged.  It costs no solve and shares the pair's Flow file (the exposure windows are centred on the two
    frame times): OUT/all_files_blur.list names `inpRGB_blur wRGB_blur Flow`.  Needs --bg_dir.
  * --relight [STRENGTH] writes the relit variant of every kept pair (DESIGN.md "Relit frames"):
    OUT/inpRGB_light/<seq>/<frame>.png and OUT/wRGB_light/<seq>/<frame>.png, the pair's two finished frames under a soft
    shadow of the objects on the background, a drifting illumination field, a flickering tone curve, a vignette and sensor
    noise (pipeline.random_light, seeded with the pair's id; every amplitude scaled by STRENGTH, default 1), from one `light`
    line per pair, handed to a worker once both frames are final: after the segments are merged and the background is
    composited, with --bg_motion after the pair's bg line.  The geometry is untouched, so it costs no solve and shares the
    pair's Flow file: OUT/all_files_light.list names `inpRGB_light wRGB_light Flow`.  Needs --bg_dir.
  * --seg [TAU [RADIUS]] writes the segment maps of every kept pair (DESIGN.md "Segment maps"), named like the pair's flow
    file, as 8-bit PNGs: OUT/Index1 and OUT/Index2, the object index of every pixel of frame 1 and of frame 2 (0: no
    object; the solved segment in list order + 1); OUT/MB and OUT/MBBwd, 255 where the full forward / backward flow jumps by
    more than TAU pixels (default 1) against a 4-neighbour; OUT/MBDist and OUT/MBDistBwd, the distance in whole pixels to the
    nearest such pixel up to RADIUS (default 140, at most 254), 255 beyond -- from one `seg` line per pair over its solved
    layers, handed to a worker once the pair's solves (and layers line) are done and before the segments are merged.  With
    --bg_motion the line carries the pair's cameras, so the background's flow counts; without it the background is static.
"""
import argparse
import json
import logging
import os
import os.path as osp
import queue
import random as rn
import re
import subprocess
import sys
import threading
import time
from dataclasses import dataclass
from multiprocessing import Pool
from typing import Callable, NamedTuple

import numpy as np
from PIL import Image

HERE = osp.dirname(osp.abspath(__file__))
sys.path.insert(0, HERE)
from arap_flow_amd import pipeline          # noqa: E402

orgcolor, orgmask = "orgRGB", "orgMasks"                              # para_gen.py:18-26
color_dir, mask_dir, constraints_dir = "inpRGB", "inpMasks", "tmpCnstr"
flow_dir, wrgb_dir, wMask_dir = "Flow", "wRGB", "wMasks"
color_blur_dir, wrgb_blur_dir = "inpRGB_blur", "wRGB_blur"
color_light_dir, wrgb_light_dir = "inpRGB_light", "wRGB_light"
SEG_DIRS = dict(idx1="Index1", idx2="Index2", mb1="MB", mb2="MBBwd", dist1="MBDist", dist2="MBDistBwd")
color_tex_dir, wrgb_tex_dir = "inpRGB_tex", "wRGB_tex"
bwd_dir, occ_bwd_dir, occ_dir = "FlowBwd", "OccBwd", "Occ"
diag_dir, fold_dir = "Diag", "Fold"
mid_dir, mid_full_dir = "Mid", "MidFull"
tracks_dir = "Tracks"
full_dir, occ_full_dir, bwd_full_dir, occ_bwd_full_dir = "FlowFull", "OccFull", "FlowBwdFull", "OccBwdFull"
NUM_ITER = 19                      # the ramp length of the ARAP drivers (main.cpp:215-221): what --mid K spreads over
LAYERS_OCC = "occl_gen"            # --multseg --occ_layers: the frame's forward occlusion, made by a `layers` line
CPP_BIN = osp.join(HERE, "arap_flow_amd", "bin", "arap_deform")


NONE_IS_OFF = ("bg_motion", "relight", "blur", "seg")      # given iff not None (a strength of 0 counts); the others iff truthy


def asked(when, flags):
    """a condition of the tables OUTPUTS, FOREIGN and EXCLUSIVE: a tuple of alternatives, each the "+"-joined flags that
    must all be given"""
    given = lambda n, v: v is not None if n in NONE_IS_OFF else bool(v)
    return any(all(given(n, getattr(flags, n, None)) for n in alt.split("+")) for alt in when)


class Output(NamedTuple):
    """one optional output of a pair beyond the base six: its key in the path table, its directory under OUT, its extension
    ("": the prefix of several files, which requested_outputs spells out) and when it is asked for (`asked`).  `use`, in words:
    "resume" -- --resume skips a pair only if it exists; "ext" -- all_files_ext.list names it; "makes" -- asking for it is a
    reason to write that list; "late" -- its line's builder makes its directory once the pair is kept (the front end makes
    the others before it can drop the pair).  `aux`: (private key, flags -> value) that goes into the path table with it."""
    key: str
    dir: str
    ext: str
    when: tuple
    use: str = "resume ext makes"
    aux: tuple = None


# A pair's variants: name -> (flag, directory of frame 1, of frame 2, use).  Their pictures, rgb1<name>_gen and
# rgb2<name>_gen, come late from the variant's own line and are listed with the pair's OWN flow in all_files_<name>.list.
VARIANTS = dict(blur=("blur", color_blur_dir, wrgb_blur_dir, "resume late"),
                light=("relight", color_light_dir, wrgb_light_dir, "resume late"),
                tex=("retex", color_tex_dir, wrgb_tex_dir, "late"))
# Every optional output, in the order all_files_ext.list names them.  Two asymmetries are INHERITED, not designed, and
# kept as they are: --resume looks for the blur, light and seg files but not for the two --retex files; and
# all_files_ext.list names none of the tex / blur / light / seg files (--tracks names its file there but does not cause
# the list -- it cannot be given without --mid / --mid_layers, which do).
OUTPUTS = (
    Output("bwd_gen", bwd_dir, ".flo", ("bwd_flow",)),
    Output("occbwd_gen", occ_bwd_dir, ".png", ("bwd_flow",)),
    Output("occ_gen", occ_dir, ".png", ("occ",)),
    Output("diag_gen", diag_dir, ".txt", ("diag",)),
    Output("fold_gen", fold_dir, ".png", ("diag",)),
    Output(LAYERS_OCC, occ_dir, ".png", ("occ_layers",)),
    Output("flowfull_gen", full_dir, ".flo", ("bg_motion",)),        # --bg_motion: the full-frame maps of what the run asks for
    Output("occfull_gen", occ_full_dir, ".png", ("bg_motion+occ", "bg_motion+occ_layers")),
    Output("bwdfull_gen", bwd_full_dir, ".flo", ("bg_motion+bwd_flow",)),
    Output("occbwdfull_gen", occ_bwd_full_dir, ".png", ("bg_motion+bwd_flow",)),
    Output("mid_gen", mid_dir, "", ("mid",), aux=("_mid", lambda flags: tuple(flags.mid_steps))),
    Output("midl_gen", mid_dir, "", ("mid_layers",), aux=("_midl", lambda flags: tuple(flags.mid_layers_steps))),
    Output("midbg_gen", mid_full_dir, "", ("mid_bg",), "resume ext makes late",
           aux=("_midbg", lambda flags: tuple(flags.mid_steps or flags.mid_layers_steps))),
    Output("trk_gen", tracks_dir, ".trk", ("tracks",), "resume ext late", aux=("_tracks", lambda flags: int(flags.tracks))),
) + tuple(Output("rgb%d%s_gen" % (n, v), d, ".png", (flag,), use)
          for v, (flag, *dirs, use) in VARIANTS.items() for n, d in enumerate(dirs, 1)
          ) + tuple(Output(k + "_seg_gen", d, ".png", ("seg",), "resume late") for k, d in SEG_DIRS.items())
LATE = {o.key for o in OUTPUTS if "late" in o.use}


def mid_paths(p, key="mid_gen", steps="_mid"):
    """--mid: every in-between file of a pair's path table, step by step (flow, frame, mask, step flow); [] without"""
    if key not in p:
        return []
    return [pipeline.mid_files(p[key], i)[k] for i in p[steps] for k in ("flow", "rgb", "mask", "step")]


def mid_layer_paths(p):
    """--mid_layers: every layered in-between file of a pair's path table: per step mid_files' four, then -- with
    --occ_layers -- the link occlusions of pipeline.mid_layer_files, step 0 first; [] without"""
    out = mid_paths(p, "midl_gen", "_midl")
    if out and LAYERS_OCC in p:
        out += [pipeline.mid_layer_files(p["midl_gen"], i)["occ"] for i in (0,) + tuple(p["_midl"])]
    return out


def mid_bg_paths(p):
    """--mid_bg: every file of a pair's bg line's mid_out= token (pipeline.bg_outputs' order: the in-between frames, the
    link flows from frame 1's on, then -- with --occ_layers -- the link occlusions); [] without"""
    if "midbg_gen" not in p:
        return []
    steps, files = tuple(p["_midbg"]), lambda i: pipeline.mid_bg_files(p["midbg_gen"], i)
    out = [files(i)["rgb"] for i in steps] + [files(i)["step"] for i in (0,) + steps]
    return out + ([files(i)["occ"] for i in (0,) + steps] if LAYERS_OCC in p else [])


def requested_outputs(p, use):
    """every optional output a pair's path table asks for, in OUTPUTS' order, that counts for `use`: "resume" (what
    --resume looks for beside the flow file) or "ext" (what all_files_ext.list names after the pair's trio)"""
    prefix_files = dict(mid_gen=mid_paths, midl_gen=mid_layer_paths, midbg_gen=mid_bg_paths)
    out = []
    for o in OUTPUTS:
        if o.key in p and use in o.use.split():
            out += prefix_files[o.key](p) if o.ext == "" else [p[o.key]]
    return out


def _pair_id(seq, stem):
    """a number per frame pair that is the same in every process and every run (str hashes are salted per process)"""
    import zlib
    return zlib.crc32(("%s/%s" % (seq, stem)).encode())


def run_matching(flags, p, seq, stem):
    """para_gen.py:227-240, or precomputed matches"""
    for k in ("rgb1_org", "rgb2_org", "msk1_org", "msk2_org"):
        assert osp.exists(p[k]), "File not found: \n%s" % p[k]
    if flags.matches is not None:
        src = osp.join(flags.matches, seq, stem + ".txt")
        assert osp.exists(src), "File not found: \n%s" % src
        open(p["cstr_tmp"], "w").write(open(src).read())
        return
    if flags.dm_bin == "builtin":
        # this repo's matcher (libarapmatch.so, include/arap_match.h) through the matcher server of one of the GPUs: same
        # inputs, same -ngh_rad, same output file format as the binary below
        from arap_flow_amd import match_server
        socks = flags.dm_sockets
        match_server.request(socks[_pair_id(seq, stem) % len(socks)], p["rgb1_org"], p["rgb2_org"], p["cstr_tmp"], 100)
        return
    cmd = "./%s %s %s -nt 0 -out %s -ngh_rad 100 " % (flags.dm_bin, p["rgb1_org"], p["rgb2_org"], p["cstr_tmp"])
    status = subprocess.call(cmd, shell=True)
    assert status == 0, "Deep matching exited with code %d. The command is \n%s" % (status, cmd)


def has_mask(m1, m2):
    """para_gen.py:243-251"""
    try:
        a, b = np.array(Image.open(m1)), np.array(Image.open(m2))
    except Exception:
        return False
    return a.sum() > 10 and b.sum() > 10


def preprocess(p, size):
    """para_gen.py:294-310"""
    out = []
    for n in ("1", "2"):
        pre, im, mk = pipeline.scale_rotate(p["rgb%s_org" % n], p["msk%s_org" % n], size)
        if pre:
            im.save(p["rgb%s_gen" % n])
            mk.save(p["msk%s_gen" % n])
            p["rgb%s_org" % n], p["msk%s_org" % n] = p["rgb%s_gen" % n], p["msk%s_gen" % n]
        out += [np.array(im.convert("RGB")), np.array(mk)]
    return out


def cleanup(p):
    """para_gen.py:311-316"""
    for k in p:
        if "_org" not in k and osp.exists(p[k]):
            logging.warning("Removing\n\t%s", p[k])
            os.remove(p[k])


# ----------------------------------------------------------------------------------------------------------------
# front end / back end of one frame pair: run in the --jobs pool
# ----------------------------------------------------------------------------------------------------------------
class Step(NamedTuple):
    """one list line of a pair's plan: the line (a pipeline *Line), the key of main's `counts` it bumps when a worker
    reports it done, and the files that go when its stage is done (kept with --keep_segments)"""
    line: object
    count: str
    remove: tuple = ()


FINISH = "finish_frame"            # the one stage of a plan that is no list of Steps: finish_frame, run in the pool


@dataclass
class Frame:
    """one frame pair on its way from prepare_pair through main to finish_frame"""
    line: pipeline.SolveLine       # the pair's list line; its outputs are the frame's outputs
    segs: list                     # --multseg: the per-segment lines that are solved in its place, else None
    layers: object                 # --occ_layers / --mid_layers: the frame's layers line (pipeline.LayersLine), else None
    bg: object                     # the still background fitted to the frame (an array), or None (--bg_motion: the bg line's)
    remove: bool                   # delete the segments' files once they are merged, and every Step's own files
    plan: list                     # the stages still to do: FINISH, or a list of Steps that may be in flight together
    left: int = 0                  # main: Steps of the current stage not yet reported done
    also_bg: tuple = ()            # further warped frames that finish_frame puts the still background behind (the twin's)

    @property
    def solves(self):
        return [self.line] if self.segs is None else self.segs


def follow_up_steps(plan):
    """every Step of a plan after its first stage: the lines main owes the workers when it hands out the solves"""
    return [st for stage in plan[1:] if stage != FINISH for st in stage]


class Pair(NamedTuple):
    """what front_end leaves to the builders of a pair's follow-up lines"""
    rec: Frame                     # the pair's Frame, its plan not yet written: line, segs, solves and the still background
    id: int                        # _pair_id
    p: dict                        # the path table without its private and late entries ...
    own: dict                      # ... and those entries
    stack: list                    # the solved layers as the layered lines name them: (mask, flow), the later on top
    masks: list                    # frame 1's mask(s) as written: one, or one per segment
    wh: tuple                      # (W, H)
    big: object                    # --bg_motion: the enlarged background (an array), else None
    mids: tuple                    # --bg_motion: the in-between frames' maps of pipeline.bg_maps_seq
    m: tuple                       # --bg_motion: M1 then M2 as a line's m= token takes them, else ()

    def rng(self):              # a FRESH generator: the bg window, the textures, the track points and the light each start one
        return rn.Random(self.id)

    def tmp(self, suffix):      # a file of the lines' own inputs, beside the pair's constraints
        return osp.splitext(self.p["cstr_tmp"])[0] + suffix

    def union_mask(self, suffix):
        """the union of the segments' masks (object where any solved segment is object) as a PNG -> its path"""
        Image.fromarray(np.minimum.reduce(self.masks)).save(self.tmp(suffix))
        return self.tmp(suffix)


def _make_dirs(paths):
    for q in paths:
        os.makedirs(osp.dirname(q), exist_ok=True)


def front_end(flags, p, bgpath, seq, stem, own):
    """para_gen.py:447-540 for one pair, up to "frame 1 and its mask(s) are written": preprocess, match, filter, background,
    masks.  Returns None when the pair is dropped (no mask, no valid constraint), else its Pair."""
    line, midl, midbg = pipeline.make_arap_path(dict(p, **own)), own.get("_midl"), own.get("_midbg")
    _make_dirs(p.values())
    im1, mk1, im2, mk2 = preprocess(p, flags.size)
    if not has_mask(p["msk1_org"], p["msk2_org"]):
        cleanup(p)
        return None
    run_matching(flags, p, seq, stem)
    cstr_lines = open(p["cstr_tmp"]).read().splitlines()
    cstrs, valids = pipeline.filter_matches(cstr_lines, mk1, mk2)
    pipeline.write_constraints(p["cstr_tmp"], cstrs)
    if len(cstrs) == 0:
        cleanup(p)
        return None
    bgim = None
    if bgpath is not None:
        try:
            bgim = np.array(Image.open(bgpath))
            if not (bgim.ndim == 3 and bgim.shape[2] == 3):
                bgim = None
        except Exception:
            bgim = None
    H, W = im1.shape[:2]
    big, mids, m = None, (), ()
    if bgim is not None and getattr(flags, "bg_motion", None) is not None:
        rng = rn.Random(_pair_id(seq, stem))
        big, (left, top) = pipeline.fit_bg_window(bgim, im1, rng=rng)          # the window and frame 1 of a run without
        # camera and objects move in step: after ramp step i every handle has covered i / NUM_ITER of its displacement
        M1, mids, M2 = pipeline.bg_maps_seq(left, top, (W, H), (big.shape[1], big.shape[0]), rng,
                                            [i / float(NUM_ITER) for i in midbg or ()], flags.fd, flags.bg_motion)
        m = tuple(float(v) for v in np.concatenate([M1, M2]))
        out1 = pipeline.add_bg(im1, mk1, big[top:top + H, left:left + W, :])
        bgim = None
    elif bgim is not None:
        bgim = pipeline.fit_bg(bgim, im1, rng=rn.Random(_pair_id(seq, stem)))
        out1 = pipeline.add_bg(im1, mk1, bgim)
    else:
        out1 = im1
    Image.fromarray(out1).save(p["rgb1_gen"])
    segs, masks = None, []
    if not flags.multseg:
        mask = np.zeros_like(mk1, dtype=np.uint8)
        mask[mk1 == 0] = pipeline.ARAP_BG                                      # :514-517
        Image.fromarray(mask).save(p["msk1_gen"])
        masks.append(mask)
    else:
        segs = []
        for s, mask in pipeline.split_segments(mk1, valids):                   # :518-540 (a kept constraint has a label > 0:
            p_ = pipeline.replace_ext(p, s, keep_orgs=["rgb1_gen", "cstr_tmp"])        # there is at least one segment)
            Image.fromarray(mask).save(p_["msk1_gen"])
            masks.append(mask)
            segs.append(pipeline.make_arap_path(p_))
            if midl:                            # the segment's snapshots lie beside its flow: <flow without .flo>_sII*
                segs[-1].extra["mid"] = pipeline.mid_token(midl, segs[-1].flow[:-len(".flo")])
    rec = Frame(line, segs, None, bgim, not getattr(flags, "keep_segments", False), plan=[])
    return Pair(rec, _pair_id(seq, stem), p, own, [(sg.mask, sg.flow) for sg in rec.solves], masks, (W, H), big, mids, m)


# -- the builders of a pair's follow-up lines: (the Pair, the flags) -> the line's Step -- the line, its counter, its own
#    temporary files -- or None when the run or the pair has no such line
def layers_step(pr, flags):
    """--occ_layers / --mid_layers: the frame's layers line, segments in list order (ascending label, later on top)"""
    midl = pr.own.get("_midl")
    if not pr.rec.segs or not (LAYERS_OCC in pr.p or midl):
        return None
    out = dict(occ=pr.p[LAYERS_OCC]) if LAYERS_OCC in pr.p else {}
    if midl:
        out["mid"] = pipeline.mid_token(midl, pr.p["midl_gen"])
    return Step(pipeline.LayersLine(pr.rec.line.rgb, pr.stack, out), "layers_done")


def track_step(pr, flags):
    """--tracks: the points from the pair's own generator, every state file of every layer named"""
    if "trk_gen" not in pr.own:
        return None
    from arap_flow_amd import trk
    _make_dirs([pr.own["trk_gen"]])
    (W, H), pts = pr.wh, pr.tmp("_pts.trk")
    trk.write(pts, W, H, pipeline.sample_track_points(pr.rng(), pr.own["_tracks"], W, H, np.stack(pr.masks)))
    steps = pr.own.get("_midl") or pipeline.parse_mid(pr.rec.line.extra["mid"])[0]
    states = lambda sg: tuple(pipeline.mid_files(pipeline.parse_mid(sg.extra["mid"])[1], i)["flow"] for i in steps) + (sg.flow,)
    return Step(pipeline.TrkLine(pts, [(sg.mask, states(sg)) for sg in pr.rec.solves], pr.own["trk_gen"]), "tracks_done", (pts,))


def _two_frames(pr, name, needs_bg=False):
    """a variant's two pictures (VARIANTS) as its line's `out`, their directories made; None without the variant, or its bg"""
    if "rgb1%s_gen" % name not in pr.own or (needs_bg and pr.rec.bg is None and pr.big is None):
        return None
    out = dict(rgb1=pr.own["rgb1%s_gen" % name], rgb2=pr.own["rgb2%s_gen" % name])
    _make_dirs(out.values())
    return out


def tex_step(pr, flags):
    """--retex: the twin, one texture per solved layer, from the pair's own generator"""
    out = _two_frames(pr, "tex")
    tex = out and tuple(pipeline.tex_layers(pr.rng(), len(pr.stack), pr.wh))
    return out and Step(pipeline.TexLine(pr.rec.line.rgb, pr.stack, tex, out), "tex_done")


def blur_step(pr, flags):
    """--blur: the solved layers over the pair's background.  A still background is the fitted picture, written beside the
    pair's constraints and seen through the identity; a moving one is the bg line's picture and maps (bg_steps)"""
    out = _two_frames(pr, "blur", needs_bg=True)
    if out is None:
        return None
    bg_png = pr.tmp("_blurbg.png" if pr.big is None else "_bg.png")
    if pr.big is None:
        Image.fromarray(pr.rec.bg).save(bg_png)
    return Step(pipeline.BlurLine(pr.rec.line.rgb, pr.stack, bg_png, *flags.blur, pr.m, out), "blur_done",
                (bg_png,) if pr.big is None else ())


def seg_step(pr, flags):
    """--seg: the segment maps over the solved layers, with the bg line's cameras where there is one"""
    out = {k: pr.own[k + "_seg_gen"] for k in SEG_DIRS if k + "_seg_gen" in pr.own}
    _make_dirs(out.values())
    return Step(pipeline.SegLine(pr.stack, *flags.seg, pr.m, out), "seg_done") if out else None


def bg_steps(pr, flags, tex):
    """--bg_motion: the pair's bg line, whose Step removes the line's own inputs, beside the pair's constraints: the enlarged
    picture as a PNG (the worker's codec), with --multseg the union mask, and the line itself as text; after it, with
    --retex, the twin's warped frame over the same moving background, a second bg line (frame 1 has it)"""
    if pr.big is None:
        return []
    p, line, bg_png, midbg = pr.p, pr.rec.line, pr.tmp("_bg.png"), pr.own.get("_midbg")
    Image.fromarray(pr.big).save(bg_png)
    mask1 = line.mask if pr.rec.segs is None else pr.union_mask("_bgmask.png")
    occ_in = p.get("occ_gen", p.get(LAYERS_OCC))
    inputs = {k: v for k, v in dict(occ=occ_in, bwd=p.get("bwd_gen"), occ_bwd=p.get("occbwd_gen")).items() if v}
    outs = {k + "_out": p[g] for k, g in dict(occ="occfull_gen", bwd="bwdfull_gen", occ_bwd="occbwdfull_gen").items()
            if k in inputs and g in p}
    tokens = {}
    if midbg:                                   # the snapshots' files exist when the line is handed out: after the solve / layers line
        _make_dirs([pr.own["midbg_gen"]])
        tokens = dict(mid=pipeline.mid_token(midbg, p.get("mid_gen", p.get("midl_gen"))),
                      mm=tuple(float(v) for v in np.concatenate(pr.mids)), mid_out=pr.own["midbg_gen"])
    bg = pipeline.BgLine(bg_png, line.rgb, mask1, line.out_rgb, line.out_mask, line.flow, m=pr.m, inputs=inputs,
                         out=("", line.out_rgb, p["flowfull_gen"]), outs=outs, **tokens)
    open(pr.tmp("_bg.txt"), "w").write(pipeline.format_line(bg))
    steps = [Step(bg, "bg_done", (bg_png,) + ((mask1,) if pr.rec.segs is not None else ()) + (pr.tmp("_bg.txt"),))]
    if tex:
        rgb1, rgb2 = tex.line.out["rgb1"], tex.line.out["rgb2"]
        steps.append(Step(bg._replace(rgb1=rgb1, rgb2=rgb2, inputs={}, out=("", rgb2, ""), outs={}, mid="", mm=(), mid_out=""),
                          "tex_done"))
    return steps


def light_step(pr, flags, bg):
    """--relight: the two finished frames, frame 1's object mask -- with --multseg the union of the segments', the bg line's
    where there is one -- and the merged warped mask as frame 2's cover; the light from the pair's own generator"""
    out = _two_frames(pr, "light", needs_bg=True)
    if out is None:
        return None
    line = pr.rec.line
    mine = (pr.union_mask("_lightmask.png"),) if pr.rec.segs is not None and not bg else ()
    mask1 = line.mask if pr.rec.segs is None else bg[0].line.mask1 if bg else mine[0]
    light = pipeline.random_light(pr.rng(), flags.relight, *pr.wh)
    return Step(pipeline.LightLine(line.rgb, mask1, line.out_rgb, line.out_mask, light, out), "light_done", mine)


def prepare_pair(args):
    """para_gen.py:447-556 for one pair: everything up to its list-file line(s).  Returns None when the pair is dropped (no
    mask, no valid constraint), else its Frame, whose plan says what is handed out when:
      1. every solve;  2. the layers line and the trk line, together;  3. the tex / blur / seg line -- they read the
      segments' files, so they come before  4. FINISH, which merges and removes them;  5. the pair's bg line;  6. the twin's
      bg line, or the light line (without --bg_motion right after FINISH)."""
    flags, p, bgpath = args
    p = dict(p)
    seq, stem = p.pop("_seq"), p.pop("_stem")
    pr = front_end(flags, p, bgpath, seq, stem, {k: p.pop(k) for k in list(p) if k.startswith("_") or k in LATE})
    if pr is None:
        return None
    some = lambda *steps: [st for st in steps if st is not None]
    merge, tex = layers_step(pr, flags), tex_step(pr, flags)
    bg = bg_steps(pr, flags, tex)
    finals = bg + some(light_step(pr, flags, bg))
    if len(finals) > 1:         # (only after a bg line) the bg line's own inputs go with the pair's LAST line that reads them
        finals[0], finals[-1] = bg[0]._replace(remove=()), finals[-1]._replace(remove=bg[0].remove + finals[-1].remove)
    plan = [[Step(ln, "solves_done") for ln in pr.rec.solves], some(merge, track_step(pr, flags)),
            some(tex, blur_step(pr, flags), seg_step(pr, flags)), FINISH] + [[st] for st in finals]
    pr.rec.layers, pr.rec.also_bg = merge and merge.line, (tex.line.out["rgb2"],) if tex else ()
    pr.rec.plan = [stage for stage in plan if stage]
    return pr.rec


def finish_frame(rec):
    """para_gen.py:202-212 for one Frame whose solve(s) are done: flatten the segments, composite the still background (a
    --bg_motion pair's comes from its bg line afterwards)"""
    merged = pipeline.parse_mid(rec.layers.out["mid"]) if rec.layers is not None and "mid" in rec.layers.out else None
    if merged and rec.remove:                               # --mid_layers: the segments' snapshot files have been merged
        for q in (q for sg in rec.segs for i in merged[0] for q in pipeline.mid_files(sg.flow[:-len(".flo")], i).values()):
            if osp.exists(q):
                os.remove(q)
    if rec.segs is not None:
        if "diag" in rec.line.extra:                        # (before flatten_backward removes the segments' extra files)
            pipeline.flatten_diag(rec.line, rec.segs, remove=rec.remove)
        if {"bwd", "occ_bwd"} & set(rec.line.extra):        # (before flatten removes the segments' warped masks)
            pipeline.flatten_backward(rec.line, rec.segs, remove=rec.remove)
        pipeline.flatten([(rec.line, rec.segs)], remove=rec.remove)
    if rec.bg is not None:      # behind the warped frame, the twin's (the same mask) and every in-between frame
        own = pipeline.parse_mid(rec.line.extra["mid"]) if "mid" in rec.line.extra else None       # --mid
        behind = [(q, rec.line.out_mask) for q in (rec.line.out_rgb,) + rec.also_bg]
        behind += [(f["rgb"], f["mask"]) for mid in (merged, own) if mid for f in (pipeline.mid_files(mid[1], i) for i in mid[0])]
        for rgb, mask in behind:
            im, m = np.array(Image.open(rgb).convert("RGB")), np.array(Image.open(mask))
            Image.fromarray(pipeline.add_bg(im, m, rec.bg)).save(rgb)


# ----------------------------------------------------------------------------------------------------------------
# GPU side: one worker per GPU id, lines to whichever has room
# ----------------------------------------------------------------------------------------------------------------
class GpuWorkers:
    """The reference's GPU queue (para_gen.py:441-445,560-567) at line granularity.  `serve`: one persistent
    `arap_bin --serve` child per GPU; `batch`: one `arap_bin listfile` child per hand-out of up to `narap` lines."""

    def __init__(self, arap_bin, gpus, narap, serve, on_done):
        self.cmd, self.narap, self.serve, self.on_done = arap_bin.split(), max(1, int(narap)), serve, on_done
        self.lines = queue.Queue()
        self.error = None
        self.batches = []                      # solves per GPU launch (serve) / per child (batch)
        self.threads, self.procs = [], []
        self.t_ready = None
        self.owed, self.closing, self.owe_lock = 0, False, threading.Lock()
        for g in gpus:
            t = threading.Thread(target=self._serve_loop if serve else self._batch_loop, args=(g,), daemon=True)
            t.start()
            self.threads.append(t)

    def put(self, line):
        self.lines.put(line)

    def owe(self):
        """a line will be put later, from a reader thread (a frame's layers line, once its last solve is done): the
        workers stay open for it"""
        with self.owe_lock:
            self.owed += 1

    def put_owed(self, line):
        with self.owe_lock:
            self.lines.put(line)
            self.owed -= 1
            if self.closing and self.owed == 0:
                self._post_end()

    def close(self):
        """no further line from the caller: end markers now, or behind the last owed line"""
        with self.owe_lock:
            self.closing = True
            if self.owed == 0:
                self._post_end()

    def _post_end(self):
        for _ in self.threads:
            self.lines.put(None)

    def join(self):
        for t in self.threads:
            while t.is_alive():
                t.join(0.2)
                self.check()
        self.check()

    def check(self):
        if self.error is not None:
            for p in self.procs:
                if p.poll() is None:
                    p.kill()
            raise AssertionError(self.error)

    def _fail(self, msg):
        if self.error is None:
            self.error = msg

    def _env(self, gpu):
        return dict(os.environ, HIP_VISIBLE_DEVICES=str(gpu))                  # reference: CUDA_VISIBLE_DEVICES (:190)

    # -- persistent worker -----------------------------------------------------------------------------------
    def _serve_loop(self, gpu):
        try:
            proc = subprocess.Popen(self.cmd + ["--serve"], env=self._env(gpu), stdin=subprocess.PIPE,
                                    stdout=subprocess.PIPE, text=True, bufsize=1)
        except OSError as e:
            self._fail("cannot start %s: %s" % (" ".join(self.cmd), e))
            return
        self.procs.append(proc)
        room = threading.Semaphore(self.narap)
        outstanding = [0]
        lock = threading.Lock()

        def reader():
            for ln in proc.stdout:
                ln = ln.rstrip("\n")
                if ln.startswith("Done "):
                    with lock:
                        outstanding[0] -= 1
                    room.release()
                    self.on_done(ln[5:])
                elif ln.startswith("Batch "):
                    self.batches.append(int(ln[6:]))
                elif ln == "Ready":
                    if self.t_ready is None:
                        self.t_ready = time.time()
                elif ln and ln != "Saved":
                    print(ln)
            rc = proc.wait()
            with lock:
                left = outstanding[0]
            if rc != 0 or left != 0:
                self._fail("ARAP worker on GPU %d exited with code %d, %d solves unfinished. The command was \n%s"
                           % (gpu, rc, left, " ".join(self.cmd + ["--serve"])))
            room.release()                                                      # never leave the feeder blocked

        rt = threading.Thread(target=reader, daemon=True)
        rt.start()
        while self.error is None:
            room.acquire()                                                      # a free place on this GPU first ...
            if proc.poll() is not None:
                break
            line = self.lines.get()                                             # ... then the next line, whoever it is
            if line is None:
                break
            with lock:
                outstanding[0] += 1
            try:
                proc.stdin.write(line + "\n")
                proc.stdin.flush()
            except (BrokenPipeError, OSError):
                self._fail("ARAP worker on GPU %d closed its input" % gpu)
                break
        try:
            proc.stdin.close()
        except OSError:
            pass
        rt.join()

    # -- one child per hand-out (any executable with arap_deform's argv contract) -------------------------------
    def _batch_loop(self, gpu):
        os.makedirs("tmp", exist_ok=True)
        while self.error is None:
            line = self.lines.get()
            if line is None:
                return
            batch, last = [line], False
            while len(batch) < self.narap:
                try:
                    nxt = self.lines.get(timeout=0.05)
                except queue.Empty:
                    break
                if nxt is None:
                    last = True
                    break
                batch.append(nxt)
            fn = osp.abspath("tmp/gpu-%d_%s.txt" % (gpu, str(time.time()).replace(".", "_")))
            print("GPU ", gpu, " ", len(batch), " files")
            try:
                open(fn, "w").write("\n".join(batch))
                status = subprocess.call(self.cmd + [fn], env=self._env(gpu))
            except OSError as e:
                status = "not started (%s)" % e
            finally:
                if osp.exists(fn):
                    os.remove(fn)
            if status != 0:
                self._fail("ARAP exited with code %s. The command was \n%s" % (status, " ".join(self.cmd + [fn])))
                return
            self.batches.append(len(batch))
            for ln in batch:
                self.on_done(pipeline.done_token(pipeline.parse_line(ln)))
            if last:
                return


def scan(flags, input_root, output_root):
    """para_gen.py:384-432: the path table of every pair to do -- the base six, the four inputs, the OUTPUTS the flags ask
    for and the private entries `_seq`, `_stem` and those that go with an output (Output.aux)"""
    rgb_org, msk_org = osp.join(input_root, orgcolor), osp.join(input_root, orgmask)
    base = dict(rgb1_gen=(color_dir, ".png"), msk1_gen=(mask_dir, ".png"), rgb2_gen=(wrgb_dir, ".png"),
                msk2_gen=(wMask_dir, ".png"), cstr_tmp=(constraints_dir, ".txt"), flow_gen=(flow_dir, ".flo"))
    wanted = [o for o in OUTPUTS if asked(o.when, flags)]
    reg = re.compile(r"(\d+)\.(jp.?g|png)$", flags=re.IGNORECASE)
    all_paths = []
    for root, dirs, _ in os.walk(rgb_org):
        for d in sorted(dirs):
            files = sorted(f for f in os.listdir(osp.join(root, d)) if reg.search(f) is not None)
            for f1 in files:
                seq = osp.join(root.replace(rgb_org, "").strip(osp.sep), d)
                f, ext = osp.splitext(f1)
                if not osp.exists(osp.join(msk_org, seq, f + ".png")):
                    continue
                num = reg.search(f1)
                n = "{:0" + str(len(num.group(1))) + "d}"
                f2 = f.replace(num.group(1), n.format(int(num.group(1)) + flags.fd))
                if not osp.exists(osp.join(rgb_org, seq, f2 + ext)) or not osp.exists(osp.join(msk_org, seq, f2 + ".png")):
                    continue
                e = {k: osp.join(output_root, d_, seq, f + x) for k, (d_, x) in base.items()}
                e.update(rgb1_org=osp.join(rgb_org, seq, f1), msk1_org=osp.join(msk_org, seq, f + ".png"),
                         rgb2_org=osp.join(rgb_org, seq, f2 + ext), msk2_org=osp.join(msk_org, seq, f2 + ".png"))
                e.update({o.key: osp.join(output_root, o.dir, seq, f + o.ext) for o in wanted})
                e = {k: osp.abspath(v) for k, v in e.items()}
                e["_seq"], e["_stem"] = seq, f
                e.update({o.aux[0]: o.aux[1](flags) for o in wanted if o.aux})
                done = [e["flow_gen"]] + requested_outputs(e, "resume")
                if not flags.resume or not all(osp.exists(q) for q in done):      # --resume (:431)
                    all_paths.append(e)
    return all_paths


def start_matchers(flags, output_root):
    """one matcher server per --gpu id (arap_flow_amd/match_server.py); their socket paths go to the pool jobs in flags"""
    import tempfile
    d = tempfile.mkdtemp(prefix="arapmatch_")
    procs, socks = [], []
    for g in flags.gpu:
        sock = osp.join(d, "gpu%d.sock" % g)
        env = dict(os.environ, HIP_VISIBLE_DEVICES=str(g))
        pr = subprocess.Popen([sys.executable, "-m", "arap_flow_amd.match_server", sock], cwd=HERE, env=env,
                              stdout=subprocess.PIPE, text=True)
        line = pr.stdout.readline()
        assert line.strip() == "Ready", "matcher server on GPU %d did not start" % g
        procs.append(pr)
        socks.append(sock)
    flags.dm_sockets = socks
    return procs


def stop_matchers(flags, procs):
    from arap_flow_amd import match_server
    for sock in getattr(flags, "dm_sockets", []):
        match_server.stop(sock)
    for pr in procs:
        try:
            pr.wait(timeout=20)
        except subprocess.TimeoutExpired:
            pr.kill()


def write_lists(flags, output_root, all_paths):
    """para_gen.py:588-603 and the additions' own list, from what is on disk: OUT/all_files.list (`rgb1 rgb2 flow` of every
    pair whose three files exist) and, when the run asks for any optional output, OUT/all_files_ext.list (the same plus
    every optional file, for the pairs that have them all).  With --max_fold a pair whose Diag file says
    pipeline.pair_rejected goes to neither but to OUT/rejected.list as `rgb1 rgb2 flow folded triangles nonfinite`.
    `all_paths`: scan's path tables.  Returns (the lines of all_files.list, those of rejected.list)."""
    max_fold = getattr(flags, "max_fold", None)
    out_paths, ext, rejected, listed = [], [], [], []
    for p in all_paths:
        ln = pipeline.make_arap_path(p)
        trio = [ln.rgb, ln.out_rgb, ln.flow]
        full = trio + requested_outputs(p, "ext")
        if not all(osp.exists(q) for q in trio):
            continue
        if max_fold is not None and osp.exists(p.get("diag_gen", "")):
            st = pipeline.parse_diag(open(p["diag_gen"]).read())
            if pipeline.pair_rejected(st, max_fold):
                rejected.append(" ".join(trio + ["%d" % st[k] for k in ("folded", "triangles", "nonfinite")]))
                continue
        out_paths.append(" ".join(trio))
        listed.append(p)
        if all(osp.exists(q) for q in full):
            ext.append(" ".join(full))
    open(osp.join(output_root, "all_files.list"), "w").write("\n".join(out_paths))
    # all_files.list stays as it is; the extra outputs get their own list
    if any("makes" in o.use and asked(o.when, flags) for o in OUTPUTS):
        open(osp.join(output_root, "all_files_ext.list"), "w").write("\n".join(ext))
    if max_fold is not None:
        open(osp.join(output_root, "rejected.list"), "w").write("\n".join(rejected))
    for name, (flag, *_) in VARIANTS.items():              # the variants of the listed pairs: their own frames, the SAME flow
        if asked((flag,), flags):
            trios = [[p["rgb1%s_gen" % name], p["rgb2%s_gen" % name], p["flow_gen"]] for p in listed]
            open(osp.join(output_root, "all_files_%s.list" % name), "w").write(
                "\n".join(" ".join(t) for t in trios if all(osp.exists(q) for q in t)))
    return out_paths, rejected


def main(flags):
    t_start = time.time()
    input_root, output_root = flags.input.rstrip(osp.sep), flags.output.rstrip(osp.sep)
    bg_paths = []
    if flags.bg_dir:
        for root, _, files in os.walk(flags.bg_dir):
            bg_paths += [osp.join(root, f) for f in files if f.upper().endswith((".PNG", ".JPG", ".JPEG"))]
    if getattr(flags, "bg_motion", None) is not None and not bg_paths:
        raise AssertionError("--bg_motion: no background picture (.png, .jpg) under %s" % flags.bg_dir)
    all_paths = scan(flags, input_root, output_root)
    print("Scanning data to be processed\t\t%d files [Done]" % len(all_paths))
    os.makedirs(output_root, exist_ok=True)

    # backgrounds: drawn without replacement until the list is used up, then refilled (para_gen.py:484-499)
    tmp_paths, picks = [], []
    for _ in all_paths:
        if not bg_paths:
            picks.append(None)
            continue
        if not tmp_paths:
            tmp_paths = sorted(bg_paths[:])
        bgpath = rn.choice(tmp_paths)
        tmp_paths.remove(bgpath)
        picks.append(bgpath)

    serve = serves(flags)
    pool = Pool(processes=max(1, flags.jobs))          # (forked before any thread exists)
    frames = {}                                        # done token of a line a worker holds -> (its Frame, its Step)
    posts, lock = [], threading.RLock()
    counts = dict(solves_done=0, frames_done=0, layers_done=0, bg_done=0, tex_done=0, tracks_done=0, blur_done=0,
                  light_done=0, seg_done=0)

    # The scheduler: a Frame's plan, stage by stage.  It knows stages and Steps, no variant -- prepare_pair wrote the plan.
    def start(rec, put):                               # (under `lock`) begin the plan's first stage; none left: the pair is done
        if rec.plan and rec.plan[0] == FINISH:         # frames_done counts the hand-over to the pool, not its return
            counts["frames_done"] += 1
            posts.append(pool.apply_async(finish_frame, (rec,), callback=lambda _: advance(rec),
                                          error_callback=lambda e: workers._fail("finish_frame failed: %r" % (e,))))
        elif rec.plan:
            rec.left = len(rec.plan[0])
            for st in rec.plan[0]:                     # the one place a line becomes text
                frames[pipeline.done_token(st.line)] = (rec, st)
                put(pipeline.format_line(st.line))

    def advance(rec):                                  # a worker thread, or the pool's result thread: the current stage is done
        try:
            with lock:
                stage = rec.plan.pop(0)
                if stage != FINISH and rec.remove:
                    for q in (q for st in stage for q in st.remove):
                        if osp.exists(q):
                            os.remove(q)
                start(rec, workers.put_owed)
        except Exception as e:                         # (an exception would end the calling thread, and the run would hang)
            workers._fail("the plan of %s stopped: %r" % (rec.line.flow, e))

    def on_done(path):                                 # a worker thread: one line finished
        with lock:
            rec, st = frames.pop(path)
            counts[st.count] += 1
            rec.left -= 1
            if rec.left == 0:
                advance(rec)

    # --dm_bin builtin: the matcher and the solver must not share a GPU at the same time (the solver's resident kernel
    # needs the whole chip: arap_resident.h), so the run has two phases -- every pair is prepared and matched first
    # (one matcher server per GPU id), the servers exit, then the ARAP workers start and are fed.
    prepared = None
    if flags.dm_bin == "builtin":
        servers = start_matchers(flags, output_root)
        try:
            jobs = ((flags, p, bg) for p, bg in zip(all_paths, picks))
            prepared = list(pool.imap(prepare_pair, jobs, chunksize=1))
        finally:
            stop_matchers(flags, servers)
        print("Matching		%d pairs [Done]" % len(prepared))
    workers = GpuWorkers(flags.arap_bin, flags.gpu, flags.narap, serve, on_done)
    n_solves = n_frames = 0
    try:
        jobs = ((flags, p, bg) for p, bg in zip(all_paths, picks))
        for i, rec in enumerate(prepared if prepared is not None else pool.imap(prepare_pair, jobs, chunksize=1)):
            print("%.3f%%" % (float(i) * 100 / len(all_paths)))
            workers.check()
            if rec is None or not rec.solves:
                continue
            for _ in follow_up_steps(rec.plan):        # the workers stay open for every line the plan puts later
                workers.owe()
            with lock:
                start(rec, workers.put)
            n_solves += len(rec.solves)
            n_frames += 1
        workers.close()
        workers.join()
        for r in posts:
            r.get()
    finally:
        pool.terminate()
        for p in workers.procs:
            if p.poll() is None:
                p.kill()
    listed = all_paths
    if flags.resume and getattr(flags, "diag", False):     # the verdicts are on disk: list the pairs finished earlier too
        listed = scan(argparse.Namespace(**dict(vars(flags), resume=False)), input_root, output_root)
    out_paths, rejected = write_lists(flags, output_root, listed)
    dt = time.time() - t_start
    stats = dict(pairs=len(all_paths), frames=n_frames, solves=n_solves, seconds=dt,
                 **{k: v for k, v in counts.items() if k != "solves_done"},        # (`solves` above says it)
                 seconds_since_workers_ready=(time.time() - workers.t_ready) if workers.t_ready else None,
                 gpus=list(flags.gpu), worker="serve" if serve else "batch", jobs=flags.jobs, narap=flags.narap,
                 batches=workers.batches,
                 mean_batch=(float(np.mean(workers.batches)) if workers.batches else 0.0))
    if getattr(flags, "max_fold", None) is not None:
        stats["rejected"] = len(rejected)
    open(osp.join(output_root, "arap_stats.json"), "w").write(json.dumps(stats))
    print("Finished: %d frames (%d solves) in %.2f s, mean batch %.1f" % (n_frames, n_solves, dt, stats["mean_batch"]))
    return out_paths


def serves(flags):
    """are the workers persistent `arap_bin --serve` children?  --worker serve, or auto with this repository's C++ driver"""
    return flags.worker == "serve" or (flags.worker == "auto" and osp.abspath(flags.arap_bin.split()[0]) == CPP_BIN)


def own_arap_bin(cmd):
    """is --arap_bin this repository's driver (the C++ arap_deform, or arap_deform.py under an interpreter)?"""
    tok = cmd.split()
    own = {CPP_BIN, osp.join(HERE, "arap_deform.py")}
    return bool(tok) and (osp.abspath(tok[0]) in own or (len(tok) > 1 and osp.abspath(tok[1]) in own))


# What needs this repository's arap_deform: (the condition (`asked`), how the refusal names the flags, what a foreign
# --arap_bin does ...).  parse() says where in its order of checks each refusal stands (refuse).
FOREIGN = dict(
    seg=(("seg",), "--seg needs", "not know the seg line"),
    relight=(("relight",), "--relight needs", "not know the light line"),
    blur=(("blur",), "--blur needs", "not know the blur line"),
    tracks=(("tracks",), "--tracks needs", "not know the trk line"),
    retex=(("retex",), "--retex needs", "not know the tex line"),
    diag=(("diag",), "--diag / --max_fold need", "not write the diagnostics"),
    occ_layers=(("occ_layers",), "--occ_layers needs", "not know the layers line"),
    bwd_occ=(("bwd_flow", "occ"), "--bwd_flow / --occ need", "not write the extra outputs"),
    bg_motion=(("bg_motion",), "--bg_motion needs", "not know the bg line"),
    mid=(("mid",), "--mid needs", "not know the mid= token"),
    mid_layers=(("mid_layers",), "--mid_layers needs", "not know the layers line"))
# What a flag cannot be combined with: flag -> (the flags it excludes, why)
_SEQUENCES = ("mid", "mid_layers", "mid_bg")
EXCLUSIVE = dict(
    seg=(_SEQUENCES + ("retex", "blur", "relight"),
         "the variants share the clean pair's geometry files, and maps of in-between frames are made with opt.seg_maps, "
         "not from this command line"),
    relight=(_SEQUENCES + ("retex", "blur"),
             "relit sequences, twins and blurred frames are made with opt.relight, not from this command line"),
    blur=(_SEQUENCES + ("retex",),
          "blurred sequences and blurred twins are made with opt.blur_layers, not from this command line"),
    tracks=(("bg_motion",), "a track of a background point assumes the static background"),
    retex=(_SEQUENCES, "sequences of retextured in-between frames are not built"))


def parse(argv=None):
    parser = argparse.ArgumentParser(description="Arguments for ARAP flow generation")
    parser.add_argument("--input", type=str, required=True, help="Path to input root")
    parser.add_argument("--output", type=str, required=True, help="Path to output root")
    parser.add_argument("--rm-cnstr")
    parser.add_argument("--rm-wmask")
    parser.add_argument("--rm-tmp-cmd")
    parser.add_argument("--img-pattern")
    parser.add_argument("--gpu", nargs="*", type=int, default=[0], help="GPU id to be used, default=0")
    parser.add_argument("--multseg", action="store_true", default=False,
                        help="if each object segment is treated separately")
    parser.add_argument("--resume", action="store_true", default=False,
                        help="To skip the images that have *.flo finished.")
    # reference default: 7 (and never read there).  Here: the most list lines one GPU holds at a time -- enough for the
    # batch being solved, the one being uploaded and the one being assembled (8 854x480 frames or ~21 segments each).
    parser.add_argument("--narap", type=int, default=64, help="Number of buffered files to be run by ARAP on gpu")
    parser.add_argument("--size", nargs=2, default=None,
                        help="2-tuple of [width] [space] [height] to which all images are resized.")
    parser.add_argument("--fd", type=int, default=1, help="distance between the 2 frames, default=1")
    parser.add_argument("--arap_bin", default=CPP_BIN if osp.exists(CPP_BIN) else "%s %s" % (sys.executable, osp.join(HERE, "arap_deform.py")),
                        help="ARAP executable (argv contract of arap_deform), default: this repo's C++ driver "
                             "arap_flow_amd/bin/arap_deform when it is built, else arap_deform.py")
    parser.add_argument("--worker", choices=["auto", "serve", "batch"], default="auto",
                        help="serve: one persistent `arap_bin --serve` per GPU (this repo's C++ driver); batch: one "
                             "`arap_bin listfile` child per hand-out; auto: serve for this repo's driver")
    try:
        ncpu = len(os.sched_getaffinity(0))
    except AttributeError:
        ncpu = os.cpu_count() or 1
    try:                                                   # a container's CPU quota (cgroup v2), if any
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            ncpu = max(1, min(ncpu, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    parser.add_argument("--jobs", type=int, default=max(1, min(96, ncpu - 2)),
                        help="worker processes for the per-pair front end and back end")
    parser.add_argument("--dm_bin", default=None,
                        help="Path to the deep matching binary, or 'builtin': this repo's GPU matcher (libarapmatch.so)")
    parser.add_argument("--matches", default=None, help="directory of precomputed matches (instead of --dm_bin)")
    parser.add_argument("--bg_dir", default=None, help="directory of background images")
    parser.add_argument("--bg_motion", type=float, nargs="?", const=1.0, default=None, metavar="STRENGTH",
                        help="with --bg_dir: move the background between the two frames (a random similarity, STRENGTH "
                             "times 2 degrees, 1 %% scale and 3 px per frame of --fd; 1.0 when given bare) and write the "
                             "full-frame flow OUT/FlowFull/<seq>/<frame>.flo and, with --occ / --occ_layers / --bwd_flow, "
                             "OUT/OccFull, OUT/FlowBwdFull, OUT/OccBwdFull (DESIGN.md \"Moving background\")")
    parser.add_argument("--bwd_flow", action="store_true", default=False,
                        help="also write the backward flow OUT/FlowBwd/<seq>/<frame>.flo and the backward occlusion "
                             "OUT/OccBwd/<seq>/<frame>.png (DESIGN.md)")
    parser.add_argument("--occ", action="store_true", default=False,
                        help="also write the forward occlusion OUT/Occ/<seq>/<frame>.png (DESIGN.md)")
    parser.add_argument("--occ_layers", action="store_true", default=False,
                        help="with --multseg: also write the forward occlusion across segments OUT/Occ/<seq>/<frame>.png, "
                             "from one layered warp per frame (DESIGN.md \"Layered warp\")")
    parser.add_argument("--mid", type=int, default=0, metavar="K",
                        help="also write K in-between frames per pair, from K ramp steps spread evenly over the solve's "
                             "constraint ramp: OUT/Mid/<seq>/<frame>_sII{.flo,.png,_mask.png,_step.flo} (DESIGN.md "
                             "\"In-between frames\")")
    parser.add_argument("--mid_layers", type=int, default=0, metavar="K",
                        help="with --multseg: also write K layered in-between frames per pair, merged from every "
                             "segment's ramp snapshots by one layered pass per snapshot: OUT/Mid/<seq>/<frame>_sII"
                             "{.flo,.png,_mask.png,_step.flo}; with --occ_layers also the link occlusions "
                             "<frame>_s00_occ.png, <frame>_sII_occ.png (DESIGN.md \"Layered in-between frames\")")
    parser.add_argument("--keep_segments", action="store_true", default=False,
                        help="with --multseg: keep the per-segment files after they are merged (for inspection)")
    parser.add_argument("--mid_bg", action="store_true", default=False,
                        help="with --bg_motion and --mid K or --multseg --mid_layers K: move the camera through the "
                             "in-between frames too and write OUT/MidFull/<seq>/<frame>_sII.png (the in-between frame over "
                             "the moving background) and _s00_step.flo, _sII_step.flo (the full-frame flow of every link); "
                             "with --mid_layers K --occ_layers also the links' full-frame occlusions _s00_occ.png, "
                             "_sII_occ.png.  A plain --mid K run has no object-side link occlusion, so it writes none and "
                             "cannot be combined with --occ here (DESIGN.md \"Moving background over in-between frames\")")
    parser.add_argument("--diag", action="store_true", default=False,
                        help="also write the fold diagnostics of every pair: the mesh statistics OUT/Diag/<seq>/<frame>.txt "
                             "and the fold map OUT/Fold/<seq>/<frame>.png, 255 where the flow value is no valid "
                             "correspondence (DESIGN.md \"Fold diagnostics\")")
    parser.add_argument("--max_fold", type=float, default=None, metavar="FRAC",
                        help="implies --diag: leave a pair out of all_files.list and all_files_ext.list, and name it in "
                             "OUT/rejected.list, when a triangle of its mesh went non-finite or more than FRAC (0 .. 1) of "
                             "them folded; its files stay on disk")
    parser.add_argument("--retex", action="store_true", default=False,
                        help="also write the random-texture twin of every pair: OUT/inpRGB_tex/<seq>/<frame>.png, frame 1 "
                             "with a procedural texture on every object (one per segment with --multseg), OUT/wRGB_tex/"
                             "<seq>/<frame>.png, its warp with the pair's solved flows, and OUT/all_files_tex.list, whose "
                             "lines name those two and the pair's own Flow file (DESIGN.md \"Random textures\")")
    parser.add_argument("--tracks", type=int, default=0, metavar="P",
                        help="with --mid K or --multseg --mid_layers K: also write the tracks of P query points of frame 1 "
                             "through the K in-between frames to frame 2, sub-pixel positions and occluded flags: "
                             "OUT/Tracks/<seq>/<frame>.trk (DESIGN.md \"Point tracks\")")
    parser.add_argument("--blur", nargs="+", default=None, metavar=("SHUTTER", "SAMPLES"),
                        help="with --bg_dir: also write the motion-blurred variant of every pair: OUT/inpRGB_blur/<seq>/"
                             "<frame>.png and OUT/wRGB_blur/<seq>/<frame>.png, frame 1 and frame 2 exposed over a window of "
                             "SHUTTER (in units of the pair's motion, centred on the frame) as the mean of SAMPLES renders "
                             "(1 .. 32, default 9), and OUT/all_files_blur.list, whose lines name those two and the pair's own "
                             "Flow file (DESIGN.md \"Motion blur\")")
    parser.add_argument("--relight", nargs="?", type=float, const=1.0, default=None, metavar="STRENGTH",
                        help="with --bg_dir: also write the relit variant of every pair: OUT/inpRGB_light/<seq>/<frame>.png and "
                             "OUT/wRGB_light/<seq>/<frame>.png, the pair's two frames under a soft shadow of the objects, a "
                             "drifting illumination field, a flickering tone curve, a vignette and sensor noise, every "
                             "amplitude scaled by STRENGTH (default 1), and OUT/all_files_light.list, whose lines name those "
                             "two and the pair's own Flow file (DESIGN.md \"Relit frames\")")
    parser.add_argument("--seg", nargs="*", default=None, metavar="TAU [RADIUS]",
                        help="also write the segment maps of every pair, 8-bit PNGs named like its flow file: OUT/Index1 and "
                             "OUT/Index2 (object index per pixel of frame 1 / frame 2), OUT/MB and OUT/MBBwd (255 where the "
                             "full forward / backward flow jumps by more than TAU pixels, default 1), OUT/MBDist and "
                             "OUT/MBDistBwd (whole pixels to the nearest such pixel up to RADIUS, default 140, at most 254; "
                             "255 beyond) (DESIGN.md \"Segment maps\")")
    flags = parser.parse_args(argv)

    def refuse(key):            # the refusals of `key`: EXCLUSIVE's, if it has a row, then FOREIGN's.  A flag counts as given
        others, reason = EXCLUSIVE.get(key, ((), ""))      # by `asked`, also while --blur / --seg still hold their raw lists
        if asked(others, flags):
            parser.error("--%s cannot be combined with %s: %s" % (key, " / ".join("--" + n for n in others), reason))
        when, subject, lacks = FOREIGN[key]
        if asked(when, flags) and not own_arap_bin(flags.arap_bin):
            parser.error("%s this repository's arap_deform (C++ or arap_deform.py): a foreign --arap_bin does %s" % (subject, lacks))

    if flags.seg is not None:
        try:
            if len(flags.seg) > 2:
                raise ValueError
            tau = float(np.float32(float(flags.seg[0]))) if flags.seg else 1.0
            radius = int(flags.seg[1]) if len(flags.seg) == 2 else 140
        except (ValueError, OverflowError):
            parser.error("--seg [TAU [RADIUS]]: a number and an integer")
        if not (np.isfinite(tau) and tau >= 0) or not 0 <= radius <= pipeline.SEG_MAX_RADIUS:
            parser.error("--seg [TAU [RADIUS]]: a finite TAU >= 0 and a RADIUS of 0 .. %d" % pipeline.SEG_MAX_RADIUS)
        flags.seg = (tau, radius)
        refuse("seg")
    if flags.relight is not None:
        if not (np.isfinite(flags.relight) and flags.relight >= 0):
            parser.error("--relight [STRENGTH]: a finite STRENGTH >= 0")
        if not flags.bg_dir:
            parser.error("--relight needs --bg_dir: a shadow needs a background to fall on")
        refuse("relight")
    if flags.blur is not None:
        try:
            if len(flags.blur) > 2:
                raise ValueError
            shutter = float(np.float32(float(flags.blur[0])))
            samples = int(flags.blur[1]) if len(flags.blur) == 2 else 9
        except (ValueError, OverflowError):
            parser.error("--blur SHUTTER [SAMPLES]: a number and an optional integer")
        if not (np.isfinite(shutter) and shutter >= 0) or not 1 <= samples <= pipeline.MAX_BLUR_SAMPLES:
            parser.error("--blur SHUTTER [SAMPLES]: a finite SHUTTER >= 0 and 1 .. %d SAMPLES" % pipeline.MAX_BLUR_SAMPLES)
        flags.blur = (shutter, samples)
        if not flags.bg_dir:
            parser.error("--blur needs --bg_dir: a blurred object needs a defined background behind it")
        refuse("blur")
    if flags.tracks:
        if not 1 <= flags.tracks <= 1 << 24:
            parser.error("--tracks P: 1 .. 2^24 points")
        if not (flags.mid or (flags.multseg and flags.mid_layers)):
            parser.error("--tracks needs --mid K or --multseg --mid_layers K: the states a point is tracked through")
        refuse("tracks")
    if flags.retex:
        refuse("retex")
    if flags.max_fold is not None:
        if not 0 <= flags.max_fold <= 1:                   # (false on NaN)
            parser.error("--max_fold FRAC must lie in 0 .. 1")
        flags.diag = True
    refuse("diag")
    if flags.mid_bg:
        if flags.bg_motion is None:
            parser.error("--mid_bg needs --bg_motion: it moves that camera through the in-between frames")
        if not (flags.mid or flags.mid_layers):
            parser.error("--mid_bg needs --mid K or --multseg --mid_layers K: there is no in-between frame")
        if flags.mid and flags.occ:
            parser.error("--mid_bg with --mid K cannot be combined with --occ: the pair's occlusion would ask for link "
                         "occlusions, which a --mid K run does not make; use --multseg --mid_layers K --occ_layers")
    if flags.occ and flags.multseg:
        parser.error("--occ cannot be combined with --multseg: forward occlusion across segments needs one query over "
                     "every segment's solve, which --occ does not do; use --multseg --occ_layers (--bwd_flow --multseg "
                     "is supported)")
    if flags.occ_layers and not flags.multseg:
        parser.error("--occ_layers needs --multseg (a single-object run takes --occ)")
    refuse("occ_layers")
    refuse("bwd_occ")
    if flags.bg_motion is not None:
        if not flags.bg_dir:
            parser.error("--bg_motion needs --bg_dir: there is no background to move")
        if (flags.mid or flags.mid_layers) and not flags.mid_bg:
            parser.error("--bg_motion cannot be combined with --mid / --mid_layers: the background motion of an "
                         "in-between frame needs the motion interpolated per snapshot, which is not built without "
                         "--mid_bg")
        refuse("bg_motion")
        if not (flags.bg_motion >= 0 and np.isfinite(flags.bg_motion)):
            parser.error("--bg_motion STRENGTH must be a finite number >= 0")
    flags.mid_steps = []
    if flags.mid:
        if flags.multseg:
            parser.error("--mid cannot be combined with --multseg: merging the segments' in-between states is a "
                         "separate piece of work, which --multseg --mid_layers K does")
        refuse("mid")
        try:
            flags.mid_steps = pipeline.mid_steps(flags.mid, NUM_ITER)
        except ValueError as e:
            parser.error(str(e))
    flags.mid_layers_steps = []
    if flags.mid_layers:
        if not flags.multseg:
            parser.error("--mid_layers needs --multseg (a single-object run takes --mid)")
        refuse("mid_layers")
        try:
            flags.mid_layers_steps = pipeline.mid_steps(flags.mid_layers, NUM_ITER)
        except ValueError as e:
            parser.error(str(e))
    if flags.size is not None:
        flags.size = tuple(int(s) for s in flags.size)
    assert 0 < flags.fd < 20, "Invalid fd number!"
    assert flags.dm_bin is not None or flags.matches is not None, "give --dm_bin or --matches"
    if flags.dm_bin is not None and flags.dm_bin != "builtin":
        assert osp.exists(flags.dm_bin), "File not found " + flags.dm_bin
    return flags


if __name__ == "__main__":
    logging.basicConfig(filename="example.log", level=logging.DEBUG)
    main(parse())
