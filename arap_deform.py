#!/usr/bin/env python3
"""arap_deform -- command-line twin of the reference's executable (ARAP/deformation/src/main.cpp:162-241).

  python arap_deform.py RGB Mask Constraint Flow warped_RGB warped_Mask       (one frame)
  python arap_deform.py listfile                                              (one solve per line, 6 paths)

A list line may carry optional output tokens after its six paths (backward flow, forward and backward occlusion), and
a line whose first word is `layers` is no solve but the layered warp of one frame, one whose first word is `bg` the
moving-background pass of one pair, one whose first word is `tex` the random-texture twin of one frame, one whose first
word is `trk` the point tracks of one sequence, one whose first word is `blur` the motion-blurred frames of one pair, one
whose first word is `light` the relit frames of one pair, one whose first word is `seg` the segment maps of one pair, one
whose first word is `score` the error table of one estimated flow, one whose first word is `tscore` the TAP-Vid table of
one estimated track file, one whose first word is `chain` the track file of chained flow estimates, one whose first word
is `fscore` the PSNR / SSIM table of one estimated frame, one whose first word is `interp` the in-between frames of a
pair from a flow estimate, one whose first word is `lscore` the DAVIS J / F table of one estimated label map, one whose
first word is `mscore` the precision / recall table of one estimated occlusion or motion-boundary map: the forms are
defined in arap_flow_amd/pipeline.py (SolveLine, parse_layers, BgLine, TexLine, TrkLine, BlurLine, LightLine, SegLine,
ScoreLine, TScoreLine, ChainLine, FScoreLine, InterpLine, LScoreLine, MScoreLine).  Any line that is no solve runs once every earlier line of the list is solved and written (its
inputs may be their outputs).

Same argument contract, same fixed schedule (numIter 19, nonLinearIter 8, linearIter 400, main.cpp:215-221),
same border pins, same outputs (.flo + two PNGs).  ARAP_PLAN may name the reference's arap_plan.t; it is then
checked by Opt_ProblemDefine (anything that is not the ARAP energy is rejected); unset = built-in energy.
The GPU is selected with HIP_VISIBLE_DEVICES where the reference used CUDA_VISIBLE_DEVICES.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def usage():
    print("Usage:\n")
    print("./arap_deform RGB Mask Constraint Flow warped_RGB warped_Mask\n")
    print("Mask and warp image using the provided optical flow field.\n")
    print("RGB \t\t [input]  path to an input RGB image (.png only)")
    print("Mask\t\t [input]  path to an input mask image (.png only) where 0 for object, 1 for background")
    print("Constraint \t [input]  path to list of constraints, text file")
    print("Flow \t\t [output] path to optical flow image with (.flo only)")
    print("warped_RGB \t [output] path to output warped image (.png), all intermediate directories must exist")
    print("warped_Mask \t [output] path to output warped mask (.png), all intermediate directories must exist")


def main(argv):
    from arap_flow_amd import opt, pipeline
    if len(argv) == 7:
        lines = [pipeline.SolveLine(*argv[1:7], extra={})]
    elif len(argv) == 2:
        try:
            lines = pipeline.read_list_items(argv[1])
        except ValueError as e:
            print(e)
            return 1
    else:
        print("Invalid Input!")
        usage()
        return 1
    if not lines:
        print("No file to be processed")
        return 1
    state = opt.State()
    plan = os.environ.get("ARAP_PLAN")
    if plan is not None:
        print("Optimization plan at %s" % plan)
        if not os.path.exists(plan):
            print(" Not found! Please run export ARAP_PLAN=/path/to/plan.t or copy the file to the running "
                  "folder with name arap_plan.t")
            return 1
        pr = state.lib.Opt_ProblemDefine(state.handle, plan.encode(), b"gaussNewtonGPU")
        if not pr:
            return 1
        state.lib.Opt_ProblemDelete(state.handle, pr)
    # runs of solve lines go to the batched solver; any other line waits for the run before it
    k = 0
    while k < len(lines):
        if not isinstance(lines[k], pipeline.SolveLine):
            if isinstance(lines[k], pipeline.BgLine):
                pipeline.run_background(state, lines[k])
            elif isinstance(lines[k], pipeline.TexLine):
                pipeline.run_texture(state, lines[k])
            elif isinstance(lines[k], pipeline.TrkLine):
                pipeline.run_tracks(state, lines[k])
            elif isinstance(lines[k], pipeline.BlurLine):
                pipeline.run_blur(state, lines[k])
            elif isinstance(lines[k], pipeline.LightLine):
                pipeline.run_light(state, lines[k])
            elif isinstance(lines[k], pipeline.SegLine):
                pipeline.run_seg(state, lines[k])
            elif isinstance(lines[k], pipeline.ScoreLine):
                pipeline.run_score(state, lines[k])
            elif isinstance(lines[k], pipeline.TScoreLine):
                pipeline.run_tscore(state, lines[k])
            elif isinstance(lines[k], pipeline.ChainLine):
                pipeline.run_chain(state, lines[k])
            elif isinstance(lines[k], pipeline.FScoreLine):
                pipeline.run_fscore(state, lines[k])
            elif isinstance(lines[k], pipeline.InterpLine):
                pipeline.run_interp(state, lines[k])
            elif isinstance(lines[k], pipeline.LScoreLine):
                pipeline.run_lscore(state, lines[k])
            elif isinstance(lines[k], pipeline.MScoreLine):
                pipeline.run_mscore(state, lines[k])
            else:
                pipeline.run_layers(state, lines[k])
            print("Saved")
            k += 1
            continue
        e = k
        while e < len(lines) and isinstance(lines[e], pipeline.SolveLine):
            e += 1
        pipeline.deform_list(state, lines[k:e], 19, 8, 400)
        k = e
    state.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
