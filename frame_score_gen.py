#!/usr/bin/env python3
"""Score estimated frames against a generated dataset (DESIGN.md "Frame scoring").

    frame_score_gen.py --data OUT --est EST_ROOT [--from_flows] [--full] [--baseline blend] [--gpu 0 1 ..] [--narap N]
                       [--arap_bin CMD] [--worker auto|serve|batch]

OUT is a tree para_gen.py wrote.  Every ground-truth frame is scored against the file of the same name relative to OUT
under EST_ROOT (OUT/Mid/a/00003_s09.png against EST_ROOT/Mid/a/00003_s09.png) by one `fscore` line of arap_deform
(pipeline.FScoreLine) on para_gen.py's workers, one persistent `arap_deform --serve` per GPU.  The ground truth:

  default   every in-between frame OUT/Mid/<seq>/<frame>_sNN.png (--mid, --mid_layers) and every frame 2
            OUT/wRGB/<seq>/<frame>.png
  --full    every in-between frame OUT/MidFull/<seq>/<frame>_sNN.png (--mid_bg)

A plane is passed only where a file defined in the scored frame's own pixel grid exists:

  Mid, MidFull  occ=<frame>_sNN_occ.png beside the frame: the occlusion of the link that starts at that snapshot
  wRGB          occ=OUT/OccBwd/<seq>/<frame>.png, the frame-2 pixels frame 1 does not show, and
                dist=OUT/MBDistBwd/<seq>/<frame>.png, the distance to a motion boundary in frame 2

Occ, MBDist, Fold and inpMasks live in frame 1's grid and are never passed; the warped masks (wMasks, _sNN_mask.png) are
in the right grid but non-zero on the object, the opposite of obj=, so the obj and bg rows stay empty here.

  --baseline blend   no estimate is read: for every in-between ground truth the rounded mean (a + b + 1) >> 1 of the
                     pair's two end frames OUT/inpRGB/<seq>/<frame>.png and OUT/wRGB/<seq>/<frame>.png is written, in
                     numpy, to OUT/FramesEst/<same relative name>, and that tree is scored: the figure an interpolator has
                     to beat.  (A frame 2 has no such estimate and is listed as missing.)

  --from_flows       (with --est, not with --baseline) EST_ROOT holds flow estimates, not frames: for every pair that has
                     in-between ground truth one `interp` line (pipeline.InterpLine, DESIGN.md "Frames from flows") on the
                     same workers turns OUT/inpRGB/<seq>/<frame>.png, OUT/wRGB/<seq>/<frame>.png and
                     EST_ROOT/Flow/<seq>/<frame>.flo -- with bwd=EST_ROOT/FlowBwd/<seq>/<frame>.flo where that file
                     exists; with --full FlowFull and FlowBwdFull, between the same two frames, which --mid_bg composites
                     -- into OUT/FramesEst/<Mid|MidFull>/<seq>/<frame>_sNN.png, at the steps of the _sNN names present
                     with n = para_gen.NUM_ITER, and that tree is scored exactly as --baseline blend's is: the Middlebury
                     interpolation error of a flow method.  A pair without a flow estimate is listed as missing, and so is
                     every frame 2.  --est OUT scores the dataset's own flow files: the oracle-flow ceiling, beside the
                     blend floor.

Written: OUT/FrameScore/<seq>/<name>.txt per frame (pipeline.format_frame_score), their exact pooled table
OUT/frame_score.txt (pipeline.add_frame_scores) and OUT/frame_score_missing.list, the ground-truth frames without an
estimate, which are counted and no error.  Prints the summary (pipeline.frame_score_summary) of the pooled table -- PSNR
and SSIM over all pixels and windows together --, the mean of the per-frame PSNRs over the frames with sse > 0, which is what
the interpolation papers report, and the number of exact frames, which have none.
"""
import argparse
import os
import os.path as osp
import re
import sys

import numpy as np
from PIL import Image

HERE = osp.dirname(osp.abspath(__file__))
sys.path.insert(0, HERE)
import para_gen                             # noqa: E402
import score_cli                            # noqa: E402
from arap_flow_amd import pipeline          # noqa: E402

MID_FRAME = re.compile(r"^(.*)_s(\d\d)\.png$")
EST_DIR = "FramesEst"


def ground_truth(data, full):
    """[(directory under OUT, seq, name without .png, pair stem or None)] of the frames to score; the stem of an
    in-between frame is its pair's, a frame 2 has None"""
    found = []
    for top in ([para_gen.mid_full_dir] if full else [para_gen.mid_dir, para_gen.wrgb_dir]):
        root = osp.join(data, top)
        for d, _, fs in sorted(os.walk(root)):
            for f in sorted(fs):
                m = MID_FRAME.match(f)
                if (m is None) != (top == para_gen.wrgb_dir) or not f.endswith(".png"):
                    continue
                found.append((top, osp.relpath(d, root), f[:-4], m.group(1) if m else None))
    return found


def planes_of(data, top, seq, name):
    """{key: path} of the planes defined in the frame's own grid (the module's docstring), those whose file exists"""
    if top == para_gen.wrgb_dir:
        planes = dict(occ=osp.join(data, para_gen.occ_bwd_dir, seq, name + ".png"),
                      dist=osp.join(data, para_gen.SEG_DIRS["dist2"], seq, name + ".png"))
    else:
        planes = dict(occ=osp.join(data, top, seq, name + "_occ.png"))
    return {k: p for k, p in planes.items() if osp.exists(p)}


def write_blend(data, full):
    """--baseline blend: OUT/FramesEst/<relative name> of every in-between ground truth whose two end frames exist"""
    for top, seq, name, stem in ground_truth(data, full):
        ends = [osp.join(data, d, seq, "%s.png" % stem) for d in (para_gen.color_dir, para_gen.wrgb_dir)]
        if stem is None or not all(osp.exists(e) for e in ends):
            continue
        a, b = (pipeline.load_rgb(e).astype(np.uint16) for e in ends)
        out = osp.join(data, EST_DIR, top, seq, name + ".png")
        os.makedirs(osp.dirname(out), exist_ok=True)
        Image.fromarray(((a + b + 1) >> 1).astype(np.uint8)).save(out)


def interp_items(data, est_root, full):
    """--from_flows: {output prefix: InterpLine} of every pair with in-between ground truth, both end frames and a flow
    estimate; a prefix is OUT/FramesEst/<Mid|MidFull>/<seq>/<frame>"""
    steps = {}
    for top, seq, name, stem in ground_truth(data, full):
        if stem is not None:
            steps.setdefault((top, seq, stem), []).append(int(name[-2:]))
    items = {}
    for (top, seq, stem), idx in sorted(steps.items()):
        a, b = (osp.join(data, d, seq, stem + ".png") for d in (para_gen.color_dir, para_gen.wrgb_dir))
        fwd = osp.join(est_root, para_gen.full_dir if full else para_gen.flow_dir, seq, stem + ".flo")
        bwd = osp.join(est_root, para_gen.bwd_full_dir if full else para_gen.bwd_dir, seq, stem + ".flo")
        idx = tuple(sorted(set(idx)))
        if not all(osp.exists(f) for f in (a, b, fwd)) or idx[0] < 1 or idx[-1] >= para_gen.NUM_ITER:
            continue
        prefix = osp.join(data, EST_DIR, top, seq, stem)
        os.makedirs(osp.dirname(prefix), exist_ok=True)
        items[prefix] = pipeline.InterpLine(a, b, fwd, idx, para_gen.NUM_ITER, bwd if osp.exists(bwd) else "", False, prefix)
    return items


def score_items(data, est_root, full, promised=None):
    """-> ([FScoreLine], [ground-truth files without an estimate]); `promised`: the estimates an interp line is about to
    write -- given, only those count as there (--from_flows: a file an earlier run left in OUT/FramesEst is no estimate)"""
    items, missing = [], []
    for top, seq, name, _ in ground_truth(data, full):
        gt, est = osp.join(data, top, seq, name + ".png"), osp.join(est_root, top, seq, name + ".png")
        if (est not in promised) if promised is not None else not osp.exists(est):
            missing.append(gt)
            continue
        out = osp.join(data, "FrameScore", seq, name + ".txt")
        os.makedirs(osp.dirname(out), exist_ok=True)
        items.append(pipeline.FScoreLine(gt, est, planes_of(data, top, seq, name), out))
    return items, missing


def summary_text(table):
    s = pipeline.frame_score_summary(table)
    text = "%-9s %11s %9s %8s %11s %9s %9s\n" % ("class", "pixels", "PSNR dB", "MAE", "windows", "SSIM", "SSIM min")
    for name in pipeline.FSCORE_ROWS[:-1]:
        r = s[name]
        text += "%-9s %11d %9.4f %8.4f %11d %9.6f %9.6f\n" % (name, r["count"], r["psnr"], r["mae"], r["windows"], r["ssim"], r["ssim_min"])
    left = s[pipeline.FSCORE_ROWS[-1]]
    return text + "left out: %d pixels, %d windows\n" % (left["pixels"], left["windows"])


def main(flags):
    data = osp.abspath(flags.data)
    if flags.baseline:
        write_blend(data, flags.full)
    interp, promised = {}, None
    if flags.from_flows:
        interp = interp_items(data, osp.abspath(flags.est), flags.full)
        promised = {pipeline.interp_files(prefix, i)["rgb"]: prefix for prefix, it in interp.items() for i in it.steps}
    items, missing = score_items(data, osp.join(data, EST_DIR) if flags.baseline or flags.from_flows else osp.abspath(flags.est),
                                 flags.full, promised)
    after = {}                                  # an interp line's prefix -> the lines that score its frames
    for it in items:
        if promised is not None:
            after.setdefault(promised[it.est], []).append(it)
    score_cli.run_lines(flags, items if promised is None else [interp[prefix] for prefix in after], after)
    tables = [pipeline.parse_frame_score_file(open(it.out).read()) for it in items]
    pooled = pipeline.add_frame_scores(tables)
    score_cli.write_results(data, "frame_score", pipeline.format_frame_score(pooled), missing)
    print("%d frames scored, %d without an estimate" % (len(items), len(missing)))
    print(summary_text(pooled), end="")
    psnr = [pipeline.frame_score_summary(t)["all"]["psnr"] for t in tables if int(t[0, 1]) > 0 and int(t[0, 0]) > 0]
    exact = sum(1 for t in tables if int(t[0, 1]) == 0)
    print("mean of the per-frame PSNRs: %s over %d frames; %d exact frames" %
          ("%.4f dB" % (sum(psnr) / len(psnr)) if psnr else "none", len(psnr), exact))
    return pooled


def parse(argv=None):
    parser = argparse.ArgumentParser(description="PSNR / SSIM tables of estimated frames against a para_gen.py dataset")
    parser.add_argument("--data", required=True, help="the dataset: para_gen.py's --output")
    parser.add_argument("--est", help="the estimates: EST/<Mid|wRGB|MidFull>/<seq>/<name>.png, named like the dataset's frames")
    parser.add_argument("--full", action="store_true", help="score the in-between frames of MidFull instead of Mid and wRGB")
    parser.add_argument("--baseline", choices=["blend"], help="score the rounded mean of a pair's end frames instead of --est")
    parser.add_argument("--from_flows", action="store_true", help="--est holds flow estimates: splat them into OUT/FramesEst first")
    score_cli.add_worker_options(parser)
    flags = parser.parse_args(argv)
    if (flags.est is None) == (flags.baseline is None):
        parser.error("one of --est and --baseline is needed")
    if flags.from_flows and flags.est is None:
        parser.error("--from_flows needs --est, the root of the flow estimates, and excludes --baseline")
    score_cli.check_driver(parser, flags, "an `fscore` line")
    return flags


if __name__ == "__main__":
    main(parse())
