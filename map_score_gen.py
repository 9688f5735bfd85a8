#!/usr/bin/env python3
"""Score estimated occlusion, motion-boundary and object index maps against a generated dataset (DESIGN.md "Map scoring").

    map_score_gen.py --data OUT --est EST_ROOT [--full] [--radius R] [--thr T,..] [--baseline still] [--gpu 0 1 ..]
                     [--narap N] [--arap_bin CMD] [--worker auto|serve|batch]

OUT is a tree para_gen.py wrote.  Every ground-truth map is scored against the file of the same name relative to OUT under
EST_ROOT (OUT/Occ/a/00003.png against EST_ROOT/Occ/a/00003.png) by one line of arap_deform on para_gen.py's workers, one
persistent `arap_deform --serve` per GPU.  The ground truth and its line:

  Occ, OccBwd        (with --full: OccFull, OccBwdFull) an `mscore` line without thresholds (pipeline.MScoreLine): the
                     histogram behind the pixelwise precision / recall curve, its average precision and best F
  MB, MBBwd          an `mscore` line with t=--thr (default 64,128,192) and r=the radius: also the tolerant boundary match
  Index1, Index2     an `lscore` line (pipeline.LScoreLine) with l= the largest label of the ground-truth file (1 if it has
                     none) and r=the radius: DAVIS J and F per object

The radius defaults to the DAVIS toolkit's ceil(0.008 * sqrt(W^2 + H^2)) of the map's own size, 8 at 854 x 480.  A map of
frame 1 (Occ, OccFull, MB, Index1) gets skip=OUT/Fold/<seq>/<frame>.png where that file exists.

  --baseline still   no estimate is read: OUT/Index1/<seq>/<frame>.png is scored as the estimate of OUT/Index2/<seq>/
                     <frame>.png, the floor with nothing moved; only Index2 is scored.
  --est OUT          the ceiling: every J, F and AP is 1.

Written: OUT/MapScore/<Dir>/<seq>/<frame>.txt per map (pipeline.format_label_score / format_map_score), their exact
pooled scores per directory in OUT/map_score.txt (`[Dir]`, then the pooled file's text) and OUT/map_score_missing.list, the
ground-truth maps without an estimate, which are counted and no error.  Prints the summary of every directory.
"""
import argparse
import math
import os
import os.path as osp
import sys

import numpy as np
from PIL import Image

HERE = osp.dirname(osp.abspath(__file__))
sys.path.insert(0, HERE)
import para_gen                             # noqa: E402
import score_cli                            # noqa: E402
from arap_flow_amd import pipeline          # noqa: E402

SCORE_DIR = "MapScore"
DEFAULT_THR = (64, 128, 192)


def directories(full):
    """{directory under OUT: (kind, whether it lies in frame 1's grid)} in the order they are scored and printed"""
    occ = [(para_gen.occ_full_dir, True), (para_gen.occ_bwd_full_dir, False)] if full else \
          [(para_gen.occ_dir, True), (para_gen.occ_bwd_dir, False)]
    dirs = {d: ("occ", first) for d, first in occ}
    dirs.update({para_gen.SEG_DIRS["mb1"]: ("mb", True), para_gen.SEG_DIRS["mb2"]: ("mb", False),
                 para_gen.SEG_DIRS["idx1"]: ("idx", True), para_gen.SEG_DIRS["idx2"]: ("idx", False)})
    return dirs


def ground_truth(data, full, only=None):
    """[(directory under OUT, seq, name without .png)] of the maps to score"""
    found = []
    for top in directories(full):
        root = osp.join(data, top)
        if only is not None and top not in only:
            continue
        for d, _, fs in sorted(os.walk(root)):
            found += [(top, osp.relpath(d, root), f[:-4]) for f in sorted(fs) if f.endswith(".png")]
    return found


def davis_radius(W, H):
    """the DAVIS toolkit's bound_th = 0.008 of the diagonal, rounded up"""
    return min(int(math.ceil(0.008 * math.sqrt(W * W + H * H))), pipeline.SEG_MAX_RADIUS)


def score_items(data, est_root, full, radius=None, thr=DEFAULT_THR, still=False):
    """-> ([(directory, line)], [ground-truth files without an estimate])"""
    dirs = directories(full)
    idx1, idx2 = para_gen.SEG_DIRS["idx1"], para_gen.SEG_DIRS["idx2"]
    items, missing = [], []
    for top, seq, name in ground_truth(data, full, [idx2] if still else None):
        gt = osp.join(data, top, seq, name + ".png")
        est = osp.join(data, idx1, seq, name + ".png") if still else osp.join(est_root, top, seq, name + ".png")
        if not osp.exists(est):
            missing.append(gt)
            continue
        kind, first = dirs[top]
        fold = osp.join(data, para_gen.fold_dir, seq, name + ".png")
        skip = fold if first and osp.exists(fold) else None
        out = osp.join(data, SCORE_DIR, top, seq, name + ".txt")
        os.makedirs(osp.dirname(out), exist_ok=True)
        with Image.open(gt) as im:
            r = davis_radius(*im.size) if radius is None else radius
            top_label = int(pipeline.load_mask_red(gt).max()) if kind == "idx" else 0
        if kind == "idx":
            items.append((top, pipeline.LScoreLine(gt, est, max(top_label, 1), r, skip, out)))
        elif kind == "mb" and thr:
            items.append((top, pipeline.MScoreLine(gt, est, tuple(thr), r, skip, out)))
        else:
            items.append((top, pipeline.MScoreLine(gt, est, (), None, skip, out)))
    return items, missing


def pooled_text(pooled):
    """OUT/map_score.txt: `[Dir]` and the directory's pooled score as its file's text, directory after directory"""
    return "".join("[%s]\n%s" % (top, pipeline.format_label_score(p) if isinstance(p, np.ndarray) else pipeline.format_map_score(p))
                   for top, p in pooled.items())


def summary_text(pooled, per_file):
    """the printed summary: per directory the figures of the pooled score and the mean of the per-file figures"""
    mean = lambda v: sum(v) / len(v) if v else float("nan")
    text = ""
    for top, p in pooled.items():
        files = per_file[top]
        if isinstance(p, np.ndarray):
            s, fs = pipeline.label_score_summary(p), [pipeline.label_score_summary(t) for t in files]
            text += "%-11s %4d maps  J %.6f  F %.6f  J&F %.6f pooled;  J %.6f  F %.6f  J&F %.6f mean of maps\n" % (
                top, len(files), s["J"], s["F"], s["JF"], mean([f["J"] for f in fs]), mean([f["F"] for f in fs]), mean([f["JF"] for f in fs]))
            for k, v in s["labels"].items():
                text += "  label %-3d J %.6f  P %.6f  R %.6f  F %.6f\n" % (k, v["J"], v["P"], v["R"], v["F"])
        else:
            s, fs = pipeline.map_score_summary(p), [pipeline.map_score_summary(t) for t in files]
            text += "%-11s %4d maps  AP %.6f  F@128 %.6f  best F %.6f at %d pooled;  AP %.6f  best F %.6f mean of maps\n" % (
                top, len(files), s["ap"], s["f128"], s["best_f"], s["best_t"], mean([f["ap"] for f in fs]), mean([f["best_f"] for f in fs]))
            for t, v in s["match"].items():
                text += "  thr %-3d   P %.6f  R %.6f  F %.6f within the radius\n" % (t, v["P"], v["R"], v["F"])
    return text


def main(flags):
    data = osp.abspath(flags.data)
    still = flags.baseline == "still"
    items, missing = score_items(data, None if still else osp.abspath(flags.est), flags.full, flags.radius, flags.thr, still)
    score_cli.run_lines(flags, [it for _, it in items])
    per_file = {}
    for top, it in items:
        text = open(it.out).read()
        per_file.setdefault(top, []).append(pipeline.parse_label_score_file(text) if isinstance(it, pipeline.LScoreLine)
                                            else pipeline.parse_map_score_file(text))
    pooled = {top: pipeline.add_label_scores(ts) if isinstance(ts[0], np.ndarray) else pipeline.add_map_scores(ts)
              for top, ts in per_file.items()}
    score_cli.write_results(data, "map_score", pooled_text(pooled), missing)
    print("%d maps scored, %d without an estimate" % (len(items), len(missing)))
    print(summary_text(pooled, per_file), end="")
    return pooled


def parse(argv=None):
    parser = argparse.ArgumentParser(description="J / F and precision / recall tables of estimated maps against a para_gen.py dataset")
    parser.add_argument("--data", required=True, help="the dataset: para_gen.py's --output")
    parser.add_argument("--est", help="the estimates: EST/<Occ|OccBwd|MB|MBBwd|Index1|Index2>/<seq>/<frame>.png, named like the dataset's maps")
    parser.add_argument("--full", action="store_true", help="score OccFull and OccBwdFull instead of Occ and OccBwd")
    parser.add_argument("--radius", type=int, help="the tolerance of the boundary match; default 0.008 of the diagonal, rounded up")
    parser.add_argument("--thr", default=",".join("%d" % t for t in DEFAULT_THR), help="thresholds of the tolerant match of MB and MBBwd")
    parser.add_argument("--baseline", choices=["still"], help="score Index1 as the estimate of Index2 instead of --est")
    score_cli.add_worker_options(parser)
    flags = parser.parse_args(argv)
    if (flags.est is None) == (flags.baseline is None):
        parser.error("one of --est and --baseline is needed")
    try:
        flags.thr = tuple(int(t) for t in flags.thr.split(",")) if flags.thr else ()
    except ValueError:
        parser.error("--thr: integers, comma separated")
    if len(flags.thr) > pipeline.MSCORE_MAX_THR or any(not 1 <= t <= 255 for t in flags.thr):
        parser.error("--thr: at most %d thresholds, each 1..255" % pipeline.MSCORE_MAX_THR)
    if flags.radius is not None and not 0 <= flags.radius <= pipeline.SEG_MAX_RADIUS:
        parser.error("--radius: 0..%d" % pipeline.SEG_MAX_RADIUS)
    score_cli.check_driver(parser, flags, "an `lscore` or `mscore` line")
    return flags


if __name__ == "__main__":
    main(parse())
