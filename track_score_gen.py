#!/usr/bin/env python3
"""Score estimated point tracks against a generated dataset (DESIGN.md "Track scoring").

    track_score_gen.py --data OUT --est EST_ROOT [--from_flows] [--tapvid] [--gpu 0 1 ..] [--narap N] [--arap_bin CMD]
                       [--worker auto|serve|batch]

OUT is a tree para_gen.py wrote with --tracks.  Every track file OUT/Tracks/<seq>/<frame>.trk is scored by one `tscore`
line of arap_deform (pipeline.TScoreLine) on para_gen.py's workers, one persistent `arap_deform --serve` per GPU:

  default       against EST_ROOT/<seq>/<frame>.trk, a tracker's output in the track file format
  --from_flows  against the chain of the per-link flow estimates EST_ROOT/<seq>/<frame>_l<j>.flo, j = 0 .. F-2 (link j
                from sequence frame j to j + 1), from the file's own query points: one `chain` line (pipeline.ChainLine)
                writes OUT/TracksEst/<seq>/<frame>.trk first; where <frame>_b<j>.flo (link j back) exists for every j they
                are its bwd=, the forward-backward check of the visibility
  --tapvid      the error is taken on the benchmark's 256 x 256 raster: s = float32(256) / float32(W), float32(256) / float32(H)

Written: OUT/TrackScore/<seq>/<frame>.txt per file (pipeline.format_track_score), their exact pooled table
OUT/track_score.txt (pipeline.add_track_scores) and OUT/track_score_missing.list, the track files without an estimate,
which are counted and no error.  Prints the summary (pipeline.track_score_summary): per class, then the `all` class per
frame index, the drift curve.  The pooled numbers are over all points together, not TAP-Vid's mean over videos.
"""
import argparse
import os
import os.path as osp
import struct
import sys

import numpy as np

HERE = osp.dirname(osp.abspath(__file__))
sys.path.insert(0, HERE)
import score_cli                            # noqa: E402
from arap_flow_amd import pipeline          # noqa: E402


def ground_truth(data):
    """[(seq, frame stem, track file)] of the track files to score"""
    gt_dir = osp.join(data, "Tracks")
    files = sorted(osp.join(d, f) for d, _, fs in os.walk(gt_dir) for f in fs if f.endswith(".trk"))
    return [(osp.relpath(osp.dirname(f), gt_dir), osp.basename(f)[:-4], f) for f in files]


def trk_header(path):
    """(W, H, F, P) of a track file"""
    with open(path, "rb") as f:
        head = f.read(24)
    if len(head) != 24 or head[:4] != b"ATRK":
        raise ValueError("%s: not a track file" % path)
    return struct.unpack("<5i", head[4:])[1:]


def score_items(data, est_root, from_flows, tapvid):
    """-> ([(ChainLine or None, TScoreLine)], [track files without an estimate])"""
    items, missing = [], []
    for seq, stem, gt in ground_truth(data):
        W, H, F, _ = trk_header(gt)
        chain = None
        if from_flows:
            named = lambda tag: [osp.join(est_root, seq, "%s_%s%d.flo" % (stem, tag, j)) for j in range(F - 1)]
            fwd, bwd = named("l"), named("b")
            if F < 2 or not all(osp.exists(p) for p in fwd):
                missing.append(gt)
                continue
            est = osp.join(data, "TracksEst", seq, stem + ".trk")
            os.makedirs(osp.dirname(est), exist_ok=True)
            chain = pipeline.ChainLine(gt, tuple(fwd), tuple(bwd) if all(osp.exists(p) for p in bwd) else (), est)
        else:
            est = osp.join(est_root, seq, stem + ".trk")
            if not osp.exists(est):
                missing.append(gt)
                continue
        scale = (float(np.float32(256) / np.float32(W)), float(np.float32(256) / np.float32(H))) if tapvid else (1.0, 1.0)
        out = osp.join(data, "TrackScore", seq, stem + ".txt")
        os.makedirs(osp.dirname(out), exist_ok=True)
        items.append((chain, pipeline.TScoreLine(gt, est, scale, out)))
    return items, missing


def summary_text(table):
    s = pipeline.track_score_summary(table)
    pct = lambda v: 100 * v
    head = "%-10s %10s %10s %7s %7s %7s" + " %7s" * 5 + " %9s\n"
    row = "%-10s %10d %10d %7.2f %7.2f %7.2f" + " %7.2f" * 5 + " %9.4f\n"
    cols = ("point-fr.", "visible", "OA %", "d_avg %", "AJ %") + tuple("d_%d %%" % x for x in pipeline.TSCORE_X) + ("err px",)
    numbers = lambda r: (r["count"], r["gt_vis"], pct(r["oa"]), pct(r["d_avg"]), pct(r["aj"])) + \
        tuple(pct(r["d_%d" % x]) for x in pipeline.TSCORE_X) + (r["err"],)
    text = "%d query points, %d invalid\n" % (s["valid"], s["invalid"])
    text += head % (("class",) + cols)
    for name in pipeline.TSCORE_CLASSES:
        text += row % ((name,) + numbers(s[name]))
    text += head % (("frame",) + cols)
    for f, r in enumerate(s["frames"], 1):
        text += row % ((str(f),) + numbers(r))
    return text


def main(flags):
    data = osp.abspath(flags.data)
    items, missing = score_items(data, osp.abspath(flags.est), flags.from_flows, flags.tapvid)
    # a chain's track file -> the line that scores it
    score_cli.run_lines(flags, [chain or ts for chain, ts in items], {chain.out: [ts] for chain, ts in items if chain is not None})
    tables = [pipeline.parse_track_score_file(open(ts.out).read()) for _, ts in items]
    pooled = pipeline.add_track_scores(tables) if tables else \
        np.zeros((2, len(pipeline.TSCORE_CLASSES), len(pipeline.TSCORE_FIELDS)), np.uint64)
    score_cli.write_results(data, "track_score", pipeline.format_track_score(pooled), missing)
    print("%d track files scored, %d without an estimate" % (len(items), len(missing)))
    print(summary_text(pooled), end="")
    return pooled


def parse(argv=None):
    parser = argparse.ArgumentParser(description="TAP-Vid tables of estimated tracks against a para_gen.py dataset")
    parser.add_argument("--data", required=True, help="the dataset: para_gen.py's --output, written with --tracks")
    parser.add_argument("--est", required=True, help="the estimates: EST/<seq>/<frame>.trk, or with --from_flows EST/<seq>/<frame>_l<j>.flo")
    parser.add_argument("--from_flows", action="store_true", help="chain per-link flow estimates into OUT/TracksEst first")
    parser.add_argument("--tapvid", action="store_true", help="take the error on the benchmark's 256 x 256 raster")
    score_cli.add_worker_options(parser)
    flags = parser.parse_args(argv)
    score_cli.check_driver(parser, flags, "a `tscore` line")
    return flags


if __name__ == "__main__":
    main(parse())
