#!/usr/bin/env python3
"""Score estimated flows against a generated dataset (DESIGN.md "Flow scoring").

    score_gen.py --data OUT --est EST_ROOT [--full] [--gpu 0 1 ..] [--arap_bin CMD] [--worker auto|serve|batch]

OUT is a tree para_gen.py wrote.  Every pair of OUT/all_files.list (without the list: every .flo under the ground-truth
directory) is scored against EST_ROOT/<seq>/<frame>.flo by one `score` line of arap_deform (pipeline.ScoreLine) on
para_gen.py's workers, one persistent `arap_deform --serve` per GPU:

  default   the ground truth is OUT/Flow, defined on the objects only: mask=OUT/inpMasks leaves every other pixel out;
            occ=OUT/Occ
  --full    the ground truth is OUT/FlowFull, defined everywhere: no mask; occ=OUT/OccFull

and in both dist=OUT/MBDist and skip=OUT/Fold; each plane only where its file exists.  Written: OUT/Score/<seq>/<frame>.txt
per pair (pipeline.format_score), their exact pooled table OUT/score.txt (pipeline.add_scores), and
OUT/score_missing.list, the ground-truth files without an estimate, which are counted and no error.  Prints the summary
(pipeline.score_summary).  Separate from para_gen.py because an estimate can only exist once the dataset does.
"""
import argparse
import os
import os.path as osp
import sys

HERE = osp.dirname(osp.abspath(__file__))
sys.path.insert(0, HERE)
import score_cli                            # noqa: E402
from arap_flow_amd import pipeline          # noqa: E402


def ground_truth(data, full):
    """[(seq, frame stem, flow file)] of the pairs to score"""
    gt_dir = osp.join(data, "FlowFull" if full else "Flow")
    lst = osp.join(data, "all_files.list")
    if osp.exists(lst):
        tail = lambda flow: flow.rsplit(osp.sep + "Flow" + osp.sep, 1)[-1]            # <seq>/<frame>.flo, wherever the tree was written
        flows = [osp.join(gt_dir, tail(ln.split(" ")[2])) for ln in open(lst).read().splitlines() if ln.strip()]
    else:
        flows = sorted(osp.join(d, f) for d, _, fs in os.walk(gt_dir) for f in fs if f.endswith(".flo"))
    return [(osp.relpath(osp.dirname(f), gt_dir), osp.basename(f)[:-4], f) for f in flows if osp.exists(f)]


def score_items(data, est_root, full):
    """-> ([ScoreLine], [ground-truth files without an estimate])"""
    items, missing = [], []
    for seq, stem, gt in ground_truth(data, full):
        est = osp.join(est_root, seq, stem + ".flo")
        if not osp.exists(est):
            missing.append(gt)
            continue
        named = lambda d: osp.join(data, d, seq, stem + ".png")
        planes = dict(occ=named("OccFull" if full else "Occ"), dist=named("MBDist"), skip=named("Fold"))
        if not full:
            planes["mask"] = named("inpMasks")
        out = osp.join(data, "Score", seq, stem + ".txt")
        os.makedirs(osp.dirname(out), exist_ok=True)
        items.append(pipeline.ScoreLine(gt, est, {k: p for k, p in planes.items() if osp.exists(p)}, out))
    return items, missing


def summary_text(table):
    s = pipeline.score_summary(table)
    text = "%-9s %10s %9s %7s %7s %7s %7s\n" % ("class", "pixels", "EPE", "R1 %", "R3 %", "R5 %", "Fl %")
    for name in pipeline.SCORE_ROWS[:-1]:
        r = s[name]
        text += "%-9s %10d %9.4f %7.2f %7.2f %7.2f %7.2f\n" % (name, r["count"], r["epe"], 100 * r["r1"], 100 * r["r3"], 100 * r["r5"], 100 * r["fl"])
    left = s[pipeline.SCORE_ROWS[-1]]
    return text + "left out: %d skipped, %d without a finite ground truth\n" % (left["skipped"], left["gt_nonfinite"])


def main(flags):
    data = osp.abspath(flags.data)
    items, missing = score_items(data, osp.abspath(flags.est), flags.full)
    score_cli.run_lines(flags, items)
    pooled = pipeline.add_scores([pipeline.parse_score_file(open(it.out).read()) for it in items])
    score_cli.write_results(data, "score", pipeline.format_score(pooled), missing)
    print("%d pairs scored, %d without an estimate" % (len(items), len(missing)))
    print(summary_text(pooled), end="")
    return pooled


def parse(argv=None):
    parser = argparse.ArgumentParser(description="Error tables of estimated flows against a para_gen.py dataset")
    parser.add_argument("--data", required=True, help="the dataset: para_gen.py's --output")
    parser.add_argument("--est", required=True, help="the estimates: EST/<seq>/<frame>.flo, named like the dataset's flow files")
    parser.add_argument("--full", action="store_true", help="score against FlowFull / OccFull, every pixel, instead of Flow on the objects")
    score_cli.add_worker_options(parser)
    flags = parser.parse_args(argv)
    score_cli.check_driver(parser, flags, "a `score` line")
    return flags


if __name__ == "__main__":
    main(parse())
