"""GPU: the `score` list line through both arap_deform twins (list file and --serve) and score_gen.py (child processes),
against the numpy twin tests/score_ref.py on the files those runs read."""
import os
import os.path as osp
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import score_ref
from arap_flow_amd import build, flo, pipeline, synth

pytestmark = pytest.mark.gpu
ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
F = np.float32


def _env():
    return dict(os.environ, HIP_VISIBLE_DEVICES=os.environ.get("HIP_VISIBLE_DEVICES", "0"))


def _run(args, cwd, stdin=None):
    r = subprocess.run(args, cwd=cwd, env=_env(), capture_output=True, text=True, timeout=600, input=stdin)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _twin_text(gt, est, occ=None, dist=None, skip=None, mask=None):
    """format_score of the twin's table on what a score line reads from these files"""
    red = pipeline.load_mask_red
    left = None
    if skip or mask:
        left = sum((red(p) != 0).astype(np.uint8) for p in (skip, mask) if p)
    t = score_ref.score_ref(flo.flow_read(gt), flo.flow_read(est), occ=red(occ) if occ else None,
                            dist=pipeline.dist_from_png(red(dist)) if dist else None, skip=left)["table"][0]
    return pipeline.format_score(t), t


def test_solve_seg_and_score_lines_all_three_hosts_equal_the_twin(tmp_path):
    """a frame of two segments through the C++ worker: its solve lines, the frame's layers and seg lines for the flow, the
    occlusion and the distance file, then score lines on a perturbed flow: list mode, --serve and arap_deform.py write
    the same bytes, the twin's"""
    W, H = 96, 64
    fr = synth.make_frame(W, H, seed=98, K=2, fd=1)
    p = lambda n: str(tmp_path / n)
    Image.fromarray(fr["rgb"]).save(p("r.png"))
    segs = pipeline.split_segments(fr["labels"].astype(np.uint8), [int(fr["labels"][c[1], c[0]]) for c in fr["constraints"]])
    assert len(segs) == 2
    for s, mask in segs:
        Image.fromarray(mask).save(p("m%d.png" % s))
        pipeline.write_constraints(p("c%d.txt" % s), [tuple(c) for c in fr["constraints"] if fr["labels"][c[1], c[0]] == s])
    cpp = build.build_host()[0]
    solves = [pipeline.SolveLine(p("r.png"), p("m%d.png" % s), p("c%d.txt" % s), p("f%d.flo" % s), p("w%d.png" % s),
                                 p("wm%d.png" % s), extra=dict(fold=p("fold%d.png" % s))) for s, _ in segs]
    layers = [(ln.mask, ln.flow) for ln in solves]
    seg = pipeline.SegLine(layers, 1.0, 140, (), dict(dist1=p("dist.png")))
    lay = pipeline.LayersLine(p("r.png"), layers, dict(occ=p("occ.png")))
    (tmp_path / "gen.txt").write_text("\n".join(pipeline.format_line(x) for x in solves + [lay, seg]) + "\n")
    _run([cpp, p("gen.txt")], str(tmp_path))
    # the ground truth: segment 0's flow; the "estimate": that flow perturbed, with a few outliers and a hole
    gt = flo.flow_read(solves[0].flow)
    rng = np.random.default_rng(5)
    est = (gt + rng.normal(size=gt.shape) * rng.choice([0.2, 1.0, 4.0], size=gt.shape[:2] + (1,))).astype(F)
    ys, xs = np.nonzero(pipeline.load_mask_red(solves[0].mask) == 0)           # on the object: a hole and an outlier
    est[ys[:12], xs[:12]] = np.nan
    est[ys[-1], xs[-1]] = (1e6, -1e6)
    flo.flow_write(p("est.flo"), est)
    planes = dict(occ=p("occ.png"), dist=p("dist.png"), skip=solves[0].extra["fold"], mask=solves[0].mask)
    variants = [dict(planes), {}, dict(mask=planes["mask"]), dict(dist=planes["dist"], skip=planes["skip"])]
    item = lambda tag, k: pipeline.ScoreLine(solves[0].flow, p("est.flo"), variants[k], p("%s_%d.txt" % (tag, k)))
    (tmp_path / "cpp.txt").write_text("".join(pipeline.format_line(item("cpp", k)) + "\n" for k in range(len(variants))))
    _run([cpp, p("cpp.txt")], str(tmp_path))
    out = _run([cpp, "--serve"], str(tmp_path), stdin="".join(pipeline.format_line(item("srv", k)) + "\n" for k in range(len(variants))))
    assert ["Done " + p("srv_%d.txt" % k) in out.splitlines() for k in range(len(variants))] == [True] * len(variants)
    (tmp_path / "py.txt").write_text("".join(pipeline.format_line(item("py", k)) + "\n" for k in range(len(variants))))
    _run([sys.executable, osp.join(ROOT, "arap_deform.py"), p("py.txt")], str(tmp_path))
    for k, v in enumerate(variants):
        text, t = _twin_text(solves[0].flow, p("est.flo"), **v)
        for tag in ("cpp", "srv", "py"):
            assert open(p("%s_%d.txt" % (tag, k))).read() == text, (tag, k)
        assert np.array_equal(pipeline.parse_score_file(text), t)
        if k == 0:                                              # the scene exercises the planes it is given
            assert t[0, 0] > 500 and t[9, 0] > 500 and t[1, 0] > 0 and t[3, 0] > 0 and t[4, 0] > 0 and t[0, 6] == 12
    # sizes that differ are an error of that line, at run time
    flo.flow_write(p("small.flo"), est[:-1])
    (tmp_path / "bad.txt").write_text(pipeline.format_line(pipeline.ScoreLine(solves[0].flow, p("small.flo"), {}, p("bad_out.txt"))) + "\n")
    assert subprocess.run([cpp, p("bad.txt")], cwd=str(tmp_path), env=_env(), capture_output=True).returncode == 1
    assert subprocess.run([sys.executable, osp.join(ROOT, "arap_deform.py"), p("bad.txt")], cwd=str(tmp_path), env=_env(),
                          capture_output=True).returncode != 0
    assert not osp.exists(p("bad_out.txt"))


@pytest.mark.parametrize("full", [False, True], ids=["objects", "full"])
def test_score_gen_over_a_generated_tree(tmp_path, full):
    """para_gen.py writes a two-pair tree with every map a score line can read; score_gen.py scores both pairs, pools the
    two files, and names a third listed pair, which has no estimate"""
    W, H = 96, 64
    inp, mdir, bgd = tmp_path / "in", tmp_path / "matches", tmp_path / "bgs"
    os.makedirs(inp / "orgRGB" / "a"); os.makedirs(inp / "orgMasks" / "a"); os.makedirs(mdir / "a"); os.makedirs(bgd)
    fr = synth.make_frame(W, H, seed=98, K=2, fd=1)
    for n in range(3):                                          # three frames: two pairs
        Image.fromarray(fr["rgb"]).save(inp / "orgRGB" / "a" / ("%05d.png" % n))
        Image.fromarray(fr["labels"].astype(np.uint8)).save(inp / "orgMasks" / "a" / ("%05d.png" % n))
        (mdir / "a" / ("%05d.txt" % n)).write_text("\n".join("%d %d %d %d 1.0 0" % tuple(c) for c in fr["constraints"]))
    Image.fromarray(np.random.default_rng(1).integers(0, 256, (140, 220, 3)).astype(np.uint8)).save(bgd / "one.png")
    outp, est = tmp_path / "out", tmp_path / "est"
    _run([sys.executable, osp.join(ROOT, "para_gen.py"), "--input", str(inp), "--output", str(outp), "--gpu", "0", "--fd", "1",
          "--matches", str(mdir), "--jobs", "2", "--occ", "--diag", "--seg", "1", "140"] +
         (["--bg_dir", str(bgd), "--bg_motion"] if full else []), str(tmp_path))
    pairs = open(outp / "all_files.list").read().splitlines()
    assert len(pairs) == 2
    gt_dir = "FlowFull" if full else "Flow"
    gts = [str(outp / gt_dir / "a" / ("%05d.flo" % k)) for k in range(2)]
    assert all(osp.exists(g) for g in gts)
    rng = np.random.default_rng(9)
    os.makedirs(est / "a")
    for k in range(2):
        gt = flo.flow_read(gts[k])
        flo.flow_write(str(est / "a" / ("%05d.flo" % k)), (gt + rng.normal(size=gt.shape) * (k + 1)).astype(F))
    # a third pair on the tree's list, a copy of pair 1, without an estimate
    with open(outp / "all_files.list", "a") as f:
        f.write("\n" + pairs[1].replace("00001", "00007") + "\n")
    flo.flow_write(str(outp / gt_dir / "a" / "00007.flo"), flo.flow_read(gts[1]))
    printed = _run([sys.executable, osp.join(ROOT, "score_gen.py"), "--data", str(outp), "--est", str(est)] + (["--full"] if full else []),
                   str(tmp_path))
    assert "2 pairs scored, 1 without an estimate" in printed
    named = lambda d, k: str(outp / d / "a" / ("%05d.png" % k))
    tables = []
    for k in range(2):
        planes = dict(occ=named("OccFull" if full else "Occ", k), dist=named("MBDist", k), skip=named("Fold", k))
        if not full:
            planes["mask"] = named("inpMasks", k)
        assert all(osp.exists(q) for q in planes.values()), planes
        text, t = _twin_text(gts[k], str(est / "a" / ("%05d.flo" % k)), **planes)
        assert open(outp / "Score" / "a" / ("%05d.txt" % k)).read() == text, k
        tables.append(t)
    pooled = pipeline.add_scores(tables)
    assert open(outp / "score.txt").read() == pipeline.format_score(pooled)
    assert open(outp / "score_missing.list").read() == str(outp / gt_dir / "a" / "00007.flo") + "\n"
    assert pooled[0, 0] > 0 and pooled[1, 0] > 0 and pooled[3:6, 0].sum() > 0 and (full or pooled[9, 0] > 0)
