"""GPU: the `lscore` and `mscore` list lines through both arap_deform twins (list file and --serve) and map_score_gen.py
(child processes), against the numpy twin tests/mscore_ref.py on the files those runs read."""
import os
import os.path as osp
import shutil
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import mscore_ref
from arap_flow_amd import build, pipeline, synth

pytestmark = pytest.mark.gpu
ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))


def _env():
    return dict(os.environ, HIP_VISIBLE_DEVICES=os.environ.get("HIP_VISIBLE_DEVICES", "0"))


def _run(args, cwd, stdin=None):
    r = subprocess.run(args, cwd=cwd, env=_env(), capture_output=True, text=True, timeout=600, input=stdin)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _twin_text(item):
    """the twin's file on what the line reads"""
    red = pipeline.load_mask_red
    skip = red(item.skip) if item.skip else None
    if isinstance(item, pipeline.LScoreLine):
        return mscore_ref.label_text(red(item.gt), red(item.est), item.L, item.radius, skip)
    return mscore_ref.map_text(red(item.gt), red(item.est), skip, item.thr, item.radius or 0)


def test_lines_all_three_hosts_equal_the_twin_on_a_solved_frame(tmp_path):
    """a frame of two segments: its two solve lines, its layers line (the forward occlusion) and its seg line (index and
    motion-boundary maps of both frames) in one list through the C++ worker, then six score lines over those maps through
    the C++ worker on a list, through --serve and through arap_deform.py: the same bytes, the twin's"""
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
                                 p("wm%d.png" % s), extra={}) for s, _ in segs]
    layers = [(ln.mask, ln.flow) for ln in solves]
    seg = pipeline.SegLine(layers, 1.0, 16, (), {k: p(k + ".png") for k in ("idx1", "idx2", "mb1", "mb2")})
    made = [pipeline.format_line(ln) for ln in solves] + [pipeline.layers_line(pipeline.LayersLine(p("r.png"), layers, dict(occ=p("occ.png")))),
                                                          pipeline.format_line(seg)]
    (tmp_path / "make.txt").write_text("\n".join(made) + "\n")
    _run([cpp, p("make.txt")], str(tmp_path))
    idx1, idx2 = pipeline.load_mask_red(p("idx1.png")), pipeline.load_mask_red(p("idx2.png"))
    assert set(np.unique(idx1)) == {0, 1, 2} and (idx1 != idx2).any() and pipeline.load_mask_red(p("occ.png")).any()
    Image.fromarray((np.random.default_rng(3).random((H, W)) < 0.1).astype(np.uint8) * 255, "L").save(p("skip.png"))

    def items(tag):
        out = lambda k: p("%s_%d.txt" % (tag, k))
        return [pipeline.LScoreLine(p("idx2.png"), p("idx1.png"), 2, 2, None, out(0)),            # nothing moved, as the estimate
                pipeline.LScoreLine(p("idx1.png"), p("idx2.png"), 1, 0, p("skip.png"), out(1)),    # label 2 above L
                pipeline.LScoreLine(p("idx1.png"), p("idx1.png"), 255, 254, None, out(2)),
                pipeline.MScoreLine(p("occ.png"), p("mb1.png"), (), None, None, out(3)),
                pipeline.MScoreLine(p("mb2.png"), p("mb1.png"), (1, 255), 3, p("skip.png"), out(4)),
                pipeline.MScoreLine(p("mb1.png"), p("idx1.png"), (1, 2, 3), 0, None, out(5))]
    lines = lambda tag: "".join(pipeline.format_line(it) + "\n" for it in items(tag))
    (tmp_path / "cpp.txt").write_text(lines("cpp"))
    _run([cpp, p("cpp.txt")], str(tmp_path))
    out = _run([cpp, "--serve"], str(tmp_path), stdin=lines("srv"))
    assert [("Done " + it.out) in out.splitlines() for it in items("srv")] == [True] * 6
    (tmp_path / "py.txt").write_text(lines("py"))
    _run([sys.executable, osp.join(ROOT, "arap_deform.py"), p("py.txt")], str(tmp_path))
    for k, it in enumerate(items("x")):
        text = _twin_text(it)
        for tag in ("cpp", "srv", "py"):
            assert open(p("%s_%d.txt" % (tag, k))).read() == text, (tag, k)
    t = pipeline.parse_label_score_file(open(p("cpp_0.txt")).read())
    s = pipeline.label_score_summary(t)
    assert t.shape == (3, 8) and (t[1:, :7] > 0).all() and 0 < s["J"] < 1 and 0 < s["F"] <= 1
    assert pipeline.parse_label_score_file(open(p("cpp_1.txt")).read())[0, [1, 3]].min() > 0       # skipped pixels; a label above L
    assert pipeline.label_score_summary(pipeline.parse_label_score_file(open(p("cpp_2.txt")).read()))["JF"] == 1.0
    m = pipeline.parse_map_score_file(open(p("cpp_4.txt")).read())
    assert m["thr"] == (1, 255) and (m["match"] > 0).all() and np.array_equal(m["match"][0], m["match"][1])     # a 0 / 255 map
    # sizes that differ are an error of that line, at run time
    Image.fromarray(idx1[:-1], "L").save(p("small.png"))
    for k, bad in enumerate((pipeline.LScoreLine(p("idx1.png"), p("small.png"), 2, 2, None, p("bad_out.txt")),
                             pipeline.MScoreLine(p("mb1.png"), p("mb2.png"), (), None, p("small.png"), p("bad_out.txt")))):
        (tmp_path / ("bad%d.txt" % k)).write_text(pipeline.format_line(bad) + "\n")
        assert subprocess.run([cpp, p("bad%d.txt" % k)], cwd=str(tmp_path), env=_env(), capture_output=True).returncode == 1
        assert subprocess.run([sys.executable, osp.join(ROOT, "arap_deform.py"), p("bad%d.txt" % k)], cwd=str(tmp_path), env=_env(),
                              capture_output=True).returncode != 0
    assert not osp.exists(p("bad_out.txt"))


def test_map_score_gen_over_a_generated_tree(tmp_path):
    """para_gen.py --seg --occ --bwd_flow writes a two-pair tree; its own maps as the estimate are the ceiling, Index1 as
    the estimate of Index2 the floor, and an estimate that is not there is listed and counted"""
    W, H = 96, 64
    inp, mdir = tmp_path / "in", tmp_path / "matches"
    os.makedirs(inp / "orgRGB" / "a"); os.makedirs(inp / "orgMasks" / "a"); os.makedirs(mdir / "a")
    fr = synth.make_frame(W, H, seed=98, K=2, fd=1)
    for n in range(3):                                                      # three frames: two pairs
        Image.fromarray(fr["rgb"]).save(inp / "orgRGB" / "a" / ("%05d.png" % n))
        Image.fromarray(fr["labels"].astype(np.uint8)).save(inp / "orgMasks" / "a" / ("%05d.png" % n))
        (mdir / "a" / ("%05d.txt" % n)).write_text("\n".join("%d %d %d %d 1.0 0" % tuple(c) for c in fr["constraints"]))
    outp = tmp_path / "out"
    _run([sys.executable, osp.join(ROOT, "para_gen.py"), "--input", str(inp), "--output", str(outp), "--gpu", "0", "--fd", "1",
          "--matches", str(mdir), "--jobs", "2", "--seg", "1", "24", "--occ", "--bwd_flow"], str(tmp_path))
    dirs = ("Occ", "OccBwd", "MB", "MBBwd", "Index1", "Index2")
    assert all(sorted(os.listdir(outp / d / "a")) == ["00000.png", "00001.png"] for d in dirs)
    gen = [sys.executable, osp.join(ROOT, "map_score_gen.py"), "--data", str(outp)]

    def pooled():
        text = open(outp / "map_score.txt").read()
        parts = {blk.split("]\n", 1)[0]: blk.split("]\n", 1)[1] for blk in text.split("[")[1:]}
        return {d: pipeline.parse_label_score_file(t) if d.startswith("Index") else pipeline.parse_map_score_file(t) for d, t in parts.items()}

    printed = _run(gen + ["--est", str(outp)], str(tmp_path))                # the ceiling
    assert "12 maps scored, 0 without an estimate" in printed and open(outp / "map_score_missing.list").read() == ""
    got = pooled()
    assert sorted(got) == sorted(dirs)
    for d in dirs:
        if d.startswith("Index"):
            s = pipeline.label_score_summary(got[d])
            assert s["J"] == s["F"] == s["JF"] == 1.0 and int(got[d][0, 0]) == 2 * W * H
        else:
            s = pipeline.map_score_summary(got[d])
            assert s["ap"] == s["best_f"] == s["f128"] == 1.0 and s["pos"] > 0
            assert all(v == dict(P=1.0, R=1.0, F=1.0) for v in s["match"].values()) and (sorted(s["match"]) == [64, 128, 192]) == d.startswith("MB")
    line = pipeline.LScoreLine(str(outp / "Index2" / "a" / "00001.png"), str(outp / "Index2" / "a" / "00001.png"), 1, 1, None, "x")
    assert open(outp / "MapScore" / "Index2" / "a" / "00001.txt").read() == _twin_text(line)       # ceil(0.008 * sqrt(96^2 + 64^2)) = 1
    shutil.rmtree(outp / "MapScore")

    printed = _run(gen + ["--baseline", "still"], str(tmp_path))            # the floor
    assert "2 maps scored, 0 without an estimate" in printed
    got = pooled()
    s = pipeline.label_score_summary(got["Index2"])
    assert list(got) == ["Index2"] and 0 < s["J"] < 1 and s["F"] < 1
    assert sorted(os.listdir(outp / "MapScore")) == ["Index2"]

    est = tmp_path / "est"                                                  # an estimate that is not there
    for d in dirs:
        shutil.copytree(outp / d, est / d)
    os.remove(est / "MB" / "a" / "00001.png")
    printed = _run(gen + ["--est", str(est), "--radius", "2", "--thr", "128"], str(tmp_path))
    assert "11 maps scored, 1 without an estimate" in printed
    assert open(outp / "map_score_missing.list").read() == str(outp / "MB" / "a" / "00001.png") + "\n"
    assert pooled()["MB"]["thr"] == (128,) and not osp.exists(outp / "MapScore" / "MB" / "a" / "00001.txt")
