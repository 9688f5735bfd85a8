"""GPU: the `fscore` list line through both arap_deform twins (list file and --serve) and frame_score_gen.py (child
processes), against the numpy twin tests/fscore_ref.py on the files those runs read."""
import os
import os.path as osp
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import fscore_ref
from arap_flow_amd import build, pipeline

pytestmark = pytest.mark.gpu
ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
ONE = fscore_ref.ONE


def _env():
    return dict(os.environ, HIP_VISIBLE_DEVICES=os.environ.get("HIP_VISIBLE_DEVICES", "0"))


def _run(args, cwd, stdin=None):
    r = subprocess.run(args, cwd=cwd, env=_env(), capture_output=True, text=True, timeout=600, input=stdin)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _twin_text(ref, est, **planes):
    """format_frame_score of the twin's table on what an fscore line reads from these files"""
    red = {k: pipeline.load_mask_red(p) for k, p in planes.items()}
    if "dist" in red:
        red["dist"] = pipeline.dist_from_png(red["dist"])
    t = fscore_ref.fscore_ref(pipeline.load_rgb(ref), pipeline.load_rgb(est), **red)["table"][0]
    return pipeline.format_frame_score(t), t


def _scene(W, H, shift, rng):
    """a textured square on a textured ground, the square `shift` pixels to the right"""
    ground = rng.integers(0, 256, (H, W, 3)).astype(np.uint8) // 4
    img = ground.copy()
    img[10:30, 8 + shift:28 + shift] = 128 + ground[10:30, 8:28]
    return img


def test_fscore_lines_all_three_hosts_equal_the_twin(tmp_path):
    """the same four lines, with all planes, none and two subsets, through the C++ worker on a list, through --serve and
    through arap_deform.py: the same bytes, the twin's"""
    W, H = 75, 41
    rng = np.random.default_rng(11)
    p = lambda n: str(tmp_path / n)
    ref = _scene(W, H, 6, rng)
    est = np.clip(ref.astype(int) + rng.integers(-9, 10, ref.shape) * (rng.random((H, W, 1)) < 0.5), 0, 255).astype(np.uint8)
    Image.fromarray(ref).save(p("ref.png"))
    Image.fromarray(est).save(p("est.png"))
    Image.fromarray(rng.choice(np.array([0, 0, 1, 255], np.uint8), size=(H, W)), "L").save(p("occ.png"))
    Image.fromarray(rng.choice(np.array([0, 9, 10, 59, 60, 139, 140, 255], np.uint8), size=(H, W)), "L").save(p("dist.png"))
    Image.fromarray((rng.random((H, W)) < 0.1).astype(np.uint8) * 255, "L").save(p("skip.png"))
    obj = np.full((H, W, 3), 255, np.uint8)
    obj[10:30, 14:34] = 0                                           # the solver's convention: red 0 is the object
    Image.fromarray(obj).save(p("obj.png"))
    planes = dict(occ=p("occ.png"), dist=p("dist.png"), skip=p("skip.png"), obj=p("obj.png"))
    variants = [dict(planes), {}, dict(obj=planes["obj"]), dict(dist=planes["dist"], skip=planes["skip"])]
    item = lambda tag, k: pipeline.FScoreLine(p("ref.png"), p("est.png"), variants[k], p("%s_%d.txt" % (tag, k)))
    lines = lambda tag: "".join(pipeline.format_line(item(tag, k)) + "\n" for k in range(len(variants)))
    cpp = build.build_host()[0]
    (tmp_path / "cpp.txt").write_text(lines("cpp"))
    _run([cpp, p("cpp.txt")], str(tmp_path))
    out = _run([cpp, "--serve"], str(tmp_path), stdin=lines("srv"))
    assert ["Done " + p("srv_%d.txt" % k) in out.splitlines() for k in range(len(variants))] == [True] * len(variants)
    (tmp_path / "py.txt").write_text(lines("py"))
    _run([sys.executable, osp.join(ROOT, "arap_deform.py"), p("py.txt")], str(tmp_path))
    for k, v in enumerate(variants):
        text, t = _twin_text(p("ref.png"), p("est.png"), **v)
        for tag in ("cpp", "srv", "py"):
            assert open(p("%s_%d.txt" % (tag, k))).read() == text, (tag, k)
        assert np.array_equal(pipeline.parse_frame_score_file(text), t)
        if k == 0:                                              # the scene exercises the planes it is given
            assert (t[:8, 0] > 0).all() and (t[:8, 4] > 0).all() and (t[8, :2] > 0).all() and t[0, 1] > 0 and t[0, 6] > 0
    # sizes that differ are an error of that line, at run time
    Image.fromarray(est[:-1]).save(p("small.png"))
    (tmp_path / "bad.txt").write_text(pipeline.format_line(pipeline.FScoreLine(p("ref.png"), p("small.png"), {}, p("bad_out.txt"))) + "\n")
    assert subprocess.run([cpp, p("bad.txt")], cwd=str(tmp_path), env=_env(), capture_output=True).returncode == 1
    assert subprocess.run([sys.executable, osp.join(ROOT, "arap_deform.py"), p("bad.txt")], cwd=str(tmp_path), env=_env(),
                          capture_output=True).returncode != 0
    assert not osp.exists(p("bad_out.txt"))


def _tree(out, full):
    """a dataset tree with one pair of sequence `a`: the end frames, two in-between frames with their link occlusions,
    and -- without `full` -- the planes of frame 2"""
    W, H = 72, 40
    rng = np.random.default_rng(12)
    mid = "MidFull" if full else "Mid"
    for d in ("inpRGB", "wRGB", mid, "OccBwd", "MBDistBwd", "Occ"):
        os.makedirs(out / d / "a")
    seed = rng.integers(1 << 30)
    frame = lambda shift: _scene(W, H, shift, np.random.default_rng(seed))          # one texture, the square moving
    Image.fromarray(frame(0)).save(out / "inpRGB" / "a" / "00000.png")
    Image.fromarray(frame(12)).save(out / "wRGB" / "a" / "00000.png")
    for step, shift in ((4, 3), (9, 7)):
        Image.fromarray(frame(shift)).save(out / mid / "a" / ("00000_s%02d.png" % step))
        Image.fromarray((rng.random((H, W)) < 0.2).astype(np.uint8) * 255, "L").save(out / mid / "a" / ("00000_s%02d_occ.png" % step))
        Image.fromarray(np.zeros((H, W), np.uint8), "L").save(out / mid / "a" / ("00000_s%02d_mask.png" % step))     # no frame, no plane
    Image.fromarray((rng.random((H, W)) < 0.2).astype(np.uint8) * 255, "L").save(out / "OccBwd" / "a" / "00000.png")
    Image.fromarray(rng.integers(0, 256, (H, W)).astype(np.uint8), "L").save(out / "MBDistBwd" / "a" / "00000.png")
    Image.fromarray(np.full((H, W), 255, np.uint8), "L").save(out / "Occ" / "a" / "00000.png")          # frame 1's grid: never passed


@pytest.mark.parametrize("full", [False, True], ids=["objects", "full"])
def test_frame_score_gen_on_a_tiny_tree(tmp_path, full):
    """the ground truth as its own estimate is exact on every row; the blend of the end frames is strictly worse, and the
    frame 2 it has no estimate for is listed and counted; the pooled file is the per-frame files pooled"""
    out = tmp_path / "out"
    _tree(out, full)
    mid = "MidFull" if full else "Mid"
    names = ["00000_s04", "00000_s09"] + ([] if full else ["00000"])
    gen = [sys.executable, osp.join(ROOT, "frame_score_gen.py"), "--data", str(out)] + (["--full"] if full else [])

    def tables():
        ts = [pipeline.parse_frame_score_file(open(out / "FrameScore" / "a" / (n + ".txt")).read()) for n in names
              if osp.exists(out / "FrameScore" / "a" / (n + ".txt"))]
        pooled = pipeline.add_frame_scores(ts)
        assert open(out / "frame_score.txt").read() == pipeline.format_frame_score(pooled)
        return ts, pooled

    printed = _run(gen + ["--est", str(out)], str(tmp_path))
    assert "%d frames scored, 0 without an estimate" % len(names) in printed and "%d exact frames" % len(names) in printed
    ts, exact = tables()
    assert len(ts) == len(names) and open(out / "frame_score_missing.list").read() == ""
    rows = [0, 1, 2] + ([] if full else [3, 4, 5])                  # occ everywhere, dist with frame 2; obj never
    assert (exact[rows, 0] > 0).all() and (exact[rows, 4] > 0).all() and not exact[6:].any()
    assert not exact[:, [1, 2, 3, 6]].any() and (exact[:8, 5] == exact[:8, 4] * ONE).all()
    s = pipeline.frame_score_summary(exact)
    assert all(s[pipeline.FSCORE_ROWS[r]]["psnr"] == float("inf") and s[pipeline.FSCORE_ROWS[r]]["ssim"] == 1.0 for r in rows)
    for n in names[:2]:                                             # a per-frame file is the twin's on the files named
        text, _ = _twin_text(str(out / mid / "a" / (n + ".png")), str(out / mid / "a" / (n + ".png")), occ=str(out / mid / "a" / (n + "_occ.png")))
        assert open(out / "FrameScore" / "a" / (n + ".txt")).read() == text
    for n in names:
        os.remove(out / "FrameScore" / "a" / (n + ".txt"))

    printed = _run(gen + ["--baseline", "blend"], str(tmp_path))
    assert "2 frames scored, %d without an estimate" % (len(names) - 2) in printed and "0 exact frames" in printed
    assert "over 2 frames" in printed
    ts, blend = tables()
    assert len(ts) == 2
    assert open(out / "frame_score_missing.list").read() == ("" if full else str(out / "wRGB" / "a" / "00000.png") + "\n")
    a, b = (np.array(Image.open(out / d / "a" / "00000.png")).astype(np.uint16) for d in ("inpRGB", "wRGB"))
    assert np.array_equal(np.array(Image.open(out / "FramesEst" / mid / "a" / "00000_s04.png")), ((a + b + 1) >> 1).astype(np.uint8))
    assert blend[0, 0] == 2 * 72 * 40 and blend[0, 1] > 0 and blend[0, 5] < blend[0, 4] * ONE and blend[0, 6] > 0
    sb = pipeline.frame_score_summary(blend)["all"]
    assert sb["psnr"] < 40 and sb["ssim"] < 0.99 and sb["ssim_min"] < 0.9
    text, _ = _twin_text(str(out / mid / "a" / "00000_s09.png"), str(out / "FramesEst" / mid / "a" / "00000_s09.png"),
                         occ=str(out / mid / "a" / "00000_s09_occ.png"))
    assert open(out / "FrameScore" / "a" / "00000_s09.txt").read() == text
