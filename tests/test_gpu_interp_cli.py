"""GPU: the `interp` list line through both arap_deform twins (list file and --serve) and frame_score_gen.py --from_flows
(child processes), against the numpy twins tests/interp_ref.py and tests/fscore_ref.py on the files those runs read."""
import os
import os.path as osp
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import fscore_ref
import interp_ref as R
from arap_flow_amd import build, flo, pipeline

pytestmark = pytest.mark.gpu
ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
F = np.float32
SQ, X0, Y0, SHIFT = 24, 8, 9, 19


def _env():
    return dict(os.environ, HIP_VISIBLE_DEVICES=os.environ.get("HIP_VISIBLE_DEVICES", "0"))


def _run(args, cwd, stdin=None):
    r = subprocess.run(args, cwd=cwd, env=_env(), capture_output=True, text=True, timeout=600, input=stdin)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _scene(W, H, seed):
    """(frame(shift), fwd, bwd): a textured square moving SHIFT pixels to the right over a textured static ground, with
    its true forward and backward flows"""
    rng = np.random.default_rng(seed)
    ground = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    square = rng.integers(0, 256, (SQ, SQ, 3)).astype(np.uint8)

    def frame(shift):
        im = ground.copy()
        im[Y0:Y0 + SQ, X0 + shift:X0 + shift + SQ] = square
        return im
    fwd, bwd = np.zeros((H, W, 2), F), np.zeros((H, W, 2), F)
    fwd[Y0:Y0 + SQ, X0:X0 + SQ, 0] = SHIFT
    bwd[Y0:Y0 + SQ, X0 + SHIFT:X0 + SHIFT + SQ, 0] = -SHIFT
    return frame, fwd, bwd


def test_interp_lines_all_three_hosts_equal_the_twin(tmp_path):
    """the same three lines -- with bwd and source maps, without either, one step with a noisy flow -- through the C++
    worker on a list, through --serve and through arap_deform.py: the twin's frames and source maps"""
    W, H = 75, 41
    p = lambda n: str(tmp_path / n)
    frame, fwd, bwd = _scene(W, H, 21)
    rng = np.random.default_rng(22)
    noisy = (fwd + np.round(rng.normal(size=fwd.shape) * 64) / 64 * (rng.random((H, W, 1)) < 0.3)).astype(F)
    noisy[5, 7:30] = np.nan
    Image.fromarray(frame(0)).save(p("a.png"))
    Image.fromarray(frame(SHIFT)).save(p("b.png"))
    flo.flow_write(p("fwd.flo"), fwd)
    flo.flow_write(p("bwd.flo"), bwd)
    flo.flow_write(p("noisy.flo"), noisy)
    variants = [((4, 9, 14), 19, "fwd.flo", "bwd.flo", True), ((4, 9), 19, "fwd.flo", "", False), ((1,), 2, "noisy.flo", "bwd.flo", True)]
    item = lambda tag, k: pipeline.InterpLine(p("a.png"), p("b.png"), p(variants[k][2]), variants[k][0], variants[k][1],
                                              p(variants[k][3]) if variants[k][3] else "", variants[k][4], p("%s_%d" % (tag, k)))
    lines = lambda tag: "".join(pipeline.format_line(item(tag, k)) + "\n" for k in range(len(variants)))
    cpp = build.build_host()[0]
    (tmp_path / "cpp.txt").write_text(lines("cpp"))
    _run([cpp, p("cpp.txt")], str(tmp_path))
    out = _run([cpp, "--serve"], str(tmp_path), stdin=lines("srv"))
    assert ["Done " + p("srv_%d" % k) in out.splitlines() for k in range(len(variants))] == [True] * len(variants)
    (tmp_path / "py.txt").write_text(lines("py"))
    _run([sys.executable, osp.join(ROOT, "arap_deform.py"), p("py.txt")], str(tmp_path))
    a, b = pipeline.load_rgb(p("a.png")), pipeline.load_rgb(p("b.png"))
    for k, (steps, n, f, g, want_src) in enumerate(variants):
        want, src = R.interp_ref(a, b, flo.flow_read(p(f)), pipeline.interp_times(steps, n), flo.flow_read(p(g)) if g else None)
        for tag in ("cpp", "srv", "py"):
            for j, i in enumerate(steps):
                names = pipeline.interp_files(p("%s_%d" % (tag, k)), i)
                assert np.array_equal(np.array(Image.open(names["rgb"]).convert("RGB")), want[j]), (tag, k, i)
                assert osp.exists(names["src"]) == want_src
                if want_src:
                    assert np.array_equal(np.array(Image.open(names["src"])), src[j]), (tag, k, i)
        if k == 0:                                              # with the true flows a step is the true frame but near the edges
            assert (want[1] == frame(9)).all(axis=-1).mean() > 0.95 and set(np.unique(src)) >= {0, 1, 2}
    # sizes that differ are an error of that line, at run time
    flo.flow_write(p("small.flo"), fwd[:-1])
    bad = pipeline.InterpLine(p("a.png"), p("b.png"), p("small.flo"), (4,), 19, "", False, p("bad"))
    (tmp_path / "bad.txt").write_text(pipeline.format_line(bad) + "\n")
    assert subprocess.run([cpp, p("bad.txt")], cwd=str(tmp_path), env=_env(), capture_output=True).returncode == 1
    assert subprocess.run([sys.executable, osp.join(ROOT, "arap_deform.py"), p("bad.txt")], cwd=str(tmp_path), env=_env(),
                          capture_output=True).returncode != 0
    assert not osp.exists(p("bad_s04.png"))


def _tree(out, full):
    """a dataset tree with one pair of sequence `a`: the end frames, two in-between frames with their link occlusions, the
    true flows in both directions, and -- without `full` -- the planes of frame 2"""
    W, H = 72, 40
    rng = np.random.default_rng(12)
    mid = "MidFull" if full else "Mid"
    flow, back = ("FlowFull", "FlowBwdFull") if full else ("Flow", "FlowBwd")
    for d in ("inpRGB", "wRGB", mid, "OccBwd", "MBDistBwd", flow, back):
        os.makedirs(out / d / "a")
    frame, fwd, bwd = _scene(W, H, 13)
    Image.fromarray(frame(0)).save(out / "inpRGB" / "a" / "00000.png")
    Image.fromarray(frame(SHIFT)).save(out / "wRGB" / "a" / "00000.png")
    for step in (4, 9):
        Image.fromarray(frame(step)).save(out / mid / "a" / ("00000_s%02d.png" % step))
        Image.fromarray((rng.random((H, W)) < 0.2).astype(np.uint8) * 255, "L").save(out / mid / "a" / ("00000_s%02d_occ.png" % step))
        Image.fromarray(np.zeros((H, W), np.uint8), "L").save(out / mid / "a" / ("00000_s%02d_mask.png" % step))     # no frame, no plane
    Image.fromarray((rng.random((H, W)) < 0.2).astype(np.uint8) * 255, "L").save(out / "OccBwd" / "a" / "00000.png")
    Image.fromarray(rng.integers(0, 256, (H, W)).astype(np.uint8), "L").save(out / "MBDistBwd" / "a" / "00000.png")
    flo.flow_write(str(out / flow / "a" / "00000.flo"), fwd)
    flo.flow_write(str(out / back / "a" / "00000.flo"), bwd)
    return frame, fwd, bwd


@pytest.mark.parametrize("full", [False, True], ids=["objects", "full"])
def test_frame_score_gen_from_flows_on_a_tiny_tree(tmp_path, full):
    """--from_flows --est OUT, the oracle flow: the frames written are the twin's, the per-frame score files the scoring
    twin's on those files, the pooled PSNR strictly above the blend's on the same tree, frame 2 listed as missing"""
    out = tmp_path / "out"
    frame, fwd, bwd = _tree(out, full)
    mid = "MidFull" if full else "Mid"
    names = ["00000_s04", "00000_s09"]
    gen = [sys.executable, osp.join(ROOT, "frame_score_gen.py"), "--data", str(out)] + (["--full"] if full else [])

    def pooled():
        ts = [pipeline.parse_frame_score_file(open(out / "FrameScore" / "a" / (n + ".txt")).read()) for n in names]
        t = pipeline.add_frame_scores(ts)
        assert open(out / "frame_score.txt").read() == pipeline.format_frame_score(t)
        return t

    printed = _run(gen + ["--est", str(out), "--from_flows"], str(tmp_path))
    assert "2 frames scored, %d without an estimate" % (0 if full else 1) in printed
    assert open(out / "frame_score_missing.list").read() == ("" if full else str(out / "wRGB" / "a" / "00000.png") + "\n")
    a, b = (pipeline.load_rgb(str(out / d / "a" / "00000.png")) for d in ("inpRGB", "wRGB"))
    want, _ = R.interp_ref(a, b, fwd, pipeline.interp_times((4, 9), 19), bwd)
    for k, n in enumerate(names):
        est = np.array(Image.open(out / "FramesEst" / mid / "a" / (n + ".png")).convert("RGB"))
        assert np.array_equal(est, want[k])
        occ = pipeline.load_mask_red(str(out / mid / "a" / (n + "_occ.png")))
        t = fscore_ref.fscore_ref(pipeline.load_rgb(str(out / mid / "a" / (n + ".png"))), est, occ=occ)["table"][0]
        assert open(out / "FrameScore" / "a" / (n + ".txt")).read() == pipeline.format_frame_score(t)
    flows = pooled()
    assert not osp.exists(out / "FrameScore" / "a" / "00000.txt")
    for n in names:
        os.remove(out / "FrameScore" / "a" / (n + ".txt"))
    _run(gen + ["--baseline", "blend"], str(tmp_path))
    blend = pooled()
    sf, sb = pipeline.frame_score_summary(flows)["all"], pipeline.frame_score_summary(blend)["all"]
    assert flows[0, 0] == blend[0, 0] == 2 * 72 * 40 and sf["psnr"] > sb["psnr"] and sf["ssim"] > sb["ssim"]
