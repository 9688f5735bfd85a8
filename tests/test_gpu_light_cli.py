"""GPU: the `light` list line through both arap_deform twins (list file and --serve) and para_gen.py --relight (child
processes), against the numpy twin tests/light_ref.py on the files those runs read."""
import filecmp
import json
import os
import os.path as osp
import random
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import light_ref
from arap_flow_amd import build, pipeline, synth

pytestmark = pytest.mark.gpu
ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))


def _env():
    return dict(os.environ, HIP_VISIBLE_DEVICES=os.environ.get("HIP_VISIBLE_DEVICES", "0"))


def _run(args, cwd, stdin=None):
    r = subprocess.run(args, cwd=cwd, env=_env(), capture_output=True, text=True, timeout=600, input=stdin)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_a_light_line_through_both_twins_equals_the_twin(tmp_path):
    """a finished pair on disk -- frame 1 with a solver mask, frame 2 with a 1-bit cover as a warp writes it -- relit by the
    C++ worker from a list, by the C++ worker through --serve and by arap_deform.py"""
    W, H = 96, 64
    fr = synth.make_frame(W, H, seed=98, K=2, fd=1)
    p = lambda n: str(tmp_path / n)
    rgb1 = fr["rgb"]
    rgb2, obj2 = np.roll(rgb1, (2, 5), (0, 1)), np.roll(fr["mask_red"] == 0, (2, 5), (0, 1))
    Image.fromarray(rgb1).save(p("r1.png"))
    Image.fromarray(rgb2).save(p("r2.png"))
    Image.fromarray(fr["mask_red"]).save(p("m1.png"))
    pipeline.save_mask(np.where(obj2, 255, 0).astype(np.uint8), p("c2.png"))
    frames = pipeline.random_light(random.Random(7), 1.0, W, H)
    assert frames[0].sh_g > 0
    want1 = light_ref.relight(rgb1, fr["mask_red"], frames[0], cover_is_mask=True)
    want2 = light_ref.relight(rgb2, np.where(obj2, 255, 0), frames[1])
    assert not np.array_equal(want1, rgb1) and not np.array_equal(want2, rgb2)
    cpp = build.build_host()[0]
    for tag, prog, serve in (("cpp", [cpp], False), ("srv", [cpp], True), ("py", [sys.executable, osp.join(ROOT, "arap_deform.py")], False)):
        q = lambda n: p(tag + "_" + n)
        item = pipeline.LightLine(p("r1.png"), p("m1.png"), p("r2.png"), p("c2.png"), frames, dict(rgb1=q("l1.png"), rgb2=q("l2.png")))
        text = pipeline.format_line(item)
        assert pipeline.parse_line(text) == item
        if serve:
            out = _run(prog + ["--serve"], str(tmp_path), stdin=text + "\n").splitlines()
            assert out[0] == "Ready" and "Done " + q("l1.png") in out
        else:
            (tmp_path / (tag + ".txt")).write_text(text + "\n")
            _run(prog + [p(tag + ".txt")], str(tmp_path))
        for k, want in (("rgb1", want1), ("rgb2", want2)):
            im = Image.open(item.out[k])
            assert im.mode == "RGB" and np.array_equal(np.array(im), want), (tag, k)
    # a line that asks for frame 2 alone reads and writes nothing of frame 1
    item = pipeline.LightLine(p("absent.png"), p("absent_too.png"), p("r2.png"), p("c2.png"), frames, dict(rgb2=p("only_l2.png")))
    (tmp_path / "only.txt").write_text(pipeline.format_line(item) + "\n")
    _run([cpp, p("only.txt")], str(tmp_path))
    assert np.array_equal(np.array(Image.open(p("only_l2.png"))), want2)
    assert [f for f in os.listdir(tmp_path) if f.startswith("only_")] == ["only_l2.png"]
    # a malformed light line fails a list run
    (tmp_path / "bad.txt").write_text("light r1.png m1.png r2.png c2.png rgb1=x\n")
    assert subprocess.run([cpp, p("bad.txt")], cwd=str(tmp_path), env=_env(), capture_output=True).returncode == 1


@pytest.mark.parametrize("multseg", [False, True], ids=["plain", "multseg-bg_motion"])
def test_para_gen_relight(tmp_path, multseg):
    sys.path.insert(0, ROOT)
    import para_gen
    W, H = 96, 64
    inp, mdir, bgd = tmp_path / "in", tmp_path / "matches", tmp_path / "bgs"
    os.makedirs(inp / "orgRGB" / "a"); os.makedirs(inp / "orgMasks" / "a"); os.makedirs(mdir / "a"); os.makedirs(bgd)
    fr = synth.make_frame(W, H, seed=98, K=2, fd=1)
    for n in range(3):                                                      # three frames: two pairs
        Image.fromarray(fr["rgb"]).save(inp / "orgRGB" / "a" / ("%05d.png" % n))
        Image.fromarray(fr["labels"].astype(np.uint8)).save(inp / "orgMasks" / "a" / ("%05d.png" % n))
        (mdir / "a" / ("%05d.txt" % n)).write_text("\n".join("%d %d %d %d 1.0 0" % tuple(c) for c in fr["constraints"]))
    Image.fromarray(np.random.default_rng(1).integers(0, 256, (140, 220, 3)).astype(np.uint8)).save(bgd / "one.png")
    base = [sys.executable, osp.join(ROOT, "para_gen.py"), "--input", str(inp), "--gpu", "0", "--fd", "1", "--matches",
            str(mdir), "--bg_dir", str(bgd), "--jobs", "2", "--keep_segments"] + (["--multseg", "--bg_motion"] if multseg else [])
    plain, outp = tmp_path / "plain", tmp_path / "out"
    _run(base + ["--output", str(plain)], str(tmp_path))
    _run(base + ["--output", str(outp), "--relight"], str(tmp_path))
    assert not (plain / "all_files_light.list").exists() and not (plain / "inpRGB_light").exists()
    for d in ("Flow", "wRGB", "wMasks", "inpRGB", "inpMasks") + (("FlowFull",) if multseg else ()):      # the pair itself: as without --relight
        names = sorted(os.listdir(plain / d / "a"))
        assert names and names == sorted(os.listdir(outp / d / "a"))
        assert filecmp.cmpfiles(plain / d / "a", outp / d / "a", names, shallow=False)[0] == names, d
    assert open(plain / "all_files.list").read().replace(str(plain), str(outp)) == open(outp / "all_files.list").read()
    pairs, relit = [open(outp / f).read().splitlines() for f in ("all_files.list", "all_files_light.list")]
    assert len(pairs) == len(relit) == 2
    for k, (pair, twin) in enumerate(zip(pairs, relit)):
        stem = "%05d" % k
        (rgb1, rgb2, flow), (l1, l2, lflow) = pair.split(" "), twin.split(" ")
        assert lflow == flow == str(outp / "Flow" / "a" / (stem + ".flo"))                          # the clean pair's file
        assert l1 == str(outp / "inpRGB_light" / "a" / (stem + ".png")) and l2 == str(outp / "wRGB_light" / "a" / (stem + ".png"))
        assert all(osp.exists(q) for q in (l1, l2, lflow))
        got1, got2 = pipeline.load_rgb(l1), pipeline.load_rgb(l2)
        assert not np.array_equal(got2, pipeline.load_rgb(rgb2)) and not np.array_equal(got1, pipeline.load_rgb(rgb1))
        # the twin over the files the run kept: the finished frames, frame 1's object mask, frame 2's warped mask, and the
        # pair's own light
        mask1 = str(outp / "tmpCnstr" / "a" / (stem + "_bgmask.png")) if multseg else str(outp / "inpMasks" / "a" / (stem + ".png"))
        frames = pipeline.random_light(random.Random(para_gen._pair_id("a", stem)), 1.0, W, H)
        want1 = light_ref.relight(pipeline.load_rgb(rgb1), pipeline.load_mask_red(mask1), frames[0], cover_is_mask=True)
        want2 = light_ref.relight(pipeline.load_rgb(rgb2), pipeline.load_mask_red(str(outp / "wMasks" / "a" / (stem + ".png"))), frames[1])
        assert np.array_equal(got1, want1) and np.array_equal(got2, want2)
    assert json.load(open(outp / "arap_stats.json"))["light_done"] == 2
