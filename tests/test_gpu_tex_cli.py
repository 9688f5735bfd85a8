"""GPU: the `tex` list line through both arap_deform twins (list file and --serve) and para_gen.py --retex (child
processes), against the library calls pipeline.run_texture makes."""
import filecmp
import os
import os.path as osp
import random
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

from arap_flow_amd import build, opt, pipeline, synth

pytestmark = pytest.mark.gpu
ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))


def _env():
    return dict(os.environ, HIP_VISIBLE_DEVICES=os.environ.get("HIP_VISIBLE_DEVICES", "0"))


def _run(args, cwd, stdin=None):
    r = subprocess.run(args, cwd=cwd, env=_env(), capture_output=True, text=True, timeout=600, input=stdin)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_solve_lines_then_a_tex_line_both_twins_equal_run_texture(tmp_path, gpu_state):
    """a frame of two segments: its two solve lines, then the frame's tex line over the flows they write -- as a list
    through the C++ worker and arap_deform.py, and line by line through --serve"""
    W, H = 96, 64
    fr = synth.make_frame(W, H, seed=98, K=2, fd=1)
    p = lambda n: str(tmp_path / n)
    Image.fromarray(fr["rgb"]).save(p("r.png"))
    segs = pipeline.split_segments(fr["labels"].astype(np.uint8), [int(fr["labels"][c[1], c[0]]) for c in fr["constraints"]])
    assert len(segs) == 2
    for s, mask in segs:
        Image.fromarray(mask).save(p("m%d.png" % s))
        rows = [tuple(c) for c in fr["constraints"] if fr["labels"][c[1], c[0]] == s]
        pipeline.write_constraints(p("c%d.txt" % s), rows)
    layers = tuple(pipeline.tex_layers(random.Random(3), 2, (W, H)))
    cpp = build.build_host()[0]
    got = {}
    for tag, prog, serve in (("cpp", [cpp], False), ("srv", [cpp], True), ("py", [sys.executable, osp.join(ROOT, "arap_deform.py")], False)):
        q = lambda n: p(tag + "_" + n)
        solves = [pipeline.SolveLine(p("r.png"), p("m%d.png" % s), p("c%d.txt" % s), q("f%d.flo" % s), q("w%d.png" % s),
                                     q("wm%d.png" % s), extra={}) for s, _ in segs]
        item = pipeline.TexLine(p("r.png"), [(ln.mask, ln.flow) for ln in solves], layers,
                                dict(rgb1=q("t1.png"), rgb2=q("t2.png"), mask2=q("tm.png")))
        text = [pipeline.format_line(ln) for ln in solves] + [pipeline.format_line(item)]
        if serve:       # --serve names only files that exist: the tex line follows the solves' "Done"
            pr = subprocess.Popen(prog + ["--serve"], cwd=str(tmp_path), env=_env(), stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                  text=True, bufsize=1)
            try:
                assert pr.stdout.readline().strip() == "Ready"
                pr.stdin.write("\n".join(text[:2]) + "\n")
                pr.stdin.flush()
                done = set()
                while len(done) < 2:
                    ln = pr.stdout.readline()
                    assert ln, "the worker ended early"
                    if ln.startswith("Done "):
                        done.add(ln[5:].strip())
                assert done == {s.flow for s in solves}
                pr.stdin.write(text[2] + "\n")
                pr.stdin.close()
                rest = pr.stdout.read().splitlines()
                assert pr.wait(timeout=120) == 0
            finally:
                if pr.poll() is None:
                    pr.kill()
            assert "Done " + pipeline.done_token(item) in rest and pipeline.done_token(item) == q("t1.png")
        else:
            (tmp_path / (tag + ".txt")).write_text("\n".join(text) + "\n")
            _run(prog + [p(tag + ".txt")], str(tmp_path))
        # the same line through the Python twin's own function, over the flows this run solved
        want = pipeline.TexLine(item.rgb, item.layers, item.tex, {k: v.replace(tag + "_", tag + "_want_") for k, v in item.out.items()})
        pipeline.run_texture(gpu_state, want)
        for k in pipeline.TEX_KEYS:
            a, b = Image.open(item.out[k]), Image.open(want.out[k])
            assert a.mode == b.mode and np.array_equal(np.array(a), np.array(b)), (tag, k)
        assert Image.open(item.out["mask2"]).mode == "1"
        got[tag] = [np.array(Image.open(item.out[k])) for k in pipeline.TEX_KEYS]
    rgb1 = got["cpp"][0]
    obj = np.any([mask == 0 for _, mask in segs], axis=0)
    assert np.array_equal(rgb1[~obj], fr["rgb"][~obj]) and (rgb1[obj] != fr["rgb"][obj]).any()
    # a line that asks for the retextured frame alone reads no flow and writes nothing else
    item = pipeline.TexLine(p("r.png"), [(p("m%d.png" % s), p("missing%d.flo" % s)) for s, _ in segs], layers, dict(rgb1=p("only_t1.png")))
    (tmp_path / "only.txt").write_text(pipeline.format_line(item) + "\n")
    _run([cpp, p("only.txt")], str(tmp_path))
    assert np.array_equal(np.array(Image.open(p("only_t1.png"))), rgb1)
    assert [f for f in os.listdir(tmp_path) if f.startswith("only_")] == ["only_t1.png"]
    # a malformed tex line fails a list run
    (tmp_path / "bad.txt").write_text("tex r.png 1 m f rgb1=x\n")
    assert subprocess.run([cpp, p("bad.txt")], cwd=str(tmp_path), env=_env(), capture_output=True).returncode == 1


@pytest.mark.parametrize("multseg", [False, True])
def test_para_gen_retex(tmp_path, gpu_state, multseg):
    W, H = 96, 64
    inp, mdir, bgd = tmp_path / "in", tmp_path / "matches", tmp_path / "bgs"
    os.makedirs(inp / "orgRGB" / "a"); os.makedirs(inp / "orgMasks" / "a"); os.makedirs(mdir / "a"); os.makedirs(bgd)
    fr = synth.make_frame(W, H, seed=98, K=2, fd=1)
    for n in range(2):                                                      # two frames: one pair
        Image.fromarray(fr["rgb"]).save(inp / "orgRGB" / "a" / ("%05d.png" % n))
        Image.fromarray(fr["labels"].astype(np.uint8)).save(inp / "orgMasks" / "a" / ("%05d.png" % n))
        (mdir / "a" / ("%05d.txt" % n)).write_text("\n".join("%d %d %d %d 1.0 0" % tuple(c) for c in fr["constraints"]))
    Image.fromarray(np.random.default_rng(1).integers(0, 256, (140, 220, 3)).astype(np.uint8)).save(bgd / "one.png")
    base = [sys.executable, osp.join(ROOT, "para_gen.py"), "--input", str(inp), "--gpu", "0", "--fd", "1", "--matches",
            str(mdir), "--bg_dir", str(bgd), "--jobs", "2"] + (["--multseg", "--keep_segments"] if multseg else [])
    plain, outp = tmp_path / "plain", tmp_path / "out"
    _run(base + ["--output", str(plain)], str(tmp_path))
    _run(base + ["--output", str(outp), "--retex"], str(tmp_path))
    assert not (plain / "all_files_tex.list").exists() and not (plain / "inpRGB_tex").exists()
    for d in ("Flow", "wRGB", "wMasks", "inpRGB"):                          # the pair itself: as without --retex
        names = sorted(os.listdir(plain / d / "a"))
        assert names and names == sorted(os.listdir(outp / d / "a"))
        assert filecmp.cmpfiles(plain / d / "a", outp / d / "a", names, shallow=False)[0] == names, d
    assert open(plain / "all_files.list").read().replace(str(plain), str(outp)) == open(outp / "all_files.list").read()
    (pair,), (twin,) = [open(outp / f).read().splitlines() for f in ("all_files.list", "all_files_tex.list")]
    (rgb1, rgb2, flow), (t1, t2, tflow) = pair.split(" "), twin.split(" ")
    assert tflow == flow and t1 == str(outp / "inpRGB_tex" / "a" / "00000.png") and t2 == str(outp / "wRGB_tex" / "a" / "00000.png")
    assert all(osp.exists(q) for q in (t1, t2, tflow))
    # frame 1 of the twin: the pair's frame 1 with the textures of the pair's id on its solved layers, nothing else
    import para_gen
    if multseg:
        seg_masks = sorted(f for f in os.listdir(outp / "inpMasks" / "a") if "_seg" in f)
        assert len(seg_masks) == 2
    else:
        seg_masks = ["00000.png"]
    masks = np.stack([pipeline.load_mask_red(str(outp / "inpMasks" / "a" / f)) for f in seg_masks])
    layers = pipeline.tex_layers(random.Random(para_gen._pair_id("a", "00000")), len(masks), (W, H))
    a, b = pipeline.load_rgb(rgb1), pipeline.load_rgb(t1)
    obj = (masks == 0).any(0)
    assert np.array_equal(b, opt.texture(gpu_state, a, masks, layers))
    assert np.array_equal(a[~obj], b[~obj]) and (a[obj] != b[obj]).any(1).mean() > 0.9
    # frame 2 of the twin: the pair's background off the warped object, the warped texture on it
    cover = np.array(Image.open(outp / "wMasks" / "a" / "00000.png")) != 0
    wa, wb = pipeline.load_rgb(rgb2), pipeline.load_rgb(t2)
    assert cover.any() and (~cover).any() and np.array_equal(wa[~cover], wb[~cover])
    assert (wa[cover] != wb[cover]).any(1).mean() > 0.9
