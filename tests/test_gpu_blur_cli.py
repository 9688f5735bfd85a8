"""GPU: the `blur` list line through both arap_deform twins (list file and --serve) and para_gen.py --blur (child
processes), against opt.blur_pair on the files those runs wrote."""
import filecmp
import os
import os.path as osp
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import bg_ref
from arap_flow_amd import build, flo, opt, pipeline, synth

pytestmark = pytest.mark.gpu
ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))


def _env():
    return dict(os.environ, HIP_VISIBLE_DEVICES=os.environ.get("HIP_VISIBLE_DEVICES", "0"))


def _run(args, cwd, stdin=None):
    r = subprocess.run(args, cwd=cwd, env=_env(), capture_output=True, text=True, timeout=600, input=stdin)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_solve_lines_then_a_blur_line_both_twins_equal_blur_pair(tmp_path, gpu_state):
    """a frame of two segments: its two solve lines, then the frame's blur line over the flows they write -- as a list
    through the C++ worker and arap_deform.py, and line by line through --serve"""
    W, H = 96, 64
    fr = synth.make_frame(W, H, seed=98, K=2, fd=1)
    p = lambda n: str(tmp_path / n)
    Image.fromarray(fr["rgb"]).save(p("r.png"))
    bg = np.random.default_rng(5).integers(0, 256, (H + 20, W + 30, 3)).astype(np.uint8)
    Image.fromarray(bg).save(p("bg.png"))
    m = tuple(float(v) for v in np.concatenate([bg_ref.similarity(2.0, 1.02, (12.0, 8.0), (W / 2, H / 2)),
                                                bg_ref.similarity(-1.5, 0.99, (15.5, 10.25), (W / 2, H / 2))]))
    segs = pipeline.split_segments(fr["labels"].astype(np.uint8), [int(fr["labels"][c[1], c[0]]) for c in fr["constraints"]])
    assert len(segs) == 2
    for s, mask in segs:
        Image.fromarray(mask).save(p("m%d.png" % s))
        rows = [tuple(c) for c in fr["constraints"] if fr["labels"][c[1], c[0]] == s]
        pipeline.write_constraints(p("c%d.txt" % s), rows)
    masks = np.stack([mask for _, mask in segs])
    cpp = build.build_host()[0]
    for tag, prog, serve in (("cpp", [cpp], False), ("srv", [cpp], True), ("py", [sys.executable, osp.join(ROOT, "arap_deform.py")], False)):
        q = lambda n: p(tag + "_" + n)
        solves = [pipeline.SolveLine(p("r.png"), p("m%d.png" % s), p("c%d.txt" % s), q("f%d.flo" % s), q("w%d.png" % s),
                                     q("wm%d.png" % s), extra={}) for s, _ in segs]
        item = pipeline.BlurLine(p("r.png"), [(ln.mask, ln.flow) for ln in solves], p("bg.png"), 0.5, 9, m,
                                 dict(rgb1=q("b1.png"), rgb2=q("b2.png"), alpha1=q("a1.png"), alpha2=q("a2.png")))
        text = [pipeline.format_line(ln) for ln in solves] + [pipeline.format_line(item)]
        if serve:       # --serve names only files that exist: the blur line follows the solves' "Done"
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
            assert "Done " + pipeline.done_token(item) in rest and pipeline.done_token(item) == q("b1.png")
        else:
            (tmp_path / (tag + ".txt")).write_text("\n".join(text) + "\n")
            _run(prog + [p(tag + ".txt")], str(tmp_path))
        # the library call on the flows this run solved
        flows = np.stack([flo.flow_read(ln.flow) for ln in solves])
        (r1, a1), (r2, a2) = opt.blur_pair(gpu_state, fr["rgb"], masks, flows, 0.5, 9, bg=bg, maps=(m[:6], m[6:]))
        for k, want in (("rgb1", r1), ("rgb2", r2), ("alpha1", a1), ("alpha2", a2)):
            im = Image.open(item.out[k])
            assert im.mode == ("RGB" if k.startswith("rgb") else "L") and np.array_equal(np.array(im), want), (tag, k)
        assert (a2 == 255).any() and ((a2 > 0) & (a2 < 255)).any() and (a2 == 0).any()
        assert not np.array_equal(r1, r2)
    # a line that asks for one frame's alpha alone writes nothing else; without m= the camera is the identity
    item = pipeline.BlurLine(p("r.png"), [(p("m%d.png" % s), p("cpp_f%d.flo" % s)) for s, _ in segs], p("bg.png"), 1.0, 3, (),
                             dict(alpha2=p("only_a2.png")))
    (tmp_path / "only.txt").write_text(pipeline.format_line(item) + "\n")
    _run([cpp, p("only.txt")], str(tmp_path))
    flows = np.stack([flo.flow_read(p("cpp_f%d.flo" % s)) for s, _ in segs])
    want = opt.blur_layers(gpu_state, fr["rgb"], masks, flows, 1.0, 1.0, 3, bg=bg, want=("alpha",))[1]
    assert np.array_equal(np.array(Image.open(p("only_a2.png"))), want)
    assert [f for f in os.listdir(tmp_path) if f.startswith("only_")] == ["only_a2.png"]
    # a malformed blur line fails a list run
    (tmp_path / "bad.txt").write_text("blur r.png 1 m f bg.png rgb1=x\n")
    assert subprocess.run([cpp, p("bad.txt")], cwd=str(tmp_path), env=_env(), capture_output=True).returncode == 1


@pytest.mark.parametrize("multseg", [False, True], ids=["plain", "multseg-bg_motion"])
def test_para_gen_blur(tmp_path, gpu_state, multseg):
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
    _run(base + ["--output", str(outp), "--blur", "0.5"], str(tmp_path))
    assert not (plain / "all_files_blur.list").exists() and not (plain / "inpRGB_blur").exists()
    for d in ("Flow", "wRGB", "wMasks", "inpRGB", "inpMasks") + (("FlowFull",) if multseg else ()):      # the pair itself: as without --blur
        names = sorted(os.listdir(plain / d / "a"))
        assert names and names == sorted(os.listdir(outp / d / "a"))
        assert filecmp.cmpfiles(plain / d / "a", outp / d / "a", names, shallow=False)[0] == names, d
    assert open(plain / "all_files.list").read().replace(str(plain), str(outp)) == open(outp / "all_files.list").read()
    pairs, blurred = [open(outp / f).read().splitlines() for f in ("all_files.list", "all_files_blur.list")]
    assert len(pairs) == len(blurred) == 2
    for k, (pair, twin) in enumerate(zip(pairs, blurred)):
        stem = "%05d" % k
        (rgb1, rgb2, flow), (b1, b2, bflow) = pair.split(" "), twin.split(" ")
        assert bflow == flow == str(outp / "Flow" / "a" / (stem + ".flo"))                          # the clean pair's file
        assert b1 == str(outp / "inpRGB_blur" / "a" / (stem + ".png")) and b2 == str(outp / "wRGB_blur" / "a" / (stem + ".png"))
        assert all(osp.exists(q) for q in (b1, b2, bflow))
        # the library call over the files the run kept: the solved layers, the line's own background and camera
        tmp = outp / "tmpCnstr" / "a"
        if multseg:
            seg = lambda d, ext: sorted(str(outp / d / "a" / f) for f in os.listdir(outp / d / "a") if f.startswith(stem + "_seg") and f.endswith(ext))
            mask_files, flow_files = seg("inpMasks", ".png"), seg("Flow", ".flo")
            assert len(mask_files) == len(flow_files) == 2
            line = pipeline.parse_line(open(tmp / (stem + "_bg.txt")).read())
            bg, maps = pipeline.load_rgb(line.bg), (line.m[:6], line.m[6:])
            assert line.m[:6] != line.m[6:]
        else:
            mask_files, flow_files = [str(outp / "inpMasks" / "a" / (stem + ".png"))], [flow]
            bg, maps = pipeline.load_rgb(str(tmp / (stem + "_blurbg.png"))), None
            assert bg.shape == (H, W, 3)
        masks = np.stack([pipeline.load_mask_red(f) for f in mask_files])
        flows = np.stack([flo.flow_read(f) for f in flow_files])
        (r1, _), (r2, _) = opt.blur_pair(gpu_state, pipeline.load_rgb(rgb1), masks, flows, 0.5, 9, bg=bg, maps=maps, want=("rgb",))
        assert np.array_equal(pipeline.load_rgb(b1), r1) and np.array_equal(pipeline.load_rgb(b2), r2)
        # a pixel no sample touches shows what the clean frame shows there (a still camera); a moving object is smeared
        if not multseg:
            a2 = opt.blur_layers(gpu_state, pipeline.load_rgb(rgb1), masks, flows, 1.0, 0.5, 9, want=("alpha",))[1]
            clean2 = pipeline.load_rgb(rgb2)
            assert (a2 == 0).any() and np.array_equal(r2[a2 == 0], clean2[a2 == 0])
            assert ((a2 > 0) & (a2 < 255)).any()
