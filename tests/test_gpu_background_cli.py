"""GPU: the `bg` list line through both arap_deform twins (list file and --serve) and para_gen.py --bg_motion (child
processes), against the library call opt.background."""
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
F = np.float32


def _env():
    return dict(os.environ, HIP_VISIBLE_DEVICES=os.environ.get("HIP_VISIBLE_DEVICES", "0"))


def _run(args, cwd, stdin=None):
    r = subprocess.run(args, cwd=cwd, env=_env(), capture_output=True, text=True, timeout=600, input=stdin)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _read_outputs(item):
    """the files of a bg line, decoded, under opt.background's names"""
    names = dict(zip(("out_rgb1", "out_rgb2", "flow_full"), item.out))
    names.update(occ_full=item.outs.get("occ_out"), bwd_full=item.outs.get("bwd_out"),
                 occ_bwd_full=item.outs.get("occ_bwd_out"))
    out = {}
    for k, path in names.items():
        if not path:
            continue
        out[k] = flo.flow_read(path) if path.endswith(".flo") else np.array(Image.open(path))
        if k.startswith("occ"):
            assert Image.open(path).mode == "L"
    return out


def test_bg_line_both_twins_equal_library(tmp_path, gpu_state):
    W, H = 67, 9
    c = bg_ref.ellipse_case(W, H, 80, 23, seed=5)
    r = opt.warp_image_ex(gpu_state, c["rgb1"], c["mask_red"], c["flow"])
    M1 = np.array([1, 0, 6, 0, 1, 7], F)
    M2 = bg_ref.compose(M1, bg_ref.similarity(3.0, 1.02, (2.5, -1.25), ((W - 1) / 2.0, (H - 1) / 2.0)))
    p = lambda n: str(tmp_path / n)
    Image.fromarray(c["bg"]).save(p("bg.png"))
    Image.fromarray(c["rgb1"]).save(p("r1.png"))
    Image.fromarray(np.stack([c["mask_red"]] * 3, -1)).save(p("m1.png"))
    Image.fromarray(r["warped_rgb"]).save(p("r2.png"))
    pipeline.save_mask(r["warped_mask"], p("m2.png"))
    flo.flow_write(p("f.flo"), c["flow"])
    pipeline.save_occ(r["occlusion"], p("occ.png"))
    flo.flow_write(p("b.flo"), r["backward_flow"])
    pipeline.save_occ(r["occlusion_bwd"], p("ob.png"))
    want = opt.background(gpu_state, c["bg"], M1, M2, c["rgb1"], c["mask_red"], r["warped_rgb"], r["warped_mask"],
                          c["flow"], occ=r["occlusion"], bwd=r["backward_flow"], occ_bwd=r["occlusion_bwd"])
    cpp = build.build_host()[0]
    runs = (("py", [sys.executable, osp.join(ROOT, "arap_deform.py")], False), ("cpp", [cpp], False), ("srv", [cpp], True))
    for tag, prog, serve in runs:
        q = lambda n: p(tag + "_" + n)
        item = pipeline.BgLine(p("bg.png"), p("r1.png"), p("m1.png"), p("r2.png"), p("m2.png"), p("f.flo"),
                               m=tuple(float(v) for v in np.concatenate([M1, M2])),
                               inputs=dict(occ=p("occ.png"), bwd=p("b.flo"), occ_bwd=p("ob.png")),
                               out=(q("o1.png"), q("o2.png"), q("ff.flo")),
                               outs=dict(occ_out=q("of.png"), bwd_out=q("bf.flo"), occ_bwd_out=q("obf.png")))
        text = pipeline.format_line(item)
        if serve:
            out = _run(prog + ["--serve"], str(tmp_path), stdin=text + "\n")
            assert "Done " + pipeline.done_token(item) in out.splitlines()
        else:
            (tmp_path / (tag + ".txt")).write_text(text + "\n")
            _run(prog + [p(tag + ".txt")], str(tmp_path))
        got = _read_outputs(item)
        assert set(got) == set(opt.BG_OUTPUTS)
        for k in opt.BG_OUTPUTS:
            assert got[k].tobytes() == want[k].tobytes(), (tag, k)
    # a line that asks for less: out_rgb1 left out, no optional maps -- and nothing else is written
    item = pipeline.BgLine(p("bg.png"), p("r1.png"), p("m1.png"), p("r2.png"), p("m2.png"), p("f.flo"),
                           m=tuple(float(v) for v in np.concatenate([M1, M2])), inputs={},
                           out=("", p("few_o2.png"), p("few_ff.flo")), outs={})
    (tmp_path / "few.txt").write_text(pipeline.format_line(item) + "\n")
    _run([cpp, p("few.txt")], str(tmp_path))
    got = _read_outputs(item)
    assert set(got) == {"out_rgb2", "flow_full"} and all(got[k].tobytes() == want[k].tobytes() for k in got)
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("few_")) == ["few_ff.flo", "few_o2.png"]
    # a malformed bg line fails a list run
    (tmp_path / "bad.txt").write_text("bg a b c d e f out=x,y,z\n")
    assert subprocess.run([cpp, p("bad.txt")], cwd=str(tmp_path), env=_env(), capture_output=True).returncode == 1


def test_para_gen_bg_motion(tmp_path, gpu_state):
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
            str(mdir), "--bg_dir", str(bgd), "--jobs", "2"]
    still, outp = tmp_path / "still", tmp_path / "out"
    _run(base + ["--output", str(still)], str(tmp_path))
    flags = ["--bg_motion", "--occ", "--bwd_flow", "--keep_segments"]
    _run(base + ["--output", str(outp)] + flags, str(tmp_path))
    lst = open(outp / "all_files.list").read().splitlines()
    ext = open(outp / "all_files_ext.list").read().splitlines()
    assert len(lst) == 2 and len(ext) == 2
    moved = 0
    for ln, le in zip(lst, ext):
        t = le.split(" ")
        assert t[:3] == ln.split(" ") and len(t) == 10 and all(osp.exists(q) for q in t)
        stem = osp.relpath(t[2], str(outp / "Flow"))[:-4]
        assert t[6:] == [str(outp / d / (stem + e)) for d, e in (("FlowFull", ".flo"), ("OccFull", ".png"),
                                                                 ("FlowBwdFull", ".flo"), ("OccBwdFull", ".png"))]
        # frame 1 is the frame of a run without the motion, byte for byte
        assert open(t[0], "rb").read() == open(still / "inpRGB" / (stem + ".png"), "rb").read()
        # the pair's own bg line, over the pair's own files
        item = pipeline.parse_line(open(outp / "tmpCnstr" / (stem + "_bg.txt")).read())
        assert isinstance(item, pipeline.BgLine) and item.out == ("", t[1], t[6]) and item.rgb1 == t[0]
        M1, M2 = np.asarray(item.m[:6], F), np.asarray(item.m[6:], F)
        moved += not np.array_equal(M1, M2)
        rgb2 = pipeline.load_rgb(item.rgb2)                     # (overwritten by the line: equal on the covered pixels)
        cover2 = np.where(pipeline.load_mask_red(item.mask2) != 0, 255, 0).astype(np.uint8)
        want = opt.background(gpu_state, pipeline.load_rgb(item.bg), M1, M2, pipeline.load_rgb(item.rgb1),
                              pipeline.load_mask_red(item.mask1), rgb2, cover2, flo.flow_read(item.flow),
                              occ=np.array(Image.open(item.inputs["occ"])), bwd=flo.flow_read(item.inputs["bwd"]),
                              occ_bwd=np.array(Image.open(item.inputs["occ_bwd"])))
        got = _read_outputs(item)
        assert set(got) == set(opt.BG_OUTPUTS) - {"out_rgb1"}
        for k in got:
            assert got[k].tobytes() == want[k].tobytes(), k
        # with an integer window out_rgb1 is the frame 1 already written
        assert np.array_equal(want["out_rgb1"], pipeline.load_rgb(item.rgb1))
        # on the object the full flow is the solve's, off it the camera's
        obj = pipeline.load_mask_red(item.mask1) == 0
        assert np.array_equal(got["flow_full"][obj], flo.flow_read(item.flow)[obj])
        # the static run's warped frame differs only off the object
        wst = pipeline.load_rgb(str(still / "wRGB" / (stem + ".png")))
        assert np.array_equal(wst[cover2 != 0], got["out_rgb2"][cover2 != 0])
    assert moved == 2
    # --resume: every requested output is there, nothing is redone
    out = _run(base + ["--output", str(outp), "--resume"] + flags, str(tmp_path))
    assert "Scanning data to be processed\t\t0 files" in out
