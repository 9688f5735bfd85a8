"""GPU: backward flow and occlusion maps through the command-line twins and para_gen.py (child processes)."""
import os
import os.path as osp
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

from arap_flow_amd import build, flo, opt, pipeline, synth

pytestmark = pytest.mark.gpu
ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))


def _run(args, cwd):
    env = dict(os.environ, HIP_VISIBLE_DEVICES=os.environ.get("HIP_VISIBLE_DEVICES", "0"))
    r = subprocess.run(args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_arap_deform_tokens_both_twins_equal_solver(tmp_path, gpu_state):
    W, H = 96, 64
    frames = [synth.make_frame(W, H, seed=s, fd=3) for s in (11, 12)]
    for k, f in enumerate(frames):
        Image.fromarray(f["rgb"]).save(tmp_path / ("r%d.png" % k))
        Image.fromarray(np.stack([f["mask_red"]] * 3, -1)).save(tmp_path / ("m%d.png" % k))
        pipeline.write_constraints(str(tmp_path / ("c%d.txt" % k)), [tuple(c) for c in f["constraints"]])
    outs = {}
    for tag, prog in (("py", [sys.executable, osp.join(ROOT, "arap_deform.py")]), ("cpp", [build.build_host()[0]])):
        lines = []
        for k in range(2):
            p = lambda n: str(tmp_path / ("%s_%s%d" % (tag, n, k)))
            six = [str(tmp_path / ("r%d.png" % k)), str(tmp_path / ("m%d.png" % k)), str(tmp_path / ("c%d.txt" % k)),
                   p("f") + ".flo", p("w") + ".png", p("wm") + ".png"]
            extra = ["bwd=%s.flo" % p("b"), "occ=%s.png" % p("o"), "occ_bwd=%s.png" % p("ob")] if k == 0 else ["x"]
            lines.append(" ".join(six + extra))
        (tmp_path / ("%s.txt" % tag)).write_text("\n".join(lines))
        _run(prog + [str(tmp_path / ("%s.txt" % tag))], str(tmp_path))
        outs[tag] = dict(b=flo.flow_read(str(tmp_path / ("%s_b0.flo" % tag))),
                         o=np.array(Image.open(tmp_path / ("%s_o0.png" % tag))),
                         ob=np.array(Image.open(tmp_path / ("%s_ob0.png" % tag))),
                         f1=flo.flow_read(str(tmp_path / ("%s_f1.flo" % tag))))
        assert Image.open(tmp_path / ("%s_o0.png" % tag)).mode == "L"
        assert not (tmp_path / ("%s_b1.flo" % tag)).exists()
    fs = opt.FrameSolver(gpu_state, W, H, batch=2)
    fs.set_outputs(backward=True, occlusion=True)
    for k, f in enumerate(frames):
        fs.set_frame(k, f["mask_red"], f["constraints"], rgb=f["rgb"])
    fs.solve(2, 19, 8, 400)
    fs.warp(2)
    r0, r1 = fs.results(0), fs.results(1)
    fs.close()
    for tag in ("py", "cpp"):
        o = outs[tag]
        assert np.array_equal(o["b"], r0["backward_flow"])
        assert np.array_equal(o["o"], r0["occlusion"]) and np.array_equal(o["ob"], r0["occlusion_bwd"])
        assert np.array_equal(o["f1"], r1["flow"])


def test_warp_image_tokens_both_twins(tmp_path, gpu_state):
    import occ_ref
    rgb, mask, fl = occ_ref.folded_case(70, 50, 3.0)
    Image.fromarray(rgb).save(tmp_path / "i.png")
    Image.fromarray(np.stack([mask] * 3, -1)).save(tmp_path / "m.png")
    flo.flow_write(str(tmp_path / "f.flo"), fl)
    ref = opt.warp_image_ex(gpu_state, rgb, mask, fl)
    for tag, prog in (("py", [sys.executable, osp.join(ROOT, "warp_image.py")]), ("cpp", [build.build_host()[1]])):
        q = lambda n: str(tmp_path / (tag + n))
        _run(prog + [str(tmp_path / "i.png"), str(tmp_path / "m.png"), str(tmp_path / "f.flo"), q("w.png"),
                     q("wm.png"), "bwd=" + q("b.flo"), "occ=" + q("o.png"), "occ_bwd=" + q("ob.png")], str(tmp_path))
        assert np.array_equal(flo.flow_read(q("b.flo")), ref["backward_flow"])
        assert np.array_equal(np.array(Image.open(q("o.png"))), ref["occlusion"])
        assert np.array_equal(np.array(Image.open(q("ob.png"))), ref["occlusion_bwd"])
        assert np.array_equal(np.array(Image.open(q("w.png"))), ref["warped_rgb"])


@pytest.mark.parametrize("multseg", [False, True])
def test_para_gen_backward_and_occlusion(tmp_path, multseg):
    W, H = 96, 64
    inp, outp, mdir = tmp_path / "in", tmp_path / "out", tmp_path / "matches"
    for seq in ("a", "b"):
        os.makedirs(inp / "orgRGB" / seq); os.makedirs(inp / "orgMasks" / seq); os.makedirs(mdir / seq)
        fr = synth.make_frame(W, H, seed=len(seq) + ord(seq), K=2, fd=1)
        for n in range(3):
            Image.fromarray(fr["rgb"]).save(inp / "orgRGB" / seq / ("%05d.png" % n))
            Image.fromarray(fr["labels"].astype(np.uint8)).save(inp / "orgMasks" / seq / ("%05d.png" % n))
            (mdir / seq / ("%05d.txt" % n)).write_text("\n".join("%d %d %d %d 1.0 0" % tuple(c) for c in fr["constraints"]))
    flags = ["--bwd_flow"] + (["--multseg"] if multseg else ["--occ"])
    _run([sys.executable, osp.join(ROOT, "para_gen.py"), "--input", str(inp), "--output", str(outp), "--gpu", "0",
          "--fd", "1", "--matches", str(mdir)] + flags, str(tmp_path))
    lst = open(outp / "all_files.list").read().splitlines()
    ext = open(outp / "all_files_ext.list").read().splitlines()
    assert len(lst) == 4 and len(ext) == 4
    for ln, le in zip(lst, ext):
        t = le.split(" ")
        assert t[:3] == ln.split(" ") and len(t) == (5 if multseg else 6)
        bwd, obwd = flo.flow_read(t[3]), np.array(Image.open(t[4]))
        stem = osp.relpath(t[2], str(outp / "Flow"))[:-4]
        assert t[3] == str(outp / "FlowBwd" / (stem + ".flo")) and t[4] == str(outp / "OccBwd" / (stem + ".png"))
        wm = np.array(Image.open(str(outp / "wMasks" / (stem + ".png")))) != 0
        assert bwd.shape == (H, W, 2) and (bwd[~wm] == 0).all() and np.abs(bwd[wm]).max() > 0.5
        assert set(np.unique(obwd)) <= {0, 255} and not (obwd[wm] == 255).any()
        if not multseg:
            obj = np.array(Image.open(str(outp / "inpMasks" / (stem + ".png"))))[..., 0] == 0 \
                if np.array(Image.open(str(outp / "inpMasks" / (stem + ".png")))).ndim == 3 \
                else np.array(Image.open(str(outp / "inpMasks" / (stem + ".png")))) == 0
            assert np.array_equal(obwd == 255, obj & ~wm)
            occ = np.array(Image.open(t[5]))
            assert t[5] == str(outp / "Occ" / (stem + ".png")) and set(np.unique(occ)) <= {0, 255}
    assert not [f for f in os.listdir(outp / "FlowBwd" / "a") if "_seg" in f]
    # --resume: every requested output is there, nothing is redone
    out = _run([sys.executable, osp.join(ROOT, "para_gen.py"), "--input", str(inp), "--output", str(outp), "--gpu", "0",
                "--fd", "1", "--matches", str(mdir), "--resume"] + flags, str(tmp_path))
    assert "Scanning data to be processed\t\t0 files" in out
