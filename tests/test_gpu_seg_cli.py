"""GPU: the `seg` list line through both arap_deform twins (list file and --serve) and para_gen.py --seg (child
processes), against opt.seg_maps on the files those runs wrote."""
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
KEYS = pipeline.SEG_KEYS


def _env():
    return dict(os.environ, HIP_VISIBLE_DEVICES=os.environ.get("HIP_VISIBLE_DEVICES", "0"))


def _run(args, cwd, stdin=None):
    r = subprocess.run(args, cwd=cwd, env=_env(), capture_output=True, text=True, timeout=600, input=stdin)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _as_files(r):
    """opt.seg_maps' arrays as a seg line's files show them"""
    return {k: pipeline.seg_dist_png(a) if k.startswith("dist") else a for k, a in r.items()}


def test_solve_lines_then_a_seg_line_both_twins_equal_seg_maps(tmp_path, gpu_state):
    """a frame of two segments: its two solve lines and the frame's seg line over the flows they write in one list through
    the C++ worker; then the same seg line through --serve and through arap_deform.py"""
    W, H = 96, 64
    fr = synth.make_frame(W, H, seed=98, K=2, fd=1)
    p = lambda n: str(tmp_path / n)
    Image.fromarray(fr["rgb"]).save(p("r.png"))
    m = tuple(float(v) for v in np.concatenate([bg_ref.similarity(2.0, 1.02, (2.0, 1.0), (W / 2, H / 2)),
                                                bg_ref.similarity(-1.5, 0.99, (3.5, 2.25), (W / 2, H / 2))]))
    segs = pipeline.split_segments(fr["labels"].astype(np.uint8), [int(fr["labels"][c[1], c[0]]) for c in fr["constraints"]])
    assert len(segs) == 2
    for s, mask in segs:
        Image.fromarray(mask).save(p("m%d.png" % s))
        rows = [tuple(c) for c in fr["constraints"] if fr["labels"][c[1], c[0]] == s]
        pipeline.write_constraints(p("c%d.txt" % s), rows)
    masks = np.stack([mask for _, mask in segs])
    cpp = build.build_host()[0]
    solves = [pipeline.SolveLine(p("r.png"), p("m%d.png" % s), p("c%d.txt" % s), p("f%d.flo" % s), p("w%d.png" % s),
                                 p("wm%d.png" % s), extra={}) for s, _ in segs]
    item = lambda tag: pipeline.SegLine([(ln.mask, ln.flow) for ln in solves], 1.0, 16, m, {k: p("%s_%s.png" % (tag, k)) for k in KEYS})
    (tmp_path / "cpp.txt").write_text("\n".join([pipeline.format_line(ln) for ln in solves] + [pipeline.format_line(item("cpp"))]) + "\n")
    _run([cpp, p("cpp.txt")], str(tmp_path))
    out = _run([cpp, "--serve"], str(tmp_path), stdin=pipeline.format_line(item("srv")) + "\n")
    assert "Done " + p("srv_idx1.png") in out.splitlines() and pipeline.done_token(item("srv")) == p("srv_idx1.png")
    (tmp_path / "py.txt").write_text(pipeline.format_line(item("py")) + "\n")
    _run([sys.executable, osp.join(ROOT, "arap_deform.py"), p("py.txt")], str(tmp_path))
    flows = np.stack([flo.flow_read(ln.flow) for ln in solves])
    want = _as_files(opt.seg_maps(gpu_state, masks, flows, tau=1.0, radius=16, M1=m[:6], M2=m[6:]))
    for k in KEYS:
        for tag in ("cpp", "srv", "py"):
            im = Image.open(p("%s_%s.png" % (tag, k)))
            assert im.mode == "L" and np.array_equal(np.array(im), want[k]), (tag, k)
        assert filecmp.cmp(p("cpp_%s.png" % k), p("srv_%s.png" % k), shallow=False), k       # one encoder: the same file
    assert set(np.unique(want["idx1"])) == {0, 1, 2} and set(np.unique(want["idx2"])) >= {0, 1}
    assert set(np.unique(want["mb1"])) == {0, 255} and (want["dist1"] == 0).any()
    assert ((want["dist1"] > 0) & (want["dist1"] <= 16)).any()
    # a line that asks for one map alone writes nothing else; without m= the background is static
    one = pipeline.SegLine([(ln.mask, ln.flow) for ln in solves], 0.5, 254, (), dict(dist2=p("only_d2.png")))
    (tmp_path / "only.txt").write_text(pipeline.format_line(one) + "\n")
    _run([cpp, p("only.txt")], str(tmp_path))
    d2 = opt.seg_maps(gpu_state, masks, flows, tau=0.5, radius=254, which=("dist2",))["dist2"]
    assert np.array_equal(np.array(Image.open(p("only_d2.png"))), pipeline.seg_dist_png(d2))
    assert [f for f in os.listdir(tmp_path) if f.startswith("only_")] == ["only_d2.png"]
    # a malformed seg line fails a list run
    (tmp_path / "bad.txt").write_text("seg 1 m f idx1=x\n")
    assert subprocess.run([cpp, p("bad.txt")], cwd=str(tmp_path), env=_env(), capture_output=True).returncode == 1


@pytest.mark.parametrize("multseg", [False, True], ids=["plain", "multseg-bg_motion"])
def test_para_gen_seg(tmp_path, gpu_state, multseg):
    W, H = 96, 64
    inp, mdir, bgd = tmp_path / "in", tmp_path / "matches", tmp_path / "bgs"
    os.makedirs(inp / "orgRGB" / "a"); os.makedirs(inp / "orgMasks" / "a"); os.makedirs(mdir / "a"); os.makedirs(bgd)
    fr = synth.make_frame(W, H, seed=98, K=2, fd=1)
    for n in range(3):                                                      # three frames: two pairs
        Image.fromarray(fr["rgb"]).save(inp / "orgRGB" / "a" / ("%05d.png" % n))
        Image.fromarray(fr["labels"].astype(np.uint8)).save(inp / "orgMasks" / "a" / ("%05d.png" % n))
        (mdir / "a" / ("%05d.txt" % n)).write_text("\n".join("%d %d %d %d 1.0 0" % tuple(c) for c in fr["constraints"]))
    Image.fromarray(np.random.default_rng(1).integers(0, 256, (140, 220, 3)).astype(np.uint8)).save(bgd / "one.png")
    outp = tmp_path / "out"
    _run([sys.executable, osp.join(ROOT, "para_gen.py"), "--input", str(inp), "--output", str(outp), "--gpu", "0", "--fd", "1",
          "--matches", str(mdir), "--jobs", "2", "--keep_segments", "--seg", "1", "24"] +
         (["--multseg", "--bg_dir", str(bgd), "--bg_motion"] if multseg else []), str(tmp_path))
    pairs = open(outp / "all_files.list").read().splitlines()
    assert len(pairs) == 2
    dirs = dict(idx1="Index1", idx2="Index2", mb1="MB", mb2="MBBwd", dist1="MBDist", dist2="MBDistBwd")
    for k, pair in enumerate(pairs):
        stem = "%05d" % k
        flow = pair.split(" ")[2]
        assert flow == str(outp / "Flow" / "a" / (stem + ".flo"))
        M1 = M2 = None
        if multseg:                                                         # the solved layers and the bg line's camera
            seg = lambda d, ext: sorted(str(outp / d / "a" / f) for f in os.listdir(outp / d / "a") if f.startswith(stem + "_seg") and f.endswith(ext))
            mask_files, flow_files = seg("inpMasks", ".png"), seg("Flow", ".flo")
            assert len(mask_files) == len(flow_files) == 2
            line = pipeline.parse_line(open(outp / "tmpCnstr" / "a" / (stem + "_bg.txt")).read())
            M1, M2 = line.m[:6], line.m[6:]
            assert M1 != M2
        else:
            mask_files, flow_files = [str(outp / "inpMasks" / "a" / (stem + ".png"))], [flow]
        masks = np.stack([pipeline.load_mask_red(f) for f in mask_files])
        flows = np.stack([flo.flow_read(f) for f in flow_files])
        want = _as_files(opt.seg_maps(gpu_state, masks, flows, tau=1.0, radius=24, M1=M1, M2=M2))
        for key, d in dirs.items():
            im = Image.open(outp / d / "a" / (stem + ".png"))
            assert im.mode == "L" and np.array_equal(np.array(im), want[key]), (stem, key)
        assert set(np.unique(want["idx1"])) == ({0, 1, 2} if multseg else {0, 1}) and (want["mb1"] == 255).any()
