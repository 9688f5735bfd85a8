"""Point tracks through the command-line tools (DESIGN.md "Point tracks"): one `trk` line through both arap_deform twins
(C++: list mode and --serve; arap_deform.py) against opt.track_points, and para_gen.py --tracks over --mid and over
--multseg --mid_layers, for both twins.  Every comparison is exact."""
import json
import os
import os.path as osp
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import layers_step_ref as sref
import track_ref as tref
from arap_flow_amd import flo, opt, pipeline, trk

pytestmark = pytest.mark.gpu
ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
PY_TWIN = [sys.executable, osp.join(ROOT, "arap_deform.py")]


def _run(args, cwd, stdin=None, ok=True):
    env = dict(os.environ, HIP_VISIBLE_DEVICES=os.environ.get("HIP_VISIBLE_DEVICES", "0"))
    r = subprocess.run(args, cwd=cwd, env=env, input=stdin, capture_output=True, text=True, timeout=600)
    assert (r.returncode == 0) == ok, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout + r.stderr


def test_trk_line_both_twins_equal_the_api(tmp_path, gpu_state):
    from arap_flow_amd import build
    W, H, n, T = 70, 50, 3, 3
    _, masks, fa, fb = sref.two_state_layers(W, H, n, 1)
    states = np.stack([fa * np.float32(0.5), fa, fb]).astype(np.float32)
    pts = tref.case_points(W, H, 1)
    p = lambda name: str(tmp_path / name)
    trk.write(p("pts.trk"), W, H, pts)
    layers = []
    for l in range(n):
        Image.fromarray(np.stack([masks[l]] * 3, -1)).save(p("m%d.png" % l))
        for s in range(T):
            flo.flow_write(p("f%d_%d.flo" % (l, s)), states[s, l])
        layers.append((p("m%d.png" % l), tuple(p("f%d_%d.flo" % (l, s)) for s in range(T))))
    want = opt.track_points(gpu_state, masks, states, pts)
    assert (want["occ"] == 255).any() and (want["occ"] == 0).any()
    cpp = build.build_host()[0]
    raw = {}
    for tag in ("py", "cpp", "serve"):
        item = pipeline.TrkLine(p("pts.trk"), layers, p(tag + "_out.trk"))
        line = pipeline.format_line(item)
        if tag == "serve":
            said = _run([cpp, "--serve"], str(tmp_path), stdin=line + "\n")
            assert "Done " + item.out in said.splitlines()
        else:
            (tmp_path / (tag + ".txt")).write_text(line + "\n")
            _run((PY_TWIN if tag == "py" else [cpp]) + [p(tag + ".txt")], str(tmp_path))
        raw[tag] = open(item.out, "rb").read()
        got = trk.read(item.out)
        assert (got["W"], got["H"]) == (W, H) and got["pos"].shape == (T + 1, len(pts), 2)
        assert got["pos"][0].tobytes() == pts.tobytes()
        assert np.array_equal(got["occ"][0], np.where(trk.in_frame(pts, W, H), 0, 255))
        assert got["pos"][1:].tobytes() == want["pos"].tobytes() and np.array_equal(got["occ"][1:], want["occ"])
    assert raw["py"] == raw["cpp"] == raw["serve"]
    # a truncated points file, a track file in the place of a points file, a missing state: a message, in both twins
    open(p("cut.trk"), "wb").write(open(p("pts.trk"), "rb").read()[:-3])
    bad_flo = list(layers)
    bad_flo[1] = (layers[1][0], (layers[1][1][0], p("gone.flo"), layers[1][1][2]))
    for name, item in (("cut.trk", pipeline.TrkLine(p("cut.trk"), layers, p("x.trk"))),
                       ("py_out.trk", pipeline.TrkLine(p("py_out.trk"), layers, p("x.trk"))),
                       ("gone.flo", pipeline.TrkLine(p("pts.trk"), bad_flo, p("x.trk")))):
        (tmp_path / "bad.txt").write_text(pipeline.format_line(item) + "\n")
        assert name in _run([cpp, p("bad.txt")], str(tmp_path), ok=False)
        with pytest.raises((ValueError, OSError)) as err:        # arap_deform.py ends with this message
            pipeline.run_tracks(gpu_state, item)
        assert name in str(err.value) and not osp.exists(p("x.trk"))


def _check_pair(gpu_state, outp, stem, layer_files, P, steps):
    """one pair's track file against the files of its states: layer_files = [(mask, flow, snapshot prefix)]"""
    import para_gen
    got = trk.read(str(outp / "Tracks" / (stem + ".trk")))
    masks = np.stack([pipeline.load_mask_red(m) for m, _, _ in layer_files])
    H, W = masks.shape[1:]
    assert (got["W"], got["H"]) == (W, H) and got["pos"].shape == (len(steps) + 2, P, 2)
    seq, frame = osp.split(stem)
    pts = pipeline.sample_track_points(random.Random(para_gen._pair_id(seq, frame)), P, W, H, masks)
    assert got["pos"][0].tobytes() == pts.tobytes() and (got["occ"][0] == 0).all()
    flows = np.stack([np.stack([flo.flow_read(pipeline.mid_files(prefix, i)["flow"]) for _, _, prefix in layer_files])
                      for i in steps] + [np.stack([flo.flow_read(f) for _, f, _ in layer_files])])
    want = opt.track_points(gpu_state, masks, flows, pts)
    assert got["pos"][1:].tobytes() == want["pos"].tobytes() and np.array_equal(got["occ"][1:], want["occ"])
    assert (got["pos"][-1] != pts).any()                         # the objects move
    return got


@pytest.mark.parametrize("twin", ["cpp", "py"])
@pytest.mark.parametrize("mode", ["mid", "mid_layers"])
def test_para_gen_tracks(tmp_path, gpu_state, twin, mode):
    from test_gpu_occ_layers import _para_gen, _tree
    inp, mdir = _tree(tmp_path)
    outp = tmp_path / "out"
    P, steps = 64, (6, 12)
    arap = [] if twin == "cpp" else ["--arap_bin", " ".join(PY_TWIN)]
    base = (["--mid", "2"] if mode == "mid" else ["--multseg", "--mid_layers", "2"]) + arap
    flags = base + ["--tracks", str(P)]
    kept = {}
    if mode == "mid_layers":                                     # the segments' files kept: the states the tracks were made of
        _para_gen(tmp_path, inp, outp, mdir, flags + ["--keep_segments"])
        for le in open(outp / "all_files_ext.list").read().splitlines():
            stem = osp.relpath(le.split(" ")[2], str(outp / "Flow"))[:-4]
            files = [(str(outp / "inpMasks" / ("%s_seg%d.png" % (stem, s))), str(outp / "Flow" / ("%s_seg%d.flo" % (stem, s))),
                      str(outp / "Flow" / ("%s_seg%d" % (stem, s)))) for s in (1, 2)]
            _check_pair(gpu_state, outp, stem, files, P, steps)
            kept[stem] = open(outp / "Tracks" / (stem + ".trk"), "rb").read()
        assert len(kept) == 4
        shutil.rmtree(outp)
    _para_gen(tmp_path, inp, outp, mdir, flags)
    plain = open(outp / "all_files.list").read().splitlines()    # unchanged: the pair's three files, nothing else
    stats = json.load(open(outp / "arap_stats.json"))
    assert stats["frames"] == 4 and stats["frames_done"] == 4 and stats["tracks_done"] == 4
    ext = open(outp / "all_files_ext.list").read().splitlines()
    assert len(ext) == 4
    for le, trio in zip(ext, plain):
        t = le.split(" ")
        stem = osp.relpath(t[2], str(outp / "Flow"))[:-4]
        assert " ".join(t[:3]) == trio and len(t) == 3 + 4 * len(steps) + 1
        assert t[-1] == str(outp / "Tracks" / (stem + ".trk"))   # listed, last
        assert all(osp.exists(q) for q in t)
        if mode == "mid":
            files = [(str(outp / "inpMasks" / (stem + ".png")), t[2], str(outp / "Mid" / stem))]
            _check_pair(gpu_state, outp, stem, files, P, steps)
        else:
            assert open(t[-1], "rb").read() == kept[stem]
            assert trk.read(t[-1])["pos"].shape == (4, P, 2)
    for seq in ("a", "b"):                                       # the segments' snapshots and the points files are gone
        assert not [f for f in os.listdir(outp / "Flow" / seq) if "_seg" in f]
        assert not [f for f in os.listdir(outp / "tmpCnstr" / seq) if f.endswith(".trk")]
        assert sorted(os.listdir(outp / "Tracks" / seq)) == ["00000.trk", "00001.trk"]
    out = _para_gen(tmp_path, inp, outp, mdir, flags + ["--resume"])
    assert "Scanning data to be processed\t\t0 files" in out
    if mode == "mid":                                            # --resume skips a pair only when its tracks exist as well
        os.remove(outp / "Tracks" / "a" / "00001.trk")
        out = _para_gen(tmp_path, inp, outp, mdir, flags + ["--resume"])
        assert "Scanning data to be processed\t\t1 files" in out and osp.exists(outp / "Tracks" / "a" / "00001.trk")
