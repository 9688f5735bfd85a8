"""GPU: the `bg` list line with mid= / mm= / mid_out= through both arap_deform twins (list file and --serve) and
para_gen.py --bg_motion --mid_bg (child processes), against the library call opt.background_seq on the decoded files."""
import os
import os.path as osp
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import bg_seq_ref
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


def _gray(path):
    im = Image.open(path)
    assert im.mode == "L", path
    return np.array(im)


def library_sequence(state, item):
    """opt.background_seq over the files a bg line names, decoded as the workers decode them -> {file: array}, keyed by
    the files of pipeline.mid_bg_files"""
    steps, prefix = pipeline.parse_mid(item.mid)
    files = [pipeline.mid_files(prefix, i) for i in steps]
    cover = lambda q: np.where(pipeline.load_mask_red(q) != 0, 255, 0).astype(np.uint8)
    covers = [None] + [cover(f["mask"]) for f in files] + [cover(item.mask2)]
    rgbs = [None] + [pipeline.load_rgb(f["rgb"]) for f in files] + [None]
    flows = [flo.flow_read(files[0]["flow"])] + [flo.flow_read(f["step"]) for f in files]
    occs = None
    if "occ" in item.inputs:
        occs = [_gray(pipeline.mid_layer_files(prefix, i)["occ"]) for i in (0,) + steps]
    maps = np.asarray(item.m[:6] + item.mm + item.m[6:], F).reshape(-1, 6)
    r = opt.background_seq(state, pipeline.load_rgb(item.bg), maps, pipeline.load_mask_red(item.mask1), covers, rgbs, flows, occs)
    out = {}
    for k, i in enumerate((0,) + steps):
        names = pipeline.mid_bg_files(item.mid_out, i)
        if k:
            out[names["rgb"]] = r["out_rgb"][k]
        out[names["step"]] = r["flow_full"][k]
        if occs is not None:
            out[names["occ"]] = r["occ_full"][k]
    assert r["out_rgb"][0] is None and r["out_rgb"][-1] is None
    return out, dict(covers=covers, flows=flows, maps=maps)


def assert_files_equal(want):
    for path, a in want.items():
        assert osp.exists(path), path
        got = flo.flow_read(path) if path.endswith(".flo") else _gray(path) if a.ndim == 2 else pipeline.load_rgb(path)
        assert got.dtype == a.dtype and got.tobytes() == a.tobytes(), path


def test_bg_line_sequence_both_twins_equal_library(tmp_path, gpu_state):
    c = bg_seq_ref.sized_case("67x9")                       # four frames: frame 1, the snapshots after steps 4 and 9, frame 2
    steps = (4, 9)
    p = lambda n: str(tmp_path / n)
    Image.fromarray(c["bg"]).save(p("bg.png"))
    Image.fromarray(c["rgbs"][0]).save(p("r1.png"))
    Image.fromarray(np.stack([c["mask_red"]] * 3, -1)).save(p("m1.png"))
    Image.fromarray(c["rgbs"][3]).save(p("r2.png"))
    pipeline.save_mask(c["covers"][3], p("m2.png"))
    pair_flow = (c["flows"][0] * F(3)).astype(F)
    flo.flow_write(p("f.flo"), pair_flow)
    pipeline.save_occ(c["occs"][0], p("occ.png"))
    flo.flow_write(pipeline.mid_files(p("mid"), steps[0])["flow"], c["flows"][0])
    pipeline.save_occ(c["occs"][0], pipeline.mid_layer_files(p("mid"), 0)["occ"])
    for k, i in enumerate(steps, 1):
        f = pipeline.mid_files(p("mid"), i)
        Image.fromarray(c["rgbs"][k]).save(f["rgb"])
        pipeline.save_mask(c["covers"][k], f["mask"])
        flo.flow_write(f["step"], c["flows"][k])
        pipeline.save_occ(c["occs"][k], pipeline.mid_layer_files(p("mid"), i)["occ"])
    M = c["maps"]
    pair = opt.background(gpu_state, c["bg"], M[0], M[3], c["rgbs"][0], c["mask_red"], c["rgbs"][3], c["covers"][3], pair_flow,
                          occ=c["occs"][0])
    cpp = build.build_host()[0]
    runs = (("py", [sys.executable, osp.join(ROOT, "arap_deform.py")], False), ("cpp", [cpp], False), ("srv", [cpp], True))

    def line(tag, occ=True, seq=True, out=True, prefix="mid"):
        q = lambda n: p(tag + "_" + n)
        return pipeline.BgLine(p("bg.png"), p("r1.png"), p("m1.png"), p("r2.png"), p("m2.png"), p("f.flo"),
                               m=tuple(float(v) for v in np.concatenate([M[0], M[3]])),
                               inputs=dict(occ=p("occ.png")) if occ else {},
                               out=(q("o1.png"), q("o2.png"), q("ff.flo")) if out else ("", "", ""),
                               outs=dict(occ_out=q("of.png")) if occ and out else {},
                               mid=pipeline.mid_token(steps, p(prefix)) if seq else "",
                               mm=tuple(float(v) for v in np.concatenate([M[1], M[2]])) if seq else (),
                               mid_out=q("full") if seq else "")

    tw = bg_seq_ref.background_seq(c["bg"], M, [opt.background_maps(M[f], M[f + 1])[0] for f in range(3)], c["mask_red"],
                                   c["covers"], c["rgbs"], c["flows"], c["occs"])
    written = lambda tag: sorted(f for f in os.listdir(tmp_path) if f.startswith(tag + "_"))
    # one process per program: the whole line; the sequence alone, without occ=; a line without the new tokens; and, in a
    # list, a line whose snapshots do not exist, which ends the run with a message
    for tag, prog, serve in runs:
        full, alone, old = line(tag + "a"), line(tag + "n", occ=False, out=False), line(tag + "o", seq=False)
        gone = line(tag + "g", prefix="gone")
        text = "".join(pipeline.format_line(it) + "\n" for it in (full, alone, old) + (() if serve else (gone,)))
        if serve:
            out = _run(prog + ["--serve"], str(tmp_path), stdin=text)
            assert all("Done " + pipeline.done_token(it) in out.splitlines() for it in (full, alone, old))
        else:
            (tmp_path / (tag + ".txt")).write_text(text)
            r = subprocess.run(prog + [p(tag + ".txt")], cwd=str(tmp_path), env=_env(), capture_output=True, text=True, timeout=600)
            assert r.returncode != 0 and "gone_s04" in r.stdout + r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
        want, _ = library_sequence(gpu_state, full)
        assert sorted(want) == sorted(pipeline.bg_outputs(full)[4:]) and len(want) == 2 + 3 + 3
        assert_files_equal(want)
        for k, i in enumerate((0,) + steps):                # the twin, on the arrays the files were written from
            names = pipeline.mid_bg_files(full.mid_out, i)
            assert want[names["step"]].tobytes() == tw["flow_full"][k].tobytes()
            assert want[names["occ"]].tobytes() == tw["occ_full"][k].tobytes()
            assert k == 0 or want[names["rgb"]].tobytes() == tw["out_rgb"][k].tobytes()
        # the pair's own outputs beside them, as without the tokens
        for it, t in ((full, tag + "a"), (old, tag + "o")):
            assert_files_equal({it.out[0]: pair["out_rgb1"], it.out[1]: pair["out_rgb2"], it.out[2]: pair["flow_full"],
                                it.outs["occ_out"]: pair["occ_full"]})
            assert written(t) == sorted(osp.basename(q) for q in pipeline.bg_outputs(it))
        assert len(written(tag + "o")) == 4                 # a line without the new tokens writes what it wrote before
        # without occ= no link occlusion is read or written; the sequence alone is an output
        want, _ = library_sequence(gpu_state, alone)
        assert len(want) == 2 + 3
        assert_files_equal(want)
        assert written(tag + "n") == sorted(osp.basename(q) for q in want)
    # a malformed line fails a list run
    (tmp_path / "bad.txt").write_text(pipeline.format_line(line("bad")).replace(" mid_out=", " mid_gone=") + "\n")
    assert subprocess.run([cpp, p("bad.txt")], cwd=str(tmp_path), env=_env(), capture_output=True).returncode == 1


# ---- para_gen.py --mid_bg ----------------------------------------------------------------------------------------------
def _tree(tmp_path):
    """the 96x64 three-frame input of test_gpu_background_cli.test_para_gen_bg_motion"""
    W, H = 96, 64
    inp, mdir, bgd = tmp_path / "in", tmp_path / "matches", tmp_path / "bgs"
    os.makedirs(inp / "orgRGB" / "a"); os.makedirs(inp / "orgMasks" / "a"); os.makedirs(mdir / "a"); os.makedirs(bgd)
    fr = synth.make_frame(W, H, seed=98, K=2, fd=1)
    for n in range(3):                                                      # three frames: two pairs
        Image.fromarray(fr["rgb"]).save(inp / "orgRGB" / "a" / ("%05d.png" % n))
        Image.fromarray(fr["labels"].astype(np.uint8)).save(inp / "orgMasks" / "a" / ("%05d.png" % n))
        (mdir / "a" / ("%05d.txt" % n)).write_text("\n".join("%d %d %d %d 1.0 0" % tuple(c) for c in fr["constraints"]))
    Image.fromarray(np.random.default_rng(1).integers(0, 256, (140, 220, 3)).astype(np.uint8)).save(bgd / "one.png")
    return [sys.executable, osp.join(ROOT, "para_gen.py"), "--input", str(inp), "--gpu", "0", "--fd", "1", "--matches",
            str(mdir), "--bg_dir", str(bgd), "--jobs", "2"]


def _check_para_gen(tmp_path, gpu_state, flags, occ):
    base = _tree(tmp_path)
    outp = tmp_path / "out"
    _run(base + ["--output", str(outp)] + flags, str(tmp_path))
    steps = tuple(pipeline.mid_steps(2, 19))
    lst = open(outp / "all_files.list").read().splitlines()
    ext = open(outp / "all_files_ext.list").read().splitlines()
    assert len(lst) == 2 and len(ext) == 2
    between = 0
    for ln, le in zip(lst, ext):
        t = le.split(" ")
        assert t[:3] == ln.split(" ") and all(osp.exists(q) for q in t)
        stem = osp.relpath(t[2], str(outp / "Flow"))[:-4]
        item = pipeline.parse_line(open(outp / "tmpCnstr" / (stem + "_bg.txt")).read())
        assert isinstance(item, pipeline.BgLine) and item.mid == pipeline.mid_token(steps, str(outp / "Mid" / stem))
        assert item.mid_out == str(outp / "MidFull" / stem) and ("occ" in item.inputs) == occ
        # the list's last columns: the files of the sequence, in bg_outputs' order
        full = pipeline.bg_outputs(item)[-(2 + 3 + (3 if occ else 0)):]
        assert t[-len(full):] == full and all(q.startswith(str(outp / "MidFull") + os.sep) for q in full)
        assert sorted(os.listdir(outp / "MidFull" / osp.dirname(stem))) == sorted(
            osp.basename(q) for e in ext for q in e.split(" ") if (os.sep + "MidFull" + os.sep) in q)
        want, inp = library_sequence(gpu_state, item)
        assert sorted(want) == sorted(full)
        assert_files_equal(want)
        # on the objects every link's full flow is the object-side flow; off them it is the camera's
        own = [pipeline.load_mask_red(item.mask1) == 0] + [cv != 0 for cv in inp["covers"][1:-1]]
        for k, i in enumerate((0,) + steps):
            got = flo.flow_read(pipeline.mid_bg_files(item.mid_out, i)["step"])
            assert own[k].any() and np.array_equal(got[own[k]], inp["flows"][k][own[k]])
        # the in-between frames keep their object-side files: nothing composited onto OUT/Mid
        for k, i in enumerate(steps, 1):
            obj_side = pipeline.load_rgb(pipeline.mid_files(str(outp / "Mid" / stem), i)["rgb"])
            comp = pipeline.load_rgb(pipeline.mid_bg_files(item.mid_out, i)["rgb"])
            assert np.array_equal(comp[own[k]], obj_side[own[k]]) and not np.array_equal(comp, obj_side)
        # the cameras: the fractions i / 19 of the pair's motion, from the pair's own draws
        M = inp["maps"]
        assert M.shape == (4, 6) and M[0].tolist()[:2] == [1, 0]
        ang = [float(np.arctan2(Mk[3], Mk[0])) for Mk in M]                      # M1 is a translation: the rotation so far
        between += ang[0] == 0 and (0 < ang[1] < ang[2] < ang[3] or 0 > ang[1] > ang[2] > ang[3])
    assert between >= 1
    # --resume: every requested output is there, nothing is redone; with a MidFull file gone the pair is redone
    out = _run(base + ["--output", str(outp), "--resume"] + flags, str(tmp_path))
    assert "Scanning data to be processed\t\t0 files" in out
    os.remove(ext[0].split(" ")[-1])
    out = _run(base + ["--output", str(outp), "--resume"] + flags, str(tmp_path))
    assert "Scanning data to be processed\t\t1 files" in out


def test_para_gen_mid_bg(tmp_path, gpu_state):
    _check_para_gen(tmp_path, gpu_state, ["--mid", "2", "--bg_motion", "--mid_bg", "--keep_segments"], occ=False)


def test_para_gen_mid_layers_bg(tmp_path, gpu_state):
    _check_para_gen(tmp_path, gpu_state, ["--multseg", "--mid_layers", "2", "--occ_layers", "--bg_motion", "--mid_bg",
                                          "--keep_segments"], occ=True)
