"""Layered in-between frames on the GPU (DESIGN.md "Layered in-between frames"): opt.warp_layers_step bit for bit
against the numpy restatement (tests/layers_step_ref.py), against the one-layer step and the layered warp, a closed
form, solved segments, and through the `layers ... mid=` line of both arap_deform twins.  Every comparison is exact."""
import os
import os.path as osp
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import layers_step_ref as sref
import mid_ref
import occ_layers_ref as lref
import occ_ref
from arap_flow_amd import flo, opt, pipeline, synth

pytestmark = pytest.mark.gpu
ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))


def _same(a, b):
    """exact, NaN payloads included"""
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _check(r, ref):
    assert np.array_equal(r["warped_mask"], ref["warped_mask"])
    assert np.array_equal(r["step"], ref["step"], equal_nan=True)
    assert np.array_equal(r["occlusion_step"], ref["occlusion_step"])


@pytest.mark.parametrize("W,H,n,seed,overlap", sref.MULTI + sref.SINGLE)
def test_equals_restatement_repeat_and_single_outputs(gpu_state, W, H, n, seed, overlap):
    rgb, masks, fa, fb = sref.two_state_layers(W, H, n, seed, overlap=overlap)
    A, B = lref.fields_from_flows(fa), lref.fields_from_flows(fb)
    if n > 1:
        assert all(sref.exercised(masks, A, B).values())
    ref = sref.layers_step_ref(masks, A, B)
    r = opt.warp_layers_step(gpu_state, rgb, masks, fa, fb)
    _check(r, ref)
    lay = opt.warp_layers(gpu_state, rgb, masks, fa, occ=False)          # RGB and mask: the layered warp's
    assert _same(r["warped_rgb"], lay["warped_rgb"]) and _same(r["warped_mask"], lay["warped_mask"])
    again = opt.warp_layers_step(gpu_state, rgb, masks, fa, fb)          # two runs, identical bytes
    for k in ("warped_rgb", "warped_mask", "step", "occlusion_step"):
        assert _same(r[k], again[k]), k
    s = opt.warp_layers_step(gpu_state, None, masks, fa, fb, step=True, occ=False)     # each on its own; no RGB
    assert s["warped_rgb"] is None and "occlusion_step" not in s and _same(s["step"], r["step"])
    o = opt.warp_layers_step(gpu_state, None, masks, fa, fb, step=False, occ=True)
    assert "step" not in o and _same(o["occlusion_step"], r["occlusion_step"])
    m = opt.warp_layers_step(gpu_state, rgb, masks, fa, fb, step=False, occ=False)
    assert _same(m["warped_rgb"], lay["warped_rgb"]) and _same(m["warped_mask"], lay["warped_mask"])


@pytest.mark.parametrize("W,H,seed,kind", [(70, 50, 5, "folded"), (129, 65, 6, "smooth"), (2, 2, 7, "folded"),
                                           (1, 5, 8, "folded"), (5, 1, 9, "folded")])
def test_one_layer_equals_warp_step(gpu_state, W, H, seed, kind):
    if min(W, H) < 8:
        rgb, mask, fa = occ_ref.folded_case(W, H, 0.5, seed=seed)
        fb = occ_ref.folded_case(W, H, 0.7, seed=seed + 1)[2]
    else:
        rgb, mask, fa, fb = mid_ref.two_state_case(W, H, seed, kind)
    a = opt.warp_layers_step(gpu_state, rgb, mask[None], fa[None], fb[None])
    b = opt.warp_step(gpu_state, rgb, mask, fa, fb)
    for k in ("warped_rgb", "warped_mask", "step"):
        assert _same(a[k], b[k]), k


@pytest.mark.parametrize("W,H,n,seed,overlap", sref.MULTI[2:5])
def test_zero_second_state_equals_layered_backward_flow(gpu_state, W, H, n, seed, overlap):
    rgb, masks, fa, _ = sref.two_state_layers(W, H, n, seed, overlap=overlap)
    a = opt.warp_layers_step(gpu_state, rgb, masks, fa, np.zeros_like(fa), occ=False)
    b = opt.warp_layers(gpu_state, rgb, masks, fa, bwd=True, occ=False)
    assert _same(a["step"], b["backward_flow"])
    assert _same(a["warped_rgb"], b["warped_rgb"]) and _same(a["warped_mask"], b["warped_mask"])


def test_upper_rectangle_moves_over_resting_lower_one(gpu_state):
    """closed form: the expected set is asserted only because the sequential statement confirms it first, on the CPU"""
    masks, fa, fb, want = sref.rectangles_case()
    A, B = lref.fields_from_flows(fa), lref.fields_from_flows(fb)
    confirmed = np.array_equal(sref.layers_step_brute(masks, A, B)["occlusion_step"] == 255, want)
    got = opt.warp_layers_step(gpu_state, None, masks, fa, fb)["occlusion_step"]
    assert confirmed and np.array_equal(got == 255, want)
    assert set(np.unique(got)) <= {0, 255}


def _solved_segments(state, seed, schedule=(19, 1, 20), snaps=(6, 12)):
    """a three-segment 854x480 frame: per segment the snapshot flows after ramp steps `snaps` and the final flow of a
    short FrameSolver schedule; every layer but the top one shifted towards the next label's centroid, by a share of the
    way that grows from state to state, so that the warped layers pass over each other between the states"""
    W, H = 854, 480
    frame = synth.make_frame(W, H, seed, K=3, fd=2)
    segs = synth.segment_masks(frame)
    fs = opt.FrameSolver(state, W, H, batch=len(segs))
    try:
        fs.set_snapshots(list(snaps))
        for b, s in enumerate(segs):
            fs.set_frame(b, s["mask_red"], s["constraints"], rgb=frame["rgb"])
        fs.solve(len(segs), *schedule)
        fs.warp(len(segs))
        states = [np.stack([fs.snapshot(b, k, want_rgb=False)["flow"] for b in range(len(segs))])
                  for k in range(len(snaps))]
        states.append(np.stack([fs.results(b)["flow"] for b in range(len(segs))]))
    finally:
        fs.close()
    masks = np.stack([s["mask_red"] for s in segs])
    cen = [np.argwhere(m == 0).mean(0)[::-1] for m in masks]
    out = []
    for st, share in zip(states, (0.5, 0.7, 0.9)):
        st = np.array(st, np.float32)
        for l in range(len(masks) - 1):
            st[l][masks[l] == 0] += np.round(share * (cen[l + 1] - cen[l])).astype(np.float32)
        out.append(st)
    return frame["rgb"], masks, out


def test_three_solved_segments_854x480(gpu_state):
    rgb, masks, states = _solved_segments(gpu_state, 3)
    assert len(masks) == 3 and len(states) == 3
    for fa, fb in zip(states, states[1:]):                       # both links
        A, B = lref.fields_from_flows(fa), lref.fields_from_flows(fb)
        ref = sref.layers_step_ref(masks, A, B, parts=True)
        assert ref["higher"].any() and (ref["step"] != 0).any()
        _check(opt.warp_layers_step(gpu_state, rgb, masks, fa, fb), ref)


def test_bad_arguments(gpu_state):
    rgb, masks, fa, fb = sref.two_state_layers(10, 8, 2, 6)
    with pytest.raises(ValueError):
        opt.warp_layers_step(gpu_state, rgb, masks[:0], fa[:0], fb[:0])                 # n = 0
    with pytest.raises(ValueError):
        opt.warp_layers_step(gpu_state, rgb, np.repeat(masks, 128, 0), np.repeat(fa, 128, 0), np.repeat(fb, 128, 0))
    lib, h = gpu_state.lib, gpu_state.handle
    import torch
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    f = lib.ArapFlow_WarpLayersStep
    assert f(h, 10, 8, 2, p, p, p, p, None, None, None, None, p) == -1          # no output
    assert f(h, 10, 8, 2, None, p, p, p, p, p, None, None, p) == -1             # out_rgb without rgb
    assert f(h, 10, 8, 2, p, None, p, p, None, p, None, None, p) == -1          # no masks
    assert f(h, 10, 8, 2, p, p, p, None, None, p, p, None, p) == -1             # no second state
    assert f(h, 10, 8, 2, p, p, p, p, None, p, None, None, None) == -1          # no scratch
    assert f(h, 0, 8, 2, p, p, p, p, None, p, None, None, p) == -1
    assert f(h, 4097, 4096, 1, p, p, p, p, None, None, None, p, p) == -1        # out_occ with N > 2^24
    assert f(h, 65536, 32768, 1, p, p, p, p, None, p, None, None, p) == -1      # N = 2^31
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0                                                   # nothing ran
    N = 854 * 480
    assert lib.ArapFlow_WarpLayersStepScratchBytes(854, 480, 3) >= 48 * N + 4


def test_leaves_later_results_unchanged(gpu_state):
    lrgb, lmasks, lflows = lref.layered_case(129, 65, 5, 22, overlap=True)
    frame = synth.make_frame(96, 64, seed=5, fd=3)

    def others():
        w = opt.warp_layers(gpu_state, lrgb, lmasks, lflows, bwd=True, occ_bwd=True, occ=True)
        fs = opt.FrameSolver(gpu_state, 96, 64, batch=1)
        try:
            fs.set_frame(0, frame["mask_red"], frame["constraints"], rgb=frame["rgb"])
            fs.solve(1, 3, 2, 20)
            fs.warp(1)
            s = fs.results(0)
        finally:
            fs.close()
        return [w[k] for k in sorted(w)] + [s["flow"], s["warped_rgb"], s["warped_mask"], s["offset"], s["angle"]]

    before = others()
    rgb, masks, fa, fb = sref.two_state_layers(129, 65, 5, 1, overlap=True)
    opt.warp_layers_step(gpu_state, rgb, masks, fa, fb)
    after = others()
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()


# ----------------------------------------------------------------------------------------------------------------------
# the `layers ... mid=` line of both arap_deform twins, and para_gen.py --multseg --mid_layers
# ----------------------------------------------------------------------------------------------------------------------
def _run(args, cwd, stdin=None):
    env = dict(os.environ, HIP_VISIBLE_DEVICES=os.environ.get("HIP_VISIBLE_DEVICES", "0"))
    r = subprocess.run(args, cwd=cwd, env=env, input=stdin, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _read_mid(prefix, step, occ=True):
    f = pipeline.mid_files(prefix, step)
    out = dict(flow=flo.flow_read(f["flow"]), rgb=np.array(Image.open(f["rgb"])), mask=np.array(Image.open(f["mask"])),
               step=flo.flow_read(f["step"]))
    if occ:
        out["occ"] = np.array(Image.open(pipeline.mid_layer_files(prefix, step)["occ"]))
    return out


def test_layers_mid_line_both_twins_equal_the_api(tmp_path, gpu_state):
    from arap_flow_amd import build
    W, H, steps = 96, 64, (6, 12)
    frame = synth.make_frame(W, H, 9, K=2, fd=3)
    segs = synth.segment_masks(frame)
    assert len(segs) == 2
    fs = opt.FrameSolver(gpu_state, W, H, batch=2)
    try:
        fs.set_snapshots(list(steps))
        for b, s in enumerate(segs):
            fs.set_frame(b, s["mask_red"], s["constraints"], rgb=frame["rgb"])
        fs.solve(2, 19, 1, 20)
        fs.warp(2)
        states = [np.stack([fs.snapshot(b, k, want_rgb=False)["flow"] for b in range(2)]) for k in range(2)]
        states.append(np.stack([fs.results(b)["flow"] for b in range(2)]))
    finally:
        fs.close()
    masks = np.stack([s["mask_red"] for s in segs])
    cen = [np.argwhere(m == 0).mean(0)[::-1] for m in masks]
    for st, share in zip(states, (0.5, 0.8, 1.0)):               # the lower segment slides under the upper one
        st[0][masks[0] == 0] += np.round(share * (cen[1] - cen[0])).astype(np.float32)
    Image.fromarray(frame["rgb"]).save(tmp_path / "r.png")
    layers = []
    for l in range(2):
        Image.fromarray(np.stack([masks[l]] * 3, -1)).save(tmp_path / ("m%d.png" % l))
        stem = str(tmp_path / ("f%d" % l))
        flo.flow_write(stem + ".flo", states[2][l])
        for k, i in enumerate(steps):
            flo.flow_write(pipeline.mid_files(stem, i)["flow"], states[k][l])
        layers.append((str(tmp_path / ("m%d.png" % l)), stem + ".flo"))
    want = [opt.warp_layers_step(gpu_state, frame["rgb"], masks, states[k], states[k + 1]) for k in range(2)]
    first = opt.warp_layers(gpu_state, None, masks, states[0])["occlusion"]
    final = opt.warp_layers(gpu_state, None, masks, states[2])["occlusion"]
    assert any((w["occlusion_step"] == 255).any() for w in want)
    cpp = build.build_host()[0]
    got = {}
    for tag in ("py", "cpp", "serve"):
        prefix = str(tmp_path / (tag + "_mid"))
        out = dict(occ=str(tmp_path / (tag + "_occ.png")), mid=pipeline.mid_token(steps, prefix))
        line = pipeline.layers_line(pipeline.LayersLine(str(tmp_path / "r.png"), layers, out))
        if tag == "serve":
            said = _run([cpp, "--serve"], str(tmp_path), stdin=line + "\n")
            assert "Done " + out["occ"] in said.splitlines()
        else:
            (tmp_path / (tag + ".txt")).write_text(line + "\n")
            _run(([sys.executable, osp.join(ROOT, "arap_deform.py")] if tag == "py" else [cpp]) +
                 [str(tmp_path / (tag + ".txt"))], str(tmp_path))
        got[tag] = [_read_mid(prefix, i) for i in steps]
        assert np.array_equal(np.array(Image.open(out["occ"])), final)           # occ= keeps its meaning: frame 1 -> 2
        s00 = Image.open(pipeline.mid_layer_files(prefix, 0)["occ"])
        assert s00.mode == "L" and np.array_equal(np.array(s00), first)
        for k, i in enumerate(steps):
            g, w = got[tag][k], want[k]
            assert Image.open(pipeline.mid_layer_files(prefix, i)["occ"]).mode == "L"
            assert np.array_equal(g["flow"], pipeline.owner_flow(masks, states[k]))
            assert np.array_equal(g["rgb"], w["warped_rgb"]) and np.array_equal(g["mask"] != 0, w["warped_mask"] != 0)
            assert np.array_equal(g["step"], w["step"]) and np.array_equal(g["occ"], w["occlusion_step"])
            for key in g:
                assert _same(g[key], got["py"][k][key]), (tag, key)
    # a flow that is not named *.flo, or a missing snapshot, ends the run with a message
    os.rename(tmp_path / "f1_s12.flo", tmp_path / "gone.flo")
    bad = pipeline.layers_line(pipeline.LayersLine(str(tmp_path / "r.png"), layers, dict(mid=pipeline.mid_token(steps, str(tmp_path / "x")))))
    (tmp_path / "bad.txt").write_text(bad)
    env = dict(os.environ, HIP_VISIBLE_DEVICES=os.environ.get("HIP_VISIBLE_DEVICES", "0"))
    for prog in ([sys.executable, osp.join(ROOT, "arap_deform.py")], [cpp]):
        r = subprocess.run(prog + [str(tmp_path / "bad.txt")], cwd=str(tmp_path), env=env, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode != 0 and "f1_s12.flo" in r.stdout + r.stderr


@pytest.mark.parametrize("twin", ["cpp", "py"])
def test_para_gen_mid_layers(tmp_path, twin):
    from test_gpu_occ_layers import _para_gen, _tree
    inp, mdir = _tree(tmp_path)
    outp = tmp_path / "out"
    arap = [] if twin == "cpp" else ["--arap_bin", "%s %s" % (sys.executable, osp.join(ROOT, "arap_deform.py"))]
    _para_gen(tmp_path, inp, outp, mdir, ["--multseg"] + arap)
    plain_list = open(outp / "all_files.list", "rb").read()
    assert len(plain_list.splitlines()) == 4 and not (outp / "Mid").exists()
    import shutil
    shutil.rmtree(outp)
    flags = ["--multseg", "--mid_layers", "2", "--occ_layers"] + arap
    _para_gen(tmp_path, inp, outp, mdir, flags)
    assert open(outp / "all_files.list", "rb").read() == plain_list
    ext = open(outp / "all_files_ext.list").read().splitlines()
    assert len(ext) == 4
    for le in ext:
        t = le.split(" ")
        stem = osp.relpath(t[2], str(outp / "Flow"))[:-4]
        prefix = str(outp / "Mid" / stem)
        want = [pipeline.mid_files(prefix, i)[k] for i in (6, 12) for k in ("flow", "rgb", "mask", "step")]
        want += [pipeline.mid_layer_files(prefix, i)["occ"] for i in (0, 6, 12)]
        assert t[3:] == [str(outp / "Occ" / (stem + ".png"))] + want and all(osp.exists(q) for q in t)
        for i in (6, 12):
            m = _read_mid(prefix, i)
            assert m["flow"].shape == (64, 96, 2) and (m["flow"] != 0).any() and (m["step"][m["mask"] != 0] != 0).any()
            assert (m["step"][m["mask"] == 0] == 0).all() and set(np.unique(m["occ"])) <= {0, 255}
    for seq in ("a", "b"):                                       # the segments' snapshot files are gone
        assert not [f for f in os.listdir(outp / "Flow" / seq) if "_seg" in f]
        assert len(os.listdir(outp / "Mid" / seq)) == 2 * (8 + 3)
    out = _para_gen(tmp_path, inp, outp, mdir, flags + ["--resume"])
    assert "Scanning data to be processed\t\t0 files" in out
