"""Layered warp on the GPU (DESIGN.md "Layered warp"): opt.warp_layers bit for bit against the numpy restatement
(tests/occ_layers_ref.py), against the single-layer entry and the host merges of n single-layer calls, a closed form,
and through para_gen.py --multseg --occ_layers with both arap_deform twins.  Every comparison is exact."""
import json
import os
import os.path as osp
import shutil
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import occ_layers_ref as lref
import occ_ref
from arap_flow_amd import flo, opt, pipeline, synth

pytestmark = pytest.mark.gpu
ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
KEYS = ("warped_rgb", "warped_mask", "backward_flow", "occlusion_bwd", "occlusion")


def _all(state, rgb, masks, flows):
    return opt.warp_layers(state, rgb, masks, flows, bwd=True, occ_bwd=True, occ=True)


def _exercises_the_rule(masks, fields, ref):
    """the condition on every multi-layer input, from the reference alone: the cross-layer map is not the union of the
    layers' own maps"""
    return bool((ref["occlusion"] != lref.union_of_single(masks, fields)).any())


SMALL = [(10, 8, 3, 2, False), (12, 7, 4, 3, False), (10, 8, 3, 4, True), (70, 50, 3, 21, False), (129, 65, 5, 22, True),
         (200, 150, 2, 23, False), (64, 4, 2, 24, False)]


@pytest.mark.parametrize("W,H,n,seed,overlap", SMALL)
def test_warp_layers_equals_restatement(gpu_state, W, H, n, seed, overlap):
    rgb, masks, flows = lref.layered_case(W, H, n, seed, overlap=overlap)
    fields = lref.fields_from_flows(flows)
    ref = lref.layers_ref(rgb, masks, fields)
    assert _exercises_the_rule(masks, fields, ref)
    r = _all(gpu_state, rgb, masks, flows)
    for k in KEYS:
        assert np.array_equal(r[k], ref[k]), k
    again = _all(gpu_state, rgb, masks, flows)                   # two runs, identical bytes
    for k in KEYS:
        assert r[k].tobytes() == again[k].tobytes(), k
    only = opt.warp_layers(gpu_state, None, masks, flows)       # each output on its own; no RGB
    assert only["warped_rgb"] is None and "backward_flow" not in only and "occlusion_bwd" not in only
    assert np.array_equal(only["occlusion"], ref["occlusion"]) and np.array_equal(only["warped_mask"], ref["warped_mask"])
    back = opt.warp_layers(gpu_state, rgb, masks, flows, bwd=True, occ=False)
    assert "occlusion" not in back and np.array_equal(back["backward_flow"], ref["backward_flow"])


def _solved_segments(state, seed):
    """a three-segment 854x480 frame: per-segment flows of a short FrameSolver schedule, plus a whole-pixel shift of every
    layer but the top one most of the way towards the next label's centroid, so that the warped layers overlap (synth's
    ellipses are disjoint and move a few pixels only; the flows are inputs of the entry, any field is legitimate)"""
    W, H = 854, 480
    frame = synth.make_frame(W, H, seed, K=3, fd=2)
    segs = synth.segment_masks(frame)
    fs = opt.FrameSolver(state, W, H, batch=len(segs))
    try:
        for b, s in enumerate(segs):
            fs.set_frame(b, s["mask_red"], s["constraints"], rgb=frame["rgb"])
        fs.solve(len(segs), 3, 2, 20)
        fs.warp(len(segs))
        flows = np.stack([fs.results(b)["flow"] for b in range(len(segs))])
    finally:
        fs.close()
    masks = np.stack([s["mask_red"] for s in segs])
    return frame["rgb"], masks, _shift_towards_next(masks, flows)


def _shift_towards_next(masks, flows):
    flows = np.array(flows, np.float32)
    cen = [np.argwhere(m == 0).mean(0)[::-1] for m in masks]     # (x, y) centroids
    for l in range(len(masks) - 1):
        d = np.round(0.8 * (cen[l + 1] - cen[l])).astype(np.float32)
        flows[l][masks[l] == 0] += d
    return flows


@pytest.mark.parametrize("seed", [3, 7])
def test_three_solved_segments_854x480(gpu_state, seed):
    rgb, masks, flows = _solved_segments(gpu_state, seed)
    assert len(masks) == 3
    fields = lref.fields_from_flows(flows)
    ref = lref.layers_ref(rgb, masks, fields)
    assert _exercises_the_rule(masks, fields, ref)
    r = _all(gpu_state, rgb, masks, flows)
    for k in KEYS:
        assert np.array_equal(r[k], ref[k]), k
    per = [opt.warp_image_ex(gpu_state, rgb, masks[l], flows[l]) for l in range(3)]
    m = lref.host_merge(per, masks)
    for k in ("warped_rgb", "warped_mask", "backward_flow", "occlusion_bwd"):
        assert np.array_equal(r[k], m[k]), k


@pytest.mark.parametrize("W,H,amp", [(70, 50, 3.0), (2, 2, 0.5), (1, 5, 1.0), (854, 480, 2.0)])
def test_one_layer_equals_warp_image_ex(gpu_state, W, H, amp):
    rgb, mask, fl = occ_ref.folded_case(W, H, amp)
    a = _all(gpu_state, rgb, mask[None], fl[None])
    b = opt.warp_image_ex(gpu_state, rgb, mask, fl)
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("W,H,n,seed,overlap", SMALL[3:6])
def test_composite_equals_host_merge_of_single_calls(gpu_state, W, H, n, seed, overlap):
    rgb, masks, flows = lref.layered_case(W, H, n, seed, overlap=overlap)
    r = _all(gpu_state, rgb, masks, flows)
    per = [opt.warp_image_ex(gpu_state, rgb, masks[l], flows[l]) for l in range(n)]
    m = lref.host_merge(per, masks)
    for k in ("warped_rgb", "warped_mask", "backward_flow", "occlusion_bwd"):
        assert np.array_equal(r[k], m[k]), k


def test_leaves_later_results_unchanged(gpu_state):
    rgb, mask, fl = occ_ref.folded_case(129, 65, 4.0)
    frame = synth.make_frame(96, 64, seed=5, fd=3)

    def others():
        w = opt.warp_image_ex(gpu_state, rgb, mask, fl)
        fs = opt.FrameSolver(gpu_state, 96, 64, batch=1)
        try:
            fs.set_frame(0, frame["mask_red"], frame["constraints"], rgb=frame["rgb"])
            fs.solve(1, 3, 2, 20)
            fs.warp(1)
            s = fs.results(0)
        finally:
            fs.close()
        return [w[k] for k in KEYS] + [s["flow"], s["warped_rgb"], s["warped_mask"], s["offset"], s["angle"]]

    before = others()
    lrgb, masks, flows = lref.layered_case(129, 65, 5, 22, overlap=True)
    _all(gpu_state, lrgb, masks, flows)
    after = others()
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()


def test_bad_arguments(gpu_state):
    rgb, masks, flows = lref.layered_case(10, 8, 2, 6)
    with pytest.raises(ValueError):
        opt.warp_layers(gpu_state, rgb, masks[:0], flows[:0])                         # n = 0
    with pytest.raises(ValueError):
        opt.warp_layers(gpu_state, rgb, np.repeat(masks, 128, 0), np.repeat(flows, 128, 0))     # n = 256
    lib = gpu_state.lib
    import torch
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    assert lib.ArapFlow_WarpLayers(gpu_state.handle, 10, 8, 2, p, p, p, None, None, None, None, None, p) == -1   # no output
    assert lib.ArapFlow_WarpLayers(gpu_state.handle, 4097, 4096, 1, p, p, p, None, None, None, None, p, p) == -1  # N > 2^24
    assert lib.ArapFlow_WarpLayers(gpu_state.handle, 65536, 32768, 1, p, p, p, None, p, None, None, None, p) == -1  # N = 2^31


def test_upper_rectangle_over_resting_lower_one(gpu_state):
    """closed form: the expected set is the sequential statement's; that it is the lower layer's vertices inside the
    closed translated rectangle is asserted only because the sequential statement confirms it first, on the CPU"""
    W, H = 16, 12
    masks = np.full((2, H, W), 255, np.uint8)
    masks[0, 2:10, 1:9] = 0
    masks[1, 3:9, 10:15] = 0
    flows = np.zeros((2, H, W, 2), np.float32)
    flows[1][masks[1] == 0] = (-6.0, -1.0)                       # lands on x 4..8, y 2..7
    fields = lref.fields_from_flows(flows)
    want = lref.layers_brute(None, masks, fields)["occlusion"]
    ys, xs = np.mgrid[0:H, 0:W]
    rect = (masks[0] == 0) & (xs >= 4) & (xs <= 8) & (ys >= 2) & (ys <= 7)
    confirmed = np.array_equal(want == 255, rect)
    assert (want != lref.union_of_single(masks, fields)).any()
    got = opt.warp_layers(gpu_state, None, masks, flows)["occlusion"]
    assert np.array_equal(got, want)
    assert confirmed and np.array_equal(got == 255, rect)


# ----------------------------------------------------------------------------------------------------------------------
# para_gen.py --multseg --occ_layers
# ----------------------------------------------------------------------------------------------------------------------
def _disc(W, H, cx, cy, r):
    ys, xs = np.mgrid[0:H, 0:W]
    return (xs - cx) ** 2 + (ys - cy) ** 2 <= r * r


def _tree(tmp_path):
    """two sequences of three frames, two labels: label 1 travels 10 pixels a frame to the right and slides UNDER the
    resting label 2 (drawn on top).  The matches carry label 1 along (and nudge label 2 by one pixel: a match must
    move), so the solved segment 1 lands partly beneath segment 2: the run shows one object passing over the other,
    not plumbing alone -- the test asserts that from the outputs."""
    W, H = 96, 64
    inp, mdir = tmp_path / "in", tmp_path / "matches"
    for si, seq in enumerate(("a", "b")):
        os.makedirs(inp / "orgRGB" / seq); os.makedirs(inp / "orgMasks" / seq); os.makedirs(mdir / seq)
        rgb = synth.make_rgb(W, H, 40 + si)
        labels = []
        for n in range(3):
            lab = np.zeros((H, W), np.uint8)
            lab[_disc(W, H, 36 + 10 * n, 30 + 2 * si, 13)] = 1
            lab[_disc(W, H, 66, 34, 13)] = 2
            labels.append(lab)
            Image.fromarray(rgb).save(inp / "orgRGB" / seq / ("%05d.png" % n))
            Image.fromarray(lab).save(inp / "orgMasks" / seq / ("%05d.png" % n))
        for n in range(3):
            rows = []
            if n + 1 < 3:
                for y in range(2, H - 2, 4):
                    for x in range(2, W - 2, 4):
                        for lab, (dx, dy) in ((1, (10, 0)), (2, (1, 0))):
                            if labels[n][y, x] == lab and labels[n + 1][y + dy, x + dx] == lab:
                                rows.append("%d %d %d %d 1.0 0" % (x, y, x + dx, y + dy))
            (mdir / seq / ("%05d.txt" % n)).write_text("\n".join(rows))
    return inp, mdir


def _para_gen(tmp_path, inp, outp, mdir, flags):
    env = dict(os.environ, HIP_VISIBLE_DEVICES=os.environ.get("HIP_VISIBLE_DEVICES", "0"))
    r = subprocess.run([sys.executable, osp.join(ROOT, "para_gen.py"), "--input", str(inp), "--output", str(outp), "--gpu",
                        "0", "--fd", "1", "--matches", str(mdir), "--jobs", "4"] + flags, cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_para_gen_occ_layers_both_twins(tmp_path, gpu_state):
    inp, mdir = _tree(tmp_path)
    outp = tmp_path / "out"
    _para_gen(tmp_path, inp, outp, mdir, ["--multseg", "--bwd_flow"])
    plain_list = open(outp / "all_files.list", "rb").read()
    assert len(plain_list.splitlines()) == 4 and not (outp / "Occ").exists()
    shutil.rmtree(outp)
    twins = {"cpp": [], "py": ["--arap_bin", "%s %s" % (sys.executable, osp.join(ROOT, "arap_deform.py"))]}
    occs = {}
    for tag, arap in twins.items():
        _para_gen(tmp_path, inp, outp, mdir, ["--multseg", "--occ_layers", "--bwd_flow", "--keep_segments"] + arap)
        assert open(outp / "all_files.list", "rb").read() == plain_list
        stats = json.load(open(outp / "arap_stats.json"))
        assert stats["frames"] == 4 and stats["frames_done"] == 4 and stats["layers_done"] == 4 and stats["solves"] == 8
        assert stats["worker"] == ("serve" if tag == "cpp" else "batch")
        ext = open(outp / "all_files_ext.list").read().splitlines()
        assert len(ext) == 4
        for le in ext:
            t = le.split(" ")
            assert len(t) == 6
            stem = osp.relpath(t[2], str(outp / "Flow"))[:-4]
            assert t[5] == str(outp / "Occ" / (stem + ".png"))
            occ = np.array(Image.open(t[5]))
            assert Image.open(t[5]).mode == "L" and set(np.unique(occ)) <= {0, 255}
            # the same segment files (kept), through the Python entry
            rgb = pipeline.load_rgb(str(outp / "inpRGB" / (stem + ".png")))
            masks = np.stack([pipeline.load_mask_red(str(outp / "inpMasks" / ("%s_seg%d.png" % (stem, s)))) for s in (1, 2)])
            flows = np.stack([flo.flow_read(str(outp / "Flow" / ("%s_seg%d.flo" % (stem, s)))) for s in (1, 2)])
            want = opt.warp_layers(gpu_state, rgb, masks, flows)["occlusion"]
            assert np.array_equal(occ, want)
            # one object passes under the other: vertices of segment 1 are hidden by segment 2, which no single-layer
            # query reports
            single = [opt.warp_image_ex(gpu_state, None, masks[l], flows[l], backward=False)["occlusion"] for l in (0, 1)]
            hidden = (occ == 255) & (masks[0] == 0) & (single[0] == 0)
            print(tag, stem, "hidden by the other segment:", int(hidden.sum()))
            assert hidden.sum() > 10, stem
            occs[(tag, stem)] = occ
        # --resume: every requested output is there, nothing is redone
        out = _para_gen(tmp_path, inp, outp, mdir, ["--multseg", "--occ_layers", "--bwd_flow", "--resume"] + arap)
        assert "Scanning data to be processed\t\t0 files" in out
        shutil.rmtree(outp)
    for (tag, stem), occ in occs.items():
        assert np.array_equal(occ, occs[("cpp", stem)]), stem


def test_segment_files_are_removed_after_the_layers_line(tmp_path):
    inp, mdir = _tree(tmp_path)
    outp = tmp_path / "out"
    _para_gen(tmp_path, inp, outp, mdir, ["--multseg", "--occ_layers"])
    assert len(open(outp / "all_files_ext.list").read().splitlines()) == 4
    for seq in ("a", "b"):
        assert len(os.listdir(outp / "Occ" / seq)) == 2
        assert not [f for f in os.listdir(outp / "Flow" / seq) if "_seg" in f]
