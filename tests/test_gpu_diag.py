"""GPU: fold diagnostics (DESIGN.md "Fold diagnostics").  k_warp_diag / k_diag_finish through opt.warp_diag, the frame
solver, the command-line twins and para_gen.py; every comparison is bit for bit against the numpy twin of
tests/diag_ref.py -- integer counts, flags and extrema in the order of the bit patterns, no tolerance."""
import os
import os.path as osp
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import diag_ref as dr
from arap_flow_amd import build, flo, opt, pipeline, synth

pytestmark = pytest.mark.gpu
ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))


def _same(got, mask, flow):
    """a warp_diag result against the twin on the flow's positions"""
    want = dr.diag(mask, dr.flow_pos(flow))
    assert dr.stats_bytes(got["stats"]) == dr.stats_bytes(want[0]), (got["stats"], want[0])
    assert got["fold"].dtype == np.uint8 and np.array_equal(got["fold"], want[1])
    return want


# ---- opt.warp_diag at 67 x 9: W no multiple of 64, H no multiple of 4, 2 x 3 blocks ----------------------------------------
@pytest.mark.parametrize("mask_name", ["all", "random", "strip"])
def test_warp_diag_equals_twin(gpu_state, mask_name):
    mask, fields = dr.masks()[mask_name], dr.fields()
    assert set(fields) >= {"zero", "mirror", "translation", "noise_a", "noise_b", "nan_inf"} and len(fields) == 10
    for name, fl in fields.items():
        want = _same(opt.warp_diag(gpu_state, mask, fl), mask, fl)
        if mask_name != "strip" and name.startswith("noise"):
            assert 0 < want[0]["folded"] < want[0]["triangles"]
        if mask_name == "all" and name.startswith("spike"):         # the only fold, and both det extrema, at that vertex
            assert 0 < want[0]["folded"] <= 3 and want[0]["det_min"] == -1.75 and want[0]["disp2_max"] == 3.8125
    if mask_name == "all":
        st = opt.warp_diag(gpu_state, mask, fields["mirror"])["stats"]
        assert (st["folded"], st["triangles"], st["det_min"], st["det_max"]) == (1056, 1056, -1, -1)
        st = opt.warp_diag(gpu_state, mask, fields["translation"])["stats"]
        assert st["outside"] == dr.translation_outside(dr.W0, dr.H0, 3, -2) and st["folded"] == 0
        st = opt.warp_diag(gpu_state, mask, fields["nan_inf"])["stats"]
        assert st["nonfinite"] == 12
    if mask_name == "strip":
        st = opt.warp_diag(gpu_state, mask, fields["noise_a"])["stats"]
        assert st["vertices"] == dr.W0 and st["triangles"] == 0 and st["det_min"] == np.inf and st["det_max"] == -np.inf


def test_warp_diag_all_background_is_the_identity(gpu_state):
    mask, fl = dr.masks()["none"], dr.fields()["noise_a"]
    r = opt.warp_diag(gpu_state, mask, fl)
    _same(r, mask, fl)
    assert r["stats"] == dict(vertices=0, outside=0, triangles=0, folded=0, nonfinite=0, det_min=np.inf, det_max=-np.inf,
                              disp2_max=0) and not r["fold"].any()


def test_warp_diag_larger_frame_twice_and_outputs_one_at_a_time(gpu_state):
    W, H = 200, 150
    rng = np.random.default_rng(17)
    mask = np.where(rng.random((H, W)) < 0.1, 255, 0).astype(np.uint8)
    fl = rng.normal(0, 0.4, (H, W, 2)).astype(np.float32)
    a = opt.warp_diag(gpu_state, mask, fl)
    want = _same(a, mask, fl)
    assert 0 < want[0]["folded"] < want[0]["triangles"]
    b = opt.warp_diag(gpu_state, mask, fl)                           # the accumulator is re-armed on the stream
    assert dr.stats_bytes(a["stats"]) == dr.stats_bytes(b["stats"]) and a["fold"].tobytes() == b["fold"].tobytes()
    only = opt.warp_diag(gpu_state, mask, fl, fold=False)
    assert only["fold"] is None and dr.stats_bytes(only["stats"]) == dr.stats_bytes(a["stats"])


def test_warp_diag_bad_arguments(gpu_state):
    import torch
    lib, h = gpu_state.lib, gpu_state.handle
    t = torch.zeros(64, dtype=torch.uint8, device="cuda")
    p = t.data_ptr()
    assert lib.ArapFlow_WarpDiag(h, 4, 4, p, p, None, None) == -1            # no output
    assert lib.ArapFlow_WarpDiag(h, 4, 4, None, p, p, None) == -1 and lib.ArapFlow_WarpDiag(h, 4, 4, p, None, p, None) == -1
    assert lib.ArapFlow_WarpDiag(None, 4, 4, p, p, p, None) == -1 and lib.ArapFlow_WarpDiag(h, 0, 4, p, p, p, None) == -1
    assert lib.ArapFlow_WarpDiag(h, 1 << 16, 1 << 15, p, p, p, None) == -1   # W * H = 2^31
    with pytest.raises(ValueError):
        opt.warp_diag(gpu_state, np.zeros((4, 4), np.uint8), np.zeros((4, 5, 2), np.float32))


# ---- the frame solver at 64 x 64 ---------------------------------------------------------------------------------------
SCHEDULE = (1, 4, 100)
CROSS = np.asarray([(24, 32, 40, 32), (40, 32, 24, 32)], np.int32)       # two handles that swap places: the mesh folds


def _frames():
    W = H = 64
    out = [dict(mask_red=np.zeros((H, W), np.uint8), constraints=CROSS, rgb=synth.make_rgb(W, H, 5))]
    out += [synth.make_frame(W, H, seed=s, K=k, fd=3) for s, k in ((31, 1), (32, 2))]
    return out


def _solve(state, frames, diag, resident, use_async):
    state.set_resident(resident)
    try:
        fs = opt.FrameSolver(state, 64, 64, batch=len(frames))
        fs.set_outputs(backward=True, occlusion=True)
        if diag:
            fs.set_diag(True)
        for b, f in enumerate(frames):
            fs.set_frame(b, f["mask_red"], f["constraints"], rgb=f["rgb"])
        host = None
        if use_async:
            fs.solve_async(len(frames), *SCHEDULE, warp=True, download=True)
            fs.wait()
            host = [{k: (v.copy() if hasattr(v, "copy") else v) for k, v in fs.host_results(b).items()} for b in range(len(frames))]
        else:
            fs.solve(len(frames), *SCHEDULE)
            fs.warp(len(frames))
        res = [fs.results(b) for b in range(len(frames))]
        fs.close()
    finally:
        state.set_resident(True)
    return res, host


@pytest.fixture(scope="module")
def solved(gpu_state):
    frames = _frames()
    runs = {(d, r, a): _solve(gpu_state, frames, d, r, a)
            for d, r, a in ((True, True, False), (True, True, True), (True, False, True), (False, True, False))}
    return frames, runs


def test_solver_diagnostics_equal_twin_on_the_offset(solved, oracle):
    frames, runs = solved
    O, _, _ = oracle.frame(frames[0]["mask_red"], CROSS, *SCHEDULE, dtype=np.float32, mode=1, trig=1)
    assert dr.diag(frames[0]["mask_red"], O)[0]["folded"] > 0            # the oracle's own mesh folds
    for key in ((True, True, False), (True, True, True), (True, False, True)):
        res, host = runs[key]
        for b, f in enumerate(frames):
            want = dr.diag(f["mask_red"], res[b]["offset"])
            for r in [res[b]] + ([host[b]] if host else []):
                assert dr.stats_bytes(r["mesh_stats"]) == dr.stats_bytes(want[0]), (key, b, r["mesh_stats"], want[0])
                assert np.array_equal(r["fold"], want[1])
            assert want[0]["vertices"] == int((f["mask_red"] == 0).sum()) and want[0]["triangles"] > 0
        assert 0 < dr.diag(frames[0]["mask_red"], res[0]["offset"])[0]["folded"] and res[0]["fold"].any()
    masks = [f["mask_red"].tobytes() for f in frames]
    assert len(set(masks)) == 3


def test_solver_outputs_keep_their_bits_with_diagnostics_on(solved):
    _, runs = solved
    on, off = runs[(True, True, False)][0], runs[(False, True, False)][0]
    for a, b in zip(on, off):
        assert "mesh_stats" not in b and "fold" not in b and "mesh_stats" in a
        for k in ("flow", "warped_rgb", "warped_mask", "offset", "angle", "backward_flow", "occlusion_bwd", "occlusion"):
            assert a[k].tobytes() == b[k].tobytes(), k


def test_solver_without_diag_reports_none(gpu_state):
    fs = opt.FrameSolver(gpu_state, 64, 64, batch=1)
    f = _frames()[1]
    fs.set_frame(0, f["mask_red"], f["constraints"], rgb=f["rgb"])
    fs.solve(1, *SCHEDULE)
    fs.warp(1)
    assert gpu_state.lib.ArapFlow_SolverGetDiag(fs.h, 0, None, None) == -1
    fs.set_diag(True)
    assert gpu_state.lib.ArapFlow_SolverGetDiag(fs.h, 0, None, None) == -1       # the last warp computed none
    fs.warp(1)
    r = fs.results(0)
    assert dr.same((r["mesh_stats"], r["fold"]), dr.diag(f["mask_red"], r["offset"]))
    fs.set_diag(False)
    fs.warp(1)
    assert "mesh_stats" not in fs.results(0)
    fs.close()


# ---- the command-line twins --------------------------------------------------------------------------------------------
def _run(args, cwd):
    env = dict(os.environ, HIP_VISIBLE_DEVICES=os.environ.get("HIP_VISIBLE_DEVICES", "0"))
    r = subprocess.run(args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_arap_deform_tokens_both_twins(tmp_path, gpu_state):
    W, H = 96, 64
    frames = [dict(mask_red=np.zeros((H, W), np.uint8), rgb=synth.make_rgb(W, H, 3),
                   constraints=np.asarray([(36, 32, 60, 32), (60, 32, 36, 32)], np.int32)),
              synth.make_frame(W, H, seed=12, fd=3)]
    for k, f in enumerate(frames):
        Image.fromarray(f["rgb"]).save(tmp_path / ("r%d.png" % k))
        Image.fromarray(np.stack([f["mask_red"]] * 3, -1)).save(tmp_path / ("m%d.png" % k))
        pipeline.write_constraints(str(tmp_path / ("c%d.txt" % k)), [tuple(c) for c in f["constraints"]])
    fs = opt.FrameSolver(gpu_state, W, H, batch=2)
    fs.set_diag(True)
    for k, f in enumerate(frames):
        fs.set_frame(k, f["mask_red"], f["constraints"], rgb=f["rgb"])
    fs.solve(2, 19, 8, 400)
    fs.warp(2)
    res = [fs.results(k) for k in range(2)]
    fs.close()
    want = [dr.diag(f["mask_red"], r["offset"]) for f, r in zip(frames, res)]
    assert want[0][0]["folded"] > 0
    for tag, prog in (("py", [sys.executable, osp.join(ROOT, "arap_deform.py")]), ("cpp", [build.build_host()[0]])):
        lines = []
        for k in range(2):
            p = lambda n: str(tmp_path / ("%s_%s%d" % (tag, n, k)))
            six = [str(tmp_path / ("r%d.png" % k)), str(tmp_path / ("m%d.png" % k)), str(tmp_path / ("c%d.txt" % k)),
                   p("f") + ".flo", p("w") + ".png", p("wm") + ".png"]
            lines.append(" ".join(six + (["diag=%s.txt" % p("d"), "junk", "fold=%s.png" % p("fo")] if k == 0 else ["diag=%s.txt" % p("d")])))
        (tmp_path / ("%s.txt" % tag)).write_text("\n".join(lines))
        _run(prog + [str(tmp_path / ("%s.txt" % tag))], str(tmp_path))
        for k in range(2):
            assert open(tmp_path / ("%s_d%d.txt" % (tag, k))).read() == pipeline.format_diag(want[k][0]), (tag, k)
            assert np.array_equal(flo.flow_read(str(tmp_path / ("%s_f%d.flo" % (tag, k)))), res[k]["flow"])
        fold = Image.open(tmp_path / ("%s_fo0.png" % tag))
        assert fold.mode == "L" and np.array_equal(np.array(fold), want[0][1])
        assert not (tmp_path / ("%s_fo1.png" % tag)).exists()


def test_warp_image_tokens_both_twins(tmp_path, gpu_state):
    import occ_ref
    rgb, mask, fl = occ_ref.folded_case(70, 50, 3.0)
    Image.fromarray(rgb).save(tmp_path / "i.png")
    Image.fromarray(np.stack([mask] * 3, -1)).save(tmp_path / "m.png")
    flo.flow_write(str(tmp_path / "f.flo"), fl)
    want = dr.diag(mask, dr.flow_pos(fl))
    assert 0 < want[0]["folded"] < want[0]["triangles"]
    ref = opt.warp_image_ex(gpu_state, rgb, mask, fl, backward=False, occlusion=True)
    for tag, prog in (("py", [sys.executable, osp.join(ROOT, "warp_image.py")]), ("cpp", [build.build_host()[1]])):
        q = lambda n: str(tmp_path / (tag + n))
        _run(prog + [str(tmp_path / "i.png"), str(tmp_path / "m.png"), str(tmp_path / "f.flo"), q("w.png"), q("wm.png"),
                     "diag=" + q("d.txt"), "occ=" + q("o.png"), "fold=" + q("fo.png")], str(tmp_path))
        assert open(q("d.txt")).read() == pipeline.format_diag(want[0])
        assert np.array_equal(np.array(Image.open(q("fo.png"))), want[1]) and Image.open(q("fo.png")).mode == "L"
        assert np.array_equal(np.array(Image.open(q("w.png"))), ref["warped_rgb"])
        assert np.array_equal(np.array(Image.open(q("o.png"))), ref["occlusion"])
    # diag= alone leaves the plain warp as it is (in process: the Python twin's file level)
    q = lambda n: str(tmp_path / ("only" + n))
    pipeline.warp_files(gpu_state, str(tmp_path / "i.png"), str(tmp_path / "m.png"), str(tmp_path / "f.flo"), q("w.png"),
                        q("wm.png"), extra=dict(diag=q("d.txt")))
    assert open(q("d.txt")).read() == pipeline.format_diag(want[0]) and not osp.exists(q("fo.png"))
    assert np.array_equal(np.array(Image.open(q("w.png"))), ref["warped_rgb"])


# ---- para_gen.py --diag --max_fold -------------------------------------------------------------------------------------
@pytest.mark.parametrize("multseg", [False, True])
def test_para_gen_diag_and_max_fold(tmp_path, multseg):
    """two pairs of a smooth two-segment sequence, two of a whole-frame object whose only matches swap two handles: the
    second folds about 0.85 % of its triangles (CPU oracle: 102 of 11970), the first none; --max_fold 0.005 parts them"""
    W, H = 96, 64
    inp, outp, mdir = tmp_path / "in", tmp_path / "out", tmp_path / "matches"
    fr = synth.make_frame(W, H, seed=1 + ord("a"), K=2, fd=1)
    whole = dict(rgb=synth.make_rgb(W, H, 9), labels=np.ones((H, W), np.uint8),
                 constraints=[(36, 32, 60, 32), (60, 32, 36, 32)])
    for seq, f in (("a", fr), ("c", whole)):
        os.makedirs(inp / "orgRGB" / seq); os.makedirs(inp / "orgMasks" / seq); os.makedirs(mdir / seq)
        for n in range(3):
            Image.fromarray(f["rgb"]).save(inp / "orgRGB" / seq / ("%05d.png" % n))
            Image.fromarray(np.asarray(f["labels"]).astype(np.uint8)).save(inp / "orgMasks" / seq / ("%05d.png" % n))
            (mdir / seq / ("%05d.txt" % n)).write_text("\n".join("%d %d %d %d 1.0 0" % tuple(c) for c in f["constraints"]))
    cmd = [sys.executable, osp.join(ROOT, "para_gen.py"), "--input", str(inp), "--output", str(outp), "--gpu", "0", "--fd", "1",
           "--matches", str(mdir), "--max_fold", "0.005"] + (["--multseg", "--keep_segments"] if multseg else [])
    _run(cmd, str(tmp_path))
    read = lambda f: open(outp / f).read().splitlines()
    lst, ext, rej = read("all_files.list"), read("all_files_ext.list"), read("rejected.list")
    assert len(lst) == 2 and len(ext) == 2 and len(rej) == 2
    for ln, le in zip(lst, ext):
        t = le.split(" ")
        stem = osp.relpath(t[2], str(outp / "Flow"))[:-4]
        assert t[:3] == ln.split(" ") and stem.startswith("a" + os.sep)
        assert t[3:] == [str(outp / "Diag" / (stem + ".txt")), str(outp / "Fold" / (stem + ".png"))]
        st = pipeline.parse_diag(open(t[3]).read())
        assert st["folded"] == 0 and st["nonfinite"] == 0 and st["triangles"] > 0 and not pipeline.pair_rejected(st, 0.005)
        assert not np.array(Image.open(t[4])).any()
    for ln in rej:
        t = ln.split(" ")
        stem = osp.relpath(t[2], str(outp / "Flow"))[:-4]
        assert len(t) == 6 and stem.startswith("c" + os.sep) and all(osp.exists(q) for q in t[:3])
        st = pipeline.parse_diag(open(outp / "Diag" / (stem + ".txt")).read())
        assert [int(v) for v in t[3:]] == [st["folded"], st["triangles"], st["nonfinite"]]
        assert st["triangles"] == 2 * (W - 1) * (H - 1) and st["folded"] > 0.005 * st["triangles"]
        fold = np.array(Image.open(outp / "Fold" / (stem + ".png")))
        # the files against the twin on the flow that was written (positions (x, y) + flow)
        flow = flo.flow_read(t[2])
        if not multseg:
            mask = np.array(Image.open(outp / "inpMasks" / (stem + ".png")).convert("RGB"))[..., 0]
            assert fold.any() and set(np.unique(fold)) <= {0, 255} and fold.shape == (H, W) and (fold[mask != 0] == 0).all()
            assert flow.shape == (H, W, 2)
    import json
    assert json.load(open(outp / "arap_stats.json"))["rejected"] == 2
    if multseg:
        # the frame's files are the merge of its segments' (kept: --keep_segments), named like the other segment outputs
        for stem in ("a/00000", "a/00001"):
            segs = sorted(f for f in os.listdir(outp / "Diag" / "a") if f.startswith(osp.basename(stem) + "_seg"))
            assert len(segs) == 2
            stats = [pipeline.parse_diag(open(outp / "Diag" / "a" / f).read()) for f in segs]
            folds = [np.array(Image.open(outp / "Fold" / "a" / f.replace(".txt", ".png"))) for f in segs]
            merged = pipeline.merge_diag(stats, folds)
            assert open(outp / "Diag" / (stem + ".txt")).read() == pipeline.format_diag(merged[0])
            assert np.array_equal(np.array(Image.open(outp / "Fold" / (stem + ".png"))), merged[1])
            assert merged[0]["vertices"] == sum(s["vertices"] for s in stats) > 0
    # --resume: every requested output is there, nothing is redone, and the lists come out the same
    out = _run(cmd + ["--resume"], str(tmp_path))
    assert "Scanning data to be processed\t\t0 files" in out
    assert (read("all_files.list"), read("all_files_ext.list"), read("rejected.list")) == (lst, ext, rej)
