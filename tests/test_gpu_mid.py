"""GPU: in-between frames from the constraint ramp (DESIGN.md "In-between frames"): k_warp_step through opt.warp_step
against the numpy restatement of tests/mid_ref.py, the frame solver's snapshots against the ramp composed from the
oracle's pieces, and the command-line hosts."""
import os
import os.path as osp
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import mid_ref
import occ_ref
from arap_flow_amd import build, flo, opt, pipeline, synth

pytestmark = pytest.mark.gpu
ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))


@pytest.mark.parametrize("W,H,kind", [(67, 45, "smooth"), (67, 45, "folded"), (16, 16, "smooth"), (16, 16, "folded")])
def test_warp_step_equals_restatement(gpu_state, W, H, kind):
    """odd W, N no multiple of 256, more than one block (67x45); one partial block (16x16); masks with holes"""
    rgb, mask, fa, fb = mid_ref.two_state_case(W, H, W * H, kind)
    r = opt.warp_step(gpu_state, rgb, mask, fa, fb)
    a, b = occ_ref.field_from_flow(fa), occ_ref.field_from_flow(fb)
    assert np.array_equal(r["step"], mid_ref.step_ref(mask, a, b))
    ref = occ_ref.warp_ref(rgb, mask, a)
    assert np.array_equal(r["warped_rgb"], ref["warped_rgb"]) and np.array_equal(r["warped_mask"], ref["warped_mask"])
    assert opt.warp_step(gpu_state, None, mask, fa, fb)["warped_rgb"] is None


def test_warp_step_towards_zero_flow_is_the_backward_flow(gpu_state):
    rgb, mask, fl = occ_ref.folded_case(67, 45, 2.0, seed=9)
    r = opt.warp_step(gpu_state, rgb, mask, fl, np.zeros_like(fl))
    ex = opt.warp_image_ex(gpu_state, rgb, mask, fl, backward=True, occlusion=False)
    assert np.array_equal(r["step"], ex["backward_flow"]) and (r["step"] != 0).any()
    wrgb, wmsk = opt.warp_image(gpu_state, rgb, mask, fl)
    assert np.array_equal(r["warped_rgb"], wrgb) and np.array_equal(r["warped_mask"], wmsk)


def test_warp_step_bad_arguments(gpu_state):
    rgb, mask, fl = occ_ref.folded_case(16, 16, 1.0, seed=1)
    with pytest.raises(ValueError):
        opt.warp_step(gpu_state, rgb, mask, fl, fl[:-1])
    lib = gpu_state.lib
    assert lib.ArapFlow_WarpStep(gpu_state.handle, 16, 16, None, None, None, None, None, None, None) == -1


# ---- the frame solver ------------------------------------------------------------------------------------------------
def _solve(state, frames, snapshots, outputs, resident=True, use_async=False):
    """one solve + warp of the solver case; per slot the results and, per snapshot, its four outputs"""
    W, H = mid_ref.SOLVER_CASE["W"], mid_ref.SOLVER_CASE["H"]
    state.set_resident(resident)
    try:
        fs = opt.FrameSolver(state, W, H, batch=len(frames))
        if outputs:
            fs.set_outputs(backward=True, occlusion=True)
        fs.set_snapshots(snapshots)
        for b, f in enumerate(frames):
            fs.set_frame(b, f["mask_red"], f["constraints"], rgb=f["rgb"])
        if use_async:
            fs.solve_async(len(frames), *mid_ref.SOLVER_CASE["schedule"], warp=True, download=True)
            fs.wait()
            host = [[{k: v.copy() for k, v in fs.host_snapshot(b, q).items()} for q in range(len(snapshots))]
                    for b in range(len(frames))]
        else:
            fs.solve(len(frames), *mid_ref.SOLVER_CASE["schedule"])
            fs.warp(len(frames))
            host = None
        res = [fs.results(b) for b in range(len(frames))]
        snaps = [[fs.snapshot(b, q) for q in range(len(snapshots))] for b in range(len(frames))]
        launches = fs.stats()["resident_launches"]
        fs.close()
    finally:
        state.set_resident(True)
    return dict(results=res, snaps=snaps, host=host, resident_launches=launches)


@pytest.fixture(scope="module")
def case(gpu_state, oracle):
    frames = mid_ref.solver_case(oracle)
    snaps = mid_ref.SOLVER_CASE["snapshots"]
    return dict(frames=frames, on=_solve(gpu_state, frames, snaps, outputs=True),
                off=_solve(gpu_state, frames, (), outputs=True))


def _same_snapshots(a, b):
    assert len(a) == len(b) and all(len(sa) == len(sb) > 0 for sa, sb in zip(a, b))
    return all(np.array_equal(x[k], y[k]) for sa, sb in zip(a, b) for x, y in zip(sa, sb) for k in ("flow", "rgb", "mask", "step"))


def test_snapshot_states_equal_the_composed_oracle_loop(case):
    """every S_i bit for bit: flow_k is S_i - grid by the final flow's expression, and flow_k + grid is S_i itself
    wherever that subtraction is exact in float32 (mid_ref.exact_flow: all but one value of this case, a vertex that
    moved to less than half its coordinate, where no flow can carry the state's last bit)"""
    W, H = mid_ref.SOLVER_CASE["W"], mid_ref.SOLVER_CASE["H"]
    grid = mid_ref.grid_field(W, H)
    assert case["on"]["resident_launches"] > 0
    for f, snaps in zip(case["frames"], case["on"]["snaps"]):
        for i, s in zip(mid_ref.SOLVER_CASE["snapshots"], snaps):
            S = f["states"][i - 1]
            assert np.array_equal(s["flow"], S - grid)
            ex = mid_ref.exact_flow(S)
            assert np.array_equal((s["flow"] + grid)[ex], S[ex])


def test_snapshot_frames_equal_the_oracle_warp_of_the_state(case, oracle):
    for f, snaps in zip(case["frames"], case["on"]["snaps"]):
        for i, s in zip(mid_ref.SOLVER_CASE["snapshots"], snaps):
            o_rgb, o_msk = oracle.warp_offset(f["rgb"], f["mask_red"], f["states"][i - 1])
            assert np.array_equal(s["rgb"], o_rgb) and np.array_equal(s["mask"], o_msk)
            assert (s["mask"] == 255).any()


def test_snapshot_steps_equal_restatement_on_consecutive_states(case):
    idx = mid_ref.SOLVER_CASE["snapshots"]
    for f, snaps in zip(case["frames"], case["on"]["snaps"]):
        S = f["states"]
        for k, s in enumerate(snaps):
            nxt = S[idx[k + 1] - 1] if k + 1 < len(idx) else S[-1]
            assert np.array_equal(s["step"], mid_ref.step_ref(f["mask_red"], S[idx[k] - 1], nxt))
        assert (snaps[0]["step"] != 0).any()


def test_last_ramp_step_snapshot_is_the_final_result(case):
    assert mid_ref.SOLVER_CASE["snapshots"][-1] == mid_ref.SOLVER_CASE["schedule"][0]
    for r, snaps in zip(case["on"]["results"], case["on"]["snaps"]):
        assert np.array_equal(snaps[-1]["flow"], r["flow"])
        assert np.array_equal(snaps[-1]["rgb"], r["warped_rgb"]) and np.array_equal(snaps[-1]["mask"], r["warped_mask"])


def test_results_are_the_same_with_snapshots_on_and_off(case):
    for a, b in zip(case["on"]["results"], case["off"]["results"]):
        assert set(a) == set(b) and "backward_flow" in a and "occlusion" in a
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    assert case["off"]["snaps"] == [[], [], []]


def test_snapshots_off_has_no_snapshot(gpu_state, case):
    f = case["frames"][0]
    fs = opt.FrameSolver(gpu_state, mid_ref.SOLVER_CASE["W"], mid_ref.SOLVER_CASE["H"], batch=1)
    fs.set_frame(0, f["mask_red"], f["constraints"], rgb=f["rgb"])
    fs.solve(1, 1, 1, 10)
    fs.warp(1)
    with pytest.raises(ValueError):
        fs.snapshot(0, 0)
    fs.close()


def test_kernel_per_phase_path_gives_identical_snapshots(gpu_state, case):
    r = _solve(gpu_state, case["frames"], mid_ref.SOLVER_CASE["snapshots"], outputs=False, resident=False)
    assert r["resident_launches"] == 0
    assert _same_snapshots(r["snaps"], case["on"]["snaps"])


def test_async_solve_host_snapshots_equal_snapshots(gpu_state, case):
    r = _solve(gpu_state, case["frames"], mid_ref.SOLVER_CASE["snapshots"], outputs=False, use_async=True)
    assert _same_snapshots(r["host"], r["snaps"]) and _same_snapshots(r["snaps"], case["on"]["snaps"])


def test_step_index_above_num_iter_is_refused_and_solver_stays_usable(gpu_state, case):
    W, H = mid_ref.SOLVER_CASE["W"], mid_ref.SOLVER_CASE["H"]
    f = case["frames"][1]
    fs = opt.FrameSolver(gpu_state, W, H, batch=1)
    fs.set_frame(0, f["mask_red"], f["constraints"], rgb=f["rgb"])
    fs.set_snapshots((1, 5))
    with pytest.raises(ValueError):
        fs.solve(1, *mid_ref.SOLVER_CASE["schedule"])                  # numIter = 4 < 5
    with pytest.raises(ValueError):
        fs.solve_async(1, *mid_ref.SOLVER_CASE["schedule"])
    for bad in ((0, 2), (2, 2), (3, 1), tuple(range(1, 10))):
        with pytest.raises(ValueError):
            fs.set_snapshots(bad)
    fs.set_snapshots(mid_ref.SOLVER_CASE["snapshots"])
    fs.solve(1, *mid_ref.SOLVER_CASE["schedule"])
    fs.warp(1)
    want = case["on"]["snaps"][1]
    assert _same_snapshots([[fs.snapshot(0, q) for q in range(3)]], [want])
    fs.close()


# ---- hosts -------------------------------------------------------------------------------------------------------------
def _run(args, cwd):
    env = dict(os.environ, HIP_VISIBLE_DEVICES=os.environ.get("HIP_VISIBLE_DEVICES", "0"))
    r = subprocess.run(args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _read_mid(prefix, step):
    f = pipeline.mid_files(prefix, step)
    return dict(flow=flo.flow_read(f["flow"]), rgb=np.array(Image.open(f["rgb"])), mask=np.array(Image.open(f["mask"])),
                step=flo.flow_read(f["step"]))


def test_arap_deform_mid_token_both_twins_equal_solver(tmp_path, gpu_state):
    W, H = 96, 64
    steps = (4, 9, 14)
    frames = [synth.make_frame(W, H, seed=s, fd=3) for s in (11, 12, 13)]
    for k, f in enumerate(frames):
        Image.fromarray(f["rgb"]).save(tmp_path / ("r%d.png" % k))
        Image.fromarray(np.stack([f["mask_red"]] * 3, -1)).save(tmp_path / ("m%d.png" % k))
        pipeline.write_constraints(str(tmp_path / ("c%d.txt" % k)), [tuple(c) for c in f["constraints"]])
    for tag, prog in (("py", [sys.executable, osp.join(ROOT, "arap_deform.py")]), ("cpp", [build.build_host()[0]])):
        lines = []
        for k in range(3):
            p = lambda n: str(tmp_path / ("%s_%s%d" % (tag, n, k)))
            six = [str(tmp_path / ("r%d.png" % k)), str(tmp_path / ("m%d.png" % k)), str(tmp_path / ("c%d.txt" % k)),
                   p("f") + ".flo", p("w") + ".png", p("wm") + ".png"]
            lines.append(" ".join(six + (["mid=%s" % pipeline.mid_token(steps, p("mid"))] if k != 1 else [])))   # line 1 is plain
        (tmp_path / ("%s.txt" % tag)).write_text("\n".join(lines))
        _run(prog + [str(tmp_path / ("%s.txt" % tag))], str(tmp_path))
        assert not [n for n in os.listdir(tmp_path) if n.startswith("%s_mid1" % tag)]
    fs = opt.FrameSolver(gpu_state, W, H, batch=3)
    fs.set_snapshots(steps)
    for k, f in enumerate(frames):
        fs.set_frame(k, f["mask_red"], f["constraints"], rgb=f["rgb"])
    fs.solve(3, 19, 8, 400)
    fs.warp(3)
    for k in range(3):
        r = fs.results(k)
        for tag in ("py", "cpp"):
            assert np.array_equal(flo.flow_read(str(tmp_path / ("%s_f%d.flo" % (tag, k)))), r["flow"])
        if k == 1:
            continue
        for q, i in enumerate(steps):
            lib = fs.snapshot(k, q)
            a, b = (_read_mid(str(tmp_path / ("%s_mid%d" % (tag, k))), i) for tag in ("py", "cpp"))
            for name in ("py", "cpp"):
                files = pipeline.mid_files(str(tmp_path / ("%s_mid%d" % (name, k))), i)
                assert Image.open(files["mask"]).mode == Image.open(tmp_path / ("%s_wm%d.png" % (name, k))).mode
            for key in ("flow", "rgb", "mask", "step"):
                assert np.array_equal(a[key], b[key]), key
            assert np.array_equal(a["flow"], lib["flow"]) and np.array_equal(a["step"], lib["step"])
            assert np.array_equal(a["rgb"], lib["rgb"]) and np.array_equal(a["mask"] != 0, lib["mask"] != 0)
    fs.close()


def test_arap_deform_differing_mid_steps_in_a_batch_is_an_error(tmp_path):
    W, H = 96, 64
    f = synth.make_frame(W, H, seed=11, fd=3)
    Image.fromarray(f["rgb"]).save(tmp_path / "r.png")
    Image.fromarray(np.stack([f["mask_red"]] * 3, -1)).save(tmp_path / "m.png")
    pipeline.write_constraints(str(tmp_path / "c.txt"), [tuple(c) for c in f["constraints"]])
    six = [str(tmp_path / n) for n in ("r.png", "m.png", "c.txt")]
    lines = [" ".join(six + [str(tmp_path / ("o%d%s" % (k, e))) for e in (".flo", ".png", "m.png")] +
                      ["mid=%s:%s" % (st, tmp_path / ("mid%d" % k))]) for k, st in enumerate(("4,9", "4,10"))]
    (tmp_path / "l.txt").write_text("\n".join(lines))
    env = dict(os.environ, HIP_VISIBLE_DEVICES=os.environ.get("HIP_VISIBLE_DEVICES", "0"))
    for prog in ([sys.executable, osp.join(ROOT, "arap_deform.py")], [build.build_host()[0]]):
        r = subprocess.run(prog + [str(tmp_path / "l.txt")], cwd=str(tmp_path), env=env, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode != 0 and "differ" in r.stdout + r.stderr


def test_para_gen_mid(tmp_path):
    W, H = 96, 64
    inp, outp, mdir = tmp_path / "in", tmp_path / "out", tmp_path / "matches"
    seq = "a"
    os.makedirs(inp / "orgRGB" / seq); os.makedirs(inp / "orgMasks" / seq); os.makedirs(mdir / seq)
    fr = synth.make_frame(W, H, seed=3, K=2, fd=1)
    for n in range(3):                                       # three frames: two pairs
        Image.fromarray(fr["rgb"]).save(inp / "orgRGB" / seq / ("%05d.png" % n))
        Image.fromarray(fr["labels"].astype(np.uint8)).save(inp / "orgMasks" / seq / ("%05d.png" % n))
        (mdir / seq / ("%05d.txt" % n)).write_text("\n".join("%d %d %d %d 1.0 0" % tuple(c) for c in fr["constraints"]))
    base = [sys.executable, osp.join(ROOT, "para_gen.py"), "--input", str(inp), "--gpu", "0", "--fd", "1", "--matches",
            str(mdir)]
    _run(base + ["--output", str(outp), "--mid", "2"], str(tmp_path))
    lst = open(outp / "all_files.list").read().splitlines()
    ext = open(outp / "all_files_ext.list").read().splitlines()
    assert len(lst) == 2 and len(ext) == 2
    for ln, le in zip(lst, ext):
        t = le.split(" ")
        assert t[:3] == ln.split(" ") and len(t) == 3 + 8
        stem = osp.relpath(t[2], str(outp / "Flow"))[:-4]
        want = [pipeline.mid_files(str(outp / "Mid" / stem), i)[k] for i in (6, 12) for k in ("flow", "rgb", "mask", "step")]
        assert t[3:] == want and all(osp.exists(q) for q in want)
        final = flo.flow_read(t[2])
        f6, f12 = flo.flow_read(want[0]), flo.flow_read(want[4])
        assert f6.shape == (H, W, 2) and np.abs(f6).max() > 0 and (f6 != f12).any() and (f12 != final).any()
        assert np.array(Image.open(want[1])).shape == (H, W, 3)
        wm = np.array(Image.open(want[2])) != 0
        st = flo.flow_read(want[3])
        assert (st[~wm] == 0).all() and (st[wm] != 0).any()
    # all_files.list is what a run without --mid writes: frame 1, warped frame, flow per pair
    assert lst == [" ".join(str(outp / d / seq / ("%05d%s" % (n, e))) for d, e in (("inpRGB", ".png"), ("wRGB", ".png"),
                                                                                  ("Flow", ".flo"))) for n in range(2)]
    # --resume skips a pair only when all its in-between files exist: one removed, that pair alone is redone
    os.remove(ext[0].split(" ")[-1])
    out = _run(base + ["--output", str(outp), "--mid", "2", "--resume"], str(tmp_path))
    assert "Scanning data to be processed\t\t1 files" in out and osp.exists(ext[0].split(" ")[-1])
