"""In-between frames from the constraint ramp (DESIGN.md "In-between frames"), no GPU: the numpy restatement of `step`
(tests/mid_ref.py) against its sequential statement and against occ_ref's backward flow, the ramp composed from the
oracle's pieces against oracle.frame, the mid= token of the list line, para_gen's --mid, and the library's new symbols."""
import ctypes

import numpy as np
import pytest

import helpers
import mid_ref
import occ_ref
from arap_flow_amd import pipeline

GPU_WARP_CASES = [(67, 45, "smooth"), (67, 45, "folded"), (16, 16, "smooth"), (16, 16, "folded")]   # test_gpu_mid.py


@pytest.mark.parametrize("W,H,seed,kind", [(6, 5, 1, "folded"), (9, 7, 2, "folded"), (8, 8, 3, "smooth"), (2, 2, 4, "folded"),
                                           (1, 5, 5, "folded"), (10, 6, 6, "smooth")])
def test_restatement_equals_sequential_definition(W, H, seed, kind):
    if kind == "folded":
        rgb, mask, fa, fb = mid_ref.two_state_case(W, H, seed, "folded")
    else:
        mask = np.where(np.random.default_rng(seed).random((H, W)) < 0.1, 255, 0).astype(np.uint8)
        fa, fb = mid_ref.smooth_flow(W, H, seed, 1.0), mid_ref.smooth_flow(W, H, seed + 1, 2.0)
    a, b = occ_ref.field_from_flow(fa), occ_ref.field_from_flow(fb)
    if W * H > 20:                               # out-of-frame and NaN positions in either state
        a[1, 1] = (np.float32(-3.5), np.float32(2.0))
        b[2, 3] = (np.float32(np.nan), np.float32(1.0))
    assert np.array_equal(mid_ref.step_ref(mask, a, b), mid_ref.step_brute(mask, a, b), equal_nan=True)


@pytest.mark.parametrize("W,H,amp,seed", [(70, 50, 3.0, None), (67, 45, 1.5, 7), (16, 16, 2.0, 8), (2, 2, 0.5, 3), (1, 5, 1.0, 4)])
def test_step_towards_the_grid_is_the_backward_flow(W, H, amp, seed):
    rgb, mask, fl = occ_ref.folded_case(W, H, amp, seed)
    a = occ_ref.field_from_flow(fl)
    want = occ_ref.warp_ref(None, mask, a)["backward_flow"]
    assert np.array_equal(mid_ref.step_ref(mask, a, mid_ref.grid_field(W, H)), want)


@pytest.mark.parametrize("W,H,kind", GPU_WARP_CASES)
def test_two_state_cases_tell_step_from_backward_flow_and_zero(W, H, kind):
    rgb, mask, fa, fb = mid_ref.two_state_case(W, H, W * H, kind)
    a, b = occ_ref.field_from_flow(fa), occ_ref.field_from_flow(fb)
    step = mid_ref.step_ref(mask, a, b)
    r = occ_ref.warp_ref(rgb, mask, a)
    cov = r["warped_mask"] == 255
    assert 0.3 * W * H < cov.sum() < W * H and (step[~cov] == 0).all()     # drawn and undrawn pixels both occur
    differs_bwd = (step != r["backward_flow"]).any(-1)[cov].mean()
    nonzero = (step != 0).any(-1)[cov].mean()
    assert differs_bwd > 0.9 and nonzero > 0.9


def test_solver_case_states_tell_step_from_backward_flow_and_zero(oracle):
    W, H = mid_ref.SOLVER_CASE["W"], mid_ref.SOLVER_CASE["H"]
    grid = mid_ref.grid_field(W, H)
    frames = mid_ref.solver_case(oracle)
    areas = [int((f["mask_red"] == 0).sum()) for f in frames]
    assert len(set(areas)) == 3 and max(areas) > 2 * min(areas)              # uneven masks
    for f in frames:
        S = f["states"]
        assert len(f["constraints"]) > 0
        for a, b in ((S[0], S[2]), (S[2], S[3])):
            step = mid_ref.step_ref(f["mask_red"], a, b)
            r = occ_ref.warp_ref(None, f["mask_red"], a)
            cov = r["warped_mask"] == 255
            assert (step != r["backward_flow"]).any(-1)[cov].mean() > 0.5 and (step != 0).any(-1)[cov].mean() > 0.5
        # the ramp moves: consecutive states differ.  flow + grid gives a state's bits back wherever Offset - grid is
        # exact in float32, which is how the GPU test reads the states: everywhere but at a vertex that moved to less
        # than half its coordinate (one value of these twelve states)
        assert all((S[i] != S[i + 1]).any() for i in range(3))
        assert all(mid_ref.exact_flow(s).mean() > 0.999 for s in S)


def test_composed_ramp_equals_oracle_frame(oracle):
    """the snapshot comparator: constraint_image at alpha_i + solve warm-started from the previous step, numIter times,
    is oracle.frame bit for bit"""
    from arap_flow_amd import synth
    f = synth.make_frame(64, 64, seed=5, K=1, fd=3)
    Os, As = mid_ref.ramp_states(oracle, f["mask_red"], f["constraints"], 4, 2, 40)
    O, A, _ = oracle.frame(f["mask_red"], f["constraints"], numIter=4, nIterations=2, lIterations=40, dtype=np.float32,
                           mode=1, trig=1)
    assert len(Os) == 4 and np.array_equal(Os[-1], O) and np.array_equal(As[-1], A)
    assert (Os[-1] != mid_ref.grid_field(64, 64)).any() and (Os[0] != Os[-1]).any()


def test_mid_token_round_trip():
    six = ["r.png", "m.png", "c.txt", "f.flo", "w.png", "wm.png"]
    ln = pipeline.parse_line(" ".join(six + ["mid=4,9,14:/out/Mid/a/00001", "bwd=b.flo"]))
    assert ln.extra == dict(mid="4,9,14:/out/Mid/a/00001", bwd="b.flo")
    assert pipeline.parse_mid(ln.extra["mid"]) == ((4, 9, 14), "/out/Mid/a/00001")
    text = pipeline.format_line(ln)
    assert text == " ".join(six + ["bwd=b.flo", "mid=4,9,14:/out/Mid/a/00001"])
    assert pipeline.parse_line(text) == ln
    assert pipeline.mid_token((4, 9, 14), "/p") == "4,9,14:/p"
    assert pipeline.mid_files("/p/x", 4) == dict(flow="/p/x_s04.flo", rgb="/p/x_s04.png", mask="/p/x_s04_mask.png",
                                                 step="/p/x_s04_step.flo")
    assert pipeline.mid_files("q", 14)["step"] == "q_s14_step.flo"
    for bad in ("mid=4,4:/p", "mid=9,4:/p", "mid=0,4:/p", "mid=4,9", "mid=4,9:", "mid=a:/p", "mid=:/p", "mid=4,:/p",
                "mid=1,2,3,4,5,6,7,8,9:/p"):
        with pytest.raises(ValueError):
            pipeline.parse_line(" ".join(six + [bad]))


def test_line_without_mid_parses_as_before():
    six = ["r.png", "m.png", "c.txt", "f.flo", "w.png", "wm.png"]
    assert pipeline.parse_line(" ".join(six)) == pipeline.SolveLine(*six, extra={})
    ln = pipeline.parse_line(" ".join(six + ["occ=o.png", "x", "middle=3"]))
    assert ln == pipeline.SolveLine(*six, extra=dict(occ="o.png"))
    assert pipeline.format_line(ln) == " ".join(six + ["occ=o.png"])
    assert pipeline.batch_snapshots([ln, pipeline.SolveLine(*six, extra={})]) == ()


def test_batch_snapshots_same_steps_or_error():
    six = ["r.png", "m.png", "c.txt", "f.flo", "w.png", "wm.png"]
    a = pipeline.SolveLine(*six, extra=dict(mid="4,9:/a"))
    b = pipeline.SolveLine(*six, extra=dict(mid="4,9:/b"))
    c = pipeline.SolveLine(*six, extra=dict(mid="4,10:/c"))
    plain = pipeline.SolveLine(*six, extra={})
    assert pipeline.batch_snapshots([plain, a, b]) == (4, 9)
    with pytest.raises(ValueError):
        pipeline.batch_snapshots([a, plain, c])


def test_mid_steps():
    assert pipeline.mid_steps(3, 19) == [4, 9, 14]
    assert pipeline.mid_steps(1, 19) == [9]
    assert pipeline.mid_steps(2, 19) == [6, 12]
    assert pipeline.mid_steps(8, 19) == [2, 4, 6, 8, 10, 12, 14, 16]
    assert pipeline.mid_steps(1, 2) == [1]
    assert pipeline.mid_steps(3, 4) == [1, 2, 3]
    for K, n in ((0, 19), (-1, 19), (9, 19), (1, 1), (3, 3), (4, 4), (8, 8)):      # none, too many, a step 0, duplicates
        with pytest.raises(ValueError):
            pipeline.mid_steps(K, n)


def test_para_gen_mid_flags(capsys):
    import para_gen
    fl = helpers.para_gen_flags(["--mid", "3"])
    assert fl.mid == 3 and fl.mid_steps == [4, 9, 14]
    assert helpers.para_gen_flags([]).mid_steps == []
    for extra in (["--mid", "2", "--multseg"], ["--mid", "2", "--arap_bin", "/bin/true"], ["--mid", "9"], ["--mid", "-1"]):
        with pytest.raises(SystemExit):
            helpers.para_gen_flags(extra)
    assert "--multseg" in capsys.readouterr().err
    p = dict(rgb1_gen="a", msk1_gen="b", cstr_tmp="c", flow_gen="d", rgb2_gen="e", msk2_gen="f", mid_gen="/o/Mid/s/0001",
             _mid=(6, 12))
    assert pipeline.make_arap_path(p).extra == dict(mid="6,12:/o/Mid/s/0001")
    assert para_gen.mid_paths(p) == ["/o/Mid/s/0001_s06.flo", "/o/Mid/s/0001_s06.png", "/o/Mid/s/0001_s06_mask.png",
                                     "/o/Mid/s/0001_s06_step.flo", "/o/Mid/s/0001_s12.flo", "/o/Mid/s/0001_s12.png",
                                     "/o/Mid/s/0001_s12_mask.png", "/o/Mid/s/0001_s12_step.flo"]


def test_new_entry_points_exported():
    from arap_flow_amd import build, capi
    lib = ctypes.CDLL(build.build())
    for name in ("ArapFlow_SolverSetSnapshots", "ArapFlow_SolverGetSnapshot", "ArapFlow_SolverHostSnapshot",
                 "ArapFlow_WarpStep"):
        assert hasattr(lib, name), name
        assert name in {s[0] for s in capi.SYMBOLS}
    assert capi.MAX_SNAPSHOTS == pipeline.MAX_SNAPSHOTS == 8
