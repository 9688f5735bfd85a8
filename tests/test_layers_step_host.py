"""Layered in-between frames (DESIGN.md "Layered in-between frames") at the host layer, no GPU: the numpy restatement of
tests/layers_step_ref.py against the sequential statement of the definitions, its identities with the one-layer step and
the layered backward flow, a closed form, the input conditions of every multi-layer GPU case, the `layers` line's mid=
token and para_gen.py's --mid_layers flag."""
import ctypes
import os.path as osp
import sys

import numpy as np
import pytest

import layers_step_ref as sref
import mid_ref
import occ_layers_ref as lref
import occ_ref
from arap_flow_amd import pipeline
from helpers import para_gen_flags as _parse

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
TINY = [c for c in sref.MULTI if c[0] * c[1] <= 96] + [(9, 8, 2, 3, False)]


def _fields(W, H, n, seed, overlap):
    rgb, masks, fa, fb = sref.two_state_layers(W, H, n, seed, overlap=overlap)
    return masks, lref.fields_from_flows(fa), lref.fields_from_flows(fb)


@pytest.mark.parametrize("W,H,n,seed,overlap", TINY)
def test_restatement_equals_sequential_definitions(W, H, n, seed, overlap):
    assert W <= 12 and H <= 8 and n <= 4
    masks, A, B = _fields(W, H, n, seed, overlap)
    if overlap:
        assert ((masks == 0).sum(0) > 1).any()
    A[0, 1, 1] = (np.float32(np.nan), np.float32(1.0))           # a NaN position: its triangles draw nothing
    B[n - 1, 2, 2] = (np.float32(np.nan), np.float32(1.0))       # a NaN landing point counts as out of frame
    a, b = sref.layers_step_ref(masks, A, B), sref.layers_step_brute(masks, A, B)
    for k in ("step", "occlusion_step", "warped_mask"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert (a["occlusion_step"] == 255).any() and (a["occlusion_step"] == 0).any()


@pytest.mark.parametrize("W,H,n,seed,overlap", sref.MULTI)
def test_multi_layer_cases_exercise_what_is_new(W, H, n, seed, overlap):
    """the input conditions of every multi-layer case of the GPU tests, from the restatement alone"""
    masks, A, B = _fields(W, H, n, seed, overlap)
    got = sref.exercised(masks, A, B)
    assert got == dict(cross=True, same=True, out=True, moves=True), got


@pytest.mark.parametrize("W,H,seed,kind", [(9, 7, 2, "folded"), (40, 30, 3, "smooth"), (70, 50, 5, "folded")])
def test_one_layer_step_equals_single_layer_reference(W, H, seed, kind):
    rgb, mask, fa, fb = mid_ref.two_state_case(W, H, seed, kind)
    A, B = occ_ref.field_from_flow(fa), occ_ref.field_from_flow(fb)
    a = sref.layers_step_ref(mask[None], A[None], B[None])
    assert np.array_equal(a["step"], mid_ref.step_ref(mask, A, B))


@pytest.mark.parametrize("W,H,n,seed,overlap", sref.MULTI)
def test_second_state_at_rest_gives_the_layered_backward_flow(W, H, n, seed, overlap):
    masks, A, _ = _fields(W, H, n, seed, overlap)
    grid = np.stack([mid_ref.grid_field(W, H)] * n)
    a = sref.layers_step_ref(masks, A, grid)
    b = lref.layers_ref(None, masks, A)
    assert np.array_equal(a["step"], b["backward_flow"]) and np.array_equal(a["warped_mask"], b["warped_mask"])


@pytest.mark.parametrize("W,H,n,seed,overlap", sref.MULTI)
def test_composite_step_equals_merge_of_single_layer_steps(W, H, n, seed, overlap):
    masks, A, B = _fields(W, H, n, seed, overlap)
    assert np.array_equal(sref.layers_step_ref(masks, A, B)["step"], sref.merged_single_steps(masks, A, B))


def test_upper_rectangle_moves_over_resting_lower_one():
    """closed form: OccStep is 255 exactly on the lower-layer and background pixels the upper rectangle newly covers;
    the sequential statement confirms the set first"""
    masks, fa, fb, want = sref.rectangles_case()
    A, B = lref.fields_from_flows(fa), lref.fields_from_flows(fb)
    b = sref.layers_step_brute(masks, A, B)
    assert np.array_equal(b["occlusion_step"] == 255, want)
    covered = b["warped_mask"] != 0
    assert (want & covered).any() and (want & ~covered).any()     # lower-layer pixels and background pixels
    a = sref.layers_step_ref(masks, A, B, parts=True)
    assert np.array_equal(a["occlusion_step"], b["occlusion_step"]) and np.array_equal(a["step"], b["step"])
    assert not a["same"].any() and not a["out"].any()             # nothing but the cross-layer rule acts here
    assert not (sref.union_of_single(masks, A, B)[covered] == 255).any()


def test_owner_flow_is_the_owner_rule():
    masks = np.full((3, 2, 3), 255, np.uint8)
    masks[0, 0, :] = 0
    masks[1, 0, 1:] = 0
    masks[2, 1, 2] = 0
    flows = np.stack([np.full((2, 3, 2), v, np.float32) for v in (1, 2, 3)])
    got = pipeline.owner_flow(masks, flows)
    assert got.dtype == np.float32
    assert np.array_equal(got[..., 0], [[1, 2, 2], [0, 0, 3]]) and np.array_equal(got[..., 0], got[..., 1])
    assert np.array_equal(lref.owner_of(masks), [[0, 1, 1], [-1, -1, 2]])


LAY = "layers /a/r.png 2 /a/m1.png /o/f1.flo /a/m2.png /o/f2.flo"


def test_mid_token_round_trip_on_a_layers_line():
    assert pipeline.LAYER_KEYS[-1] == "mid" and pipeline.LAYER_KEYS[0] == "occ"
    text = LAY + " mid=6,12:/o/Mid/f occ=/o/o.png"
    spec = pipeline.parse_line(text)
    assert spec.out == dict(mid="6,12:/o/Mid/f", occ="/o/o.png")
    assert pipeline.done_token(spec) == "6,12:/o/Mid/f"          # the first output token on the line
    canonical = pipeline.format_line(spec)
    assert canonical == LAY + " occ=/o/o.png mid=6,12:/o/Mid/f"  # layers_line still writes occ first, mid last
    again = pipeline.parse_line(canonical)
    assert again.out == spec.out and pipeline.done_token(again) == "/o/o.png"
    assert pipeline.format_line(again) == canonical
    only = pipeline.parse_line(LAY + " mid=3:/o/p")               # mid alone is an output
    assert pipeline.done_token(only) == "3:/o/p"
    for bad in ("mid=", "mid=:/o/p", "mid=0:/o/p", "mid=3,3:/o/p", "mid=4,2:/o/p", "mid=3", "mid=x:/o/p",
                "mid=1,2,3,4,5,6,7,8,9:/o/p"):
        with pytest.raises(ValueError):
            pipeline.parse_line(LAY + " " + bad)


def test_mid_layer_files_and_mid_files_unchanged():
    assert pipeline.mid_layer_files("/o/Mid/f", 6) == dict(occ="/o/Mid/f_s06_occ.png")
    assert pipeline.mid_layer_files("/o/Mid/f", 0) == dict(occ="/o/Mid/f_s00_occ.png")
    assert sorted(pipeline.mid_files("/o/Mid/f", 6)) == ["flow", "mask", "rgb", "step"]


def _cpp_list(tmp_path, text):
    import subprocess
    from arap_flow_amd import build
    (tmp_path / "l.txt").write_text(text)
    return subprocess.run([build.build_host()[0], str(tmp_path / "l.txt")], capture_output=True, text=True, timeout=120)


def test_cpp_twin_reads_the_mid_token(tmp_path):
    """the C++ driver accepts the good forms (it then stops at the first input file, which does not exist) and refuses
    the malformed ones as parse_line does"""
    good = _cpp_list(tmp_path, LAY + " occ=/o/o.png mid=6,12:/o/Mid/f\n" + LAY + " mid=3:/o/p\n")
    assert good.returncode != 0 and "Invalid" not in good.stdout
    for bad in ("mid=", "mid=:/o/p", "mid=0:/o/p", "mid=3,3:/o/p", "mid=3"):
        r = _cpp_list(tmp_path, LAY + " " + bad + "\n")
        assert r.returncode == 1 and "Invalid layers line" in r.stdout, bad


def test_para_gen_mid_layers_flag(capsys):
    with pytest.raises(SystemExit):
        _parse(["--mid_layers", "2"])                             # needs --multseg
    with pytest.raises(SystemExit):
        _parse(["--multseg", "--mid_layers", "2", "--arap_bin", "/usr/bin/true"])     # a foreign driver
    with pytest.raises(SystemExit):
        _parse(["--multseg", "--mid_layers", "9"])
    capsys.readouterr()
    with pytest.raises(SystemExit):
        _parse(["--mid", "2", "--multseg"])                       # still refused, with a pointer
    assert "--mid_layers" in capsys.readouterr().err
    f = _parse(["--multseg", "--mid_layers", "2"])
    assert f.multseg and f.mid_layers == 2 and f.mid_layers_steps == [6, 12] and not f.mid and f.mid_steps == []
    f = _parse(["--multseg", "--mid_layers", "3", "--occ_layers",
                "--arap_bin", "%s %s" % (sys.executable, osp.join(ROOT, "arap_deform.py"))])
    assert f.mid_layers_steps == [4, 9, 14] and f.occ_layers
    assert _parse([]).mid_layers == 0


def test_para_gen_mid_layer_paths():
    import para_gen
    p = dict(midl_gen="/o/Mid/a/00000", _midl=(6, 12))
    four = ["/o/Mid/a/00000_s%02d%s" % (i, e) for i in (6, 12) for e in (".flo", ".png", "_mask.png", "_step.flo")]
    assert para_gen.mid_layer_paths(p) == four
    p[para_gen.LAYERS_OCC] = "/o/Occ/a/00000.png"
    assert para_gen.mid_layer_paths(p) == four + ["/o/Mid/a/00000_s%02d_occ.png" % i for i in (0, 6, 12)]
    assert para_gen.mid_layer_paths({}) == []


def test_new_entry_points_exported():
    from arap_flow_amd import build, capi
    lib = ctypes.CDLL(build.build())
    for name in ("ArapFlow_WarpLayersStepScratchBytes", "ArapFlow_WarpLayersStep"):
        assert hasattr(lib, name), name
        assert name in [s[0] for s in capi.SYMBOLS]
    lib.ArapFlow_WarpLayersStepScratchBytes.restype = ctypes.c_uint64
    N = 854 * 480
    got = lib.ArapFlow_WarpLayersStepScratchBytes(854, 480, 3)
    assert 48 * N + 4 <= got <= 48 * N + 4 + 6 * 256             # 48 bytes per pixel, parts aligned to 256
    assert got == lib.ArapFlow_WarpLayersStepScratchBytes(854, 480, 200)
