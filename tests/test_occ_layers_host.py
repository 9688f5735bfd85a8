"""Layered warp (DESIGN.md "Layered warp") at the host layer, no GPU: the numpy restatement of tests/occ_layers_ref.py
against the sequential statement of the definitions and against the host merges of single-layer results, the `layers`
list line, para_gen.py's --occ_layers flag and the library's new entry points."""
import ctypes
import os.path as osp
import sys

import numpy as np
import pytest

import occ_layers_ref as lref
import occ_ref
from arap_flow_amd import pipeline

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
KEYS = ("warped_rgb", "warped_mask", "backward_flow", "occlusion_bwd", "occlusion")

# (W, H, layers, seed, overlapping masks): folds and out-of-frame motion come with layered_case's flows
TINY = [(10, 8, 3, 2, False), (12, 7, 4, 3, False), (10, 8, 3, 4, True), (9, 9, 2, 5, False), (10, 8, 2, 6, False),
        (10, 8, 3, 7, False)]


@pytest.mark.parametrize("W,H,n,seed,overlap", TINY)
def test_restatement_equals_sequential_definitions(W, H, n, seed, overlap):
    rgb, masks, flows = lref.layered_case(W, H, n, seed, overlap=overlap)
    fields = lref.fields_from_flows(flows)
    fields[0, 1, 1] = (np.float32(np.nan), np.float32(1.0))      # a NaN warp position counts as out of frame
    if overlap:
        assert ((masks == 0).sum(0) > 1).any()
    a, b = lref.layers_ref(rgb, masks, fields), lref.layers_brute(rgb, masks, fields)
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    # the cases exercise what is new: the layered map is not what the layers give one by one
    assert (a["occlusion"] != lref.union_of_single(masks, fields)).any()
    assert (a["occlusion"] == 255).any() and (a["occlusion"] == 0).any()


@pytest.mark.parametrize("W,H,amp,seed", [(9, 7, 2.0, 2), (2, 2, 0.5, 3), (1, 5, 1.0, 4), (70, 50, 3.0, 5)])
def test_one_layer_equals_single_layer_reference(W, H, amp, seed):
    rgb, mask, fl = occ_ref.folded_case(W, H, amp, seed)
    field = occ_ref.field_from_flow(fl)
    a, b = lref.layers_ref(rgb, mask[None], field[None]), occ_ref.warp_ref(rgb, mask, field)
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("W,H,n,seed,overlap", TINY + [(90, 60, 3, 11, False), (64, 40, 5, 12, True)])
def test_composite_equals_host_merges(W, H, n, seed, overlap):
    rgb, masks, flows = lref.layered_case(W, H, n, seed, overlap=overlap)
    fields = lref.fields_from_flows(flows)
    a = lref.layers_ref(rgb, masks, fields)
    per = [occ_ref.warp_ref(rgb, masks[l], fields[l]) for l in range(n)]
    m = lref.host_merge(per, masks)
    for k in ("warped_rgb", "warped_mask", "backward_flow", "occlusion_bwd"):
        assert np.array_equal(a[k], m[k]), k


def test_upper_rectangle_over_resting_lower_one():
    """closed form: the upper layer, translated by whole pixels, hides the lower layer's vertices inside the closed
    translated rectangle, and nothing else; the lower layer never hides the upper one"""
    W, H = 16, 12
    masks = np.full((2, H, W), 255, np.uint8)
    masks[0, 2:10, 1:9] = 0                       # lower, at rest
    masks[1, 3:9, 10:15] = 0                      # upper, moves 6 to the left and 1 up: x 4..8, y 2..7
    flows = np.zeros((2, H, W, 2), np.float32)
    flows[1][masks[1] == 0] = (-6.0, -1.0)
    fields = lref.fields_from_flows(flows)
    a, b = lref.layers_ref(None, masks, fields), lref.layers_brute(None, masks, fields)
    assert np.array_equal(a["occlusion"], b["occlusion"])
    ys, xs = np.mgrid[0:H, 0:W]
    want = (masks[0] == 0) & (xs >= 4) & (xs <= 8) & (ys >= 2) & (ys <= 7)
    assert np.array_equal(b["occlusion"] == 255, want)
    assert not (lref.union_of_single(masks, fields) == 255).any()


def test_layers_line_round_trip_and_old_lines_unchanged(tmp_path):
    six = "r.png m.png c.txt f.flo w.png wm.png"
    lay = "layers /a/r.png 2 /a/m1.png /a/f1.flo /a/m2.png /a/f2.flo bwd=/o/b.flo occ=/o/o.png"
    (tmp_path / "l.txt").write_text("%s\n%s occ=/x.png\n%s\n%s tail\n" % (six, six, lay, six))
    assert pipeline.read_list(str(tmp_path / "l.txt")) == [tuple(six.split())] * 3
    assert [e for _, e in pipeline.read_list_ex(str(tmp_path / "l.txt"))] == [{}, dict(occ="/x.png"), {}]
    items = pipeline.read_list_items(str(tmp_path / "l.txt"))
    assert [i[0] for i in items] == ["solve", "solve", "layers", "solve"]
    spec = items[2][1]
    assert spec["rgb"] == "/a/r.png" and spec["layers"] == [("/a/m1.png", "/a/f1.flo"), ("/a/m2.png", "/a/f2.flo")]
    assert spec["out"] == dict(bwd="/o/b.flo", occ="/o/o.png")
    assert pipeline.layers_done_token(spec) == "/o/b.flo"        # the first output token on the line
    again = pipeline.parse_layers(pipeline.layers_line(spec["rgb"], spec["layers"], spec["out"]).split())
    assert again["layers"] == spec["layers"] and again["out"] == spec["out"]
    assert pipeline.layers_done_token(again) == "/o/o.png"       # layers_line writes occ first
    for bad in ("layers r.png 2 m1 f1 m2 f2",                     # no output
                "layers r.png 2 m1 f1 m2 occ=o.png",             # a layer short
                "layers r.png 0 occ=o.png", "layers r.png x m f occ=o.png", "layers r.png 1 m f junk",
                "layers r.png 1 m f occ="):
        with pytest.raises(ValueError):
            pipeline.parse_layers(bad.split())


def test_cpp_twin_refuses_a_bad_layers_line(tmp_path):
    import subprocess
    from arap_flow_amd import build
    (tmp_path / "l.txt").write_text("layers r.png 2 m1 f1 m2 f2\n")
    r = subprocess.run([build.build_host()[0], str(tmp_path / "l.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "Invalid layers line" in r.stdout


def _parse(extra):
    import para_gen
    return para_gen.parse(["--input", "in", "--output", "out", "--matches", "m"] + extra)


def test_para_gen_occ_layers_flag(capsys):
    with pytest.raises(SystemExit):
        _parse(["--occ_layers"])
    with pytest.raises(SystemExit):
        _parse(["--multseg", "--occ_layers", "--arap_bin", "/usr/bin/true"])
    capsys.readouterr()
    with pytest.raises(SystemExit):
        _parse(["--occ", "--multseg"])
    assert "--occ_layers" in capsys.readouterr().err
    f = _parse(["--multseg", "--occ_layers"])
    assert f.multseg and f.occ_layers and not f.occ
    f = _parse(["--multseg", "--occ_layers", "--bwd_flow",
                "--arap_bin", "%s %s" % (sys.executable, osp.join(ROOT, "arap_deform.py"))])
    assert f.occ_layers and f.bwd_flow


def test_workers_stay_open_for_an_owed_line():
    """GpuWorkers.close() before a frame's layers line exists: the end markers go behind the owed line"""
    import para_gen
    w = para_gen.GpuWorkers("true", [], 4, False, lambda p: None)
    w.threads = [None, None]                     # two workers' worth of end markers, no process
    w.owe()
    w.put("solve")
    w.close()
    assert w.lines.qsize() == 1                  # no marker yet
    w.put_owed("layers")
    assert [w.lines.get_nowait() for _ in range(4)] == ["solve", "layers", None, None]
    w2 = para_gen.GpuWorkers("true", [], 4, False, lambda p: None)
    w2.threads = [None]
    w2.close()
    assert w2.lines.get_nowait() is None


def test_new_entry_points_exported():
    from arap_flow_amd import build, capi
    lib = ctypes.CDLL(build.build())
    for name in ("ArapFlow_WarpLayersScratchBytes", "ArapFlow_WarpLayers"):
        assert hasattr(lib, name), name
        assert name in [s[0] for s in capi.SYMBOLS]
    lib.ArapFlow_WarpLayersScratchBytes.restype = ctypes.c_uint64
    N = 854 * 480
    assert lib.ArapFlow_WarpLayersScratchBytes(854, 480, 3) >= 8 * N + 4 * (N + 1) + 4 * N + 16 * N + N
