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
from helpers import para_gen_flags as _parse

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
    items = pipeline.read_list_items(str(tmp_path / "l.txt"))
    assert [isinstance(i, pipeline.SolveLine) for i in items] == [True, True, False, True]    # a layers line is no solve
    solves = items[:2] + items[3:]
    assert [ln[:6] for ln in solves] == [tuple(six.split())] * 3
    assert [ln.extra for ln in solves] == [{}, dict(occ="/x.png"), {}]
    spec = items[2]
    assert spec.rgb == "/a/r.png" and spec.layers == [("/a/m1.png", "/a/f1.flo"), ("/a/m2.png", "/a/f2.flo")]
    assert spec.out == dict(bwd="/o/b.flo", occ="/o/o.png")
    assert pipeline.done_token(spec) == "/o/b.flo"               # the first output token on the line
    again = pipeline.parse_layers(pipeline.layers_line(spec).split())
    assert again.layers == spec.layers and again.out == spec.out
    assert pipeline.done_token(again) == "/o/o.png"              # layers_line writes occ first
    for bad in BAD_LAYERS:
        with pytest.raises(ValueError):
            pipeline.parse_layers(bad.split())


BAD_LAYERS = ("layers r.png 2 m1 f1 m2 f2",                       # no output
              "layers r.png 2 m1 f1 m2 occ=o.png",               # a layer short
              "layers r.png 0 occ=o.png", "layers r.png x m f occ=o.png", "layers r.png 1 m f junk",
              "layers r.png 1 m f occ=")

SIX = "/a/r.png /a/m.png /a/c.txt /o/f.flo /o/w.png /o/wm.png"
LAY = "layers /a/r.png 2 /a/m1.png /o/f1.flo /a/m2.png /o/f2.flo"
# (line, what format_line makes of it, the path a worker reports it done by)
ALL3 = SIX + " bwd=/o/b.flo occ=/o/o.png occ_bwd=/o/ob.png"
LINES = [(SIX, SIX, "/o/f.flo"),
         (ALL3, ALL3, "/o/f.flo"),
         (SIX + " occ=/o/o.png tail", SIX + " occ=/o/o.png", "/o/f.flo"),             # an unknown token is dropped
         (LAY + " occ=/o/o.png bwd=/o/b.flo", LAY + " occ=/o/o.png bwd=/o/b.flo", "/o/o.png"),
         # outputs in another order than layers_line's: the worker reports the first ON THE LINE, the text is re-ordered
         (LAY + " mask2=/o/m2.png bwd=/o/b.flo occ=/o/o.png", LAY + " occ=/o/o.png bwd=/o/b.flo mask2=/o/m2.png",
          "/o/m2.png")]


def test_list_line_round_trip_and_done_token():
    """parse_line / format_line / done_token over both line forms: a line in canonical token order comes back as it
    was; the formatted text of any line is a fixed point and parses to the same item"""
    for text, canonical, done in LINES:
        item = pipeline.parse_line(text)
        assert pipeline.format_line(item) == canonical
        assert pipeline.done_token(item) == done
        assert pipeline.parse_line(text.split()) == item                       # tokens or text
        again = pipeline.parse_line(canonical)
        assert again == item and pipeline.format_line(again) == canonical
    assert pipeline.parse_line(LINES[2][0]).extra == dict(occ="/o/o.png")
    assert pipeline.done_token(pipeline.parse_line(LINES[4][1])) == "/o/o.png"  # ... of the re-ordered text: occ first
    for bad in BAD_LAYERS:
        with pytest.raises(ValueError):
            pipeline.parse_line(bad)
    with pytest.raises(ValueError, match="list line needs 6 paths"):
        pipeline.parse_line("only three paths")


def _cpp_list(tmp_path, text):
    import subprocess
    from arap_flow_amd import build
    (tmp_path / "l.txt").write_text(text)
    return subprocess.run([build.build_host()[0], str(tmp_path / "l.txt")], capture_output=True, text=True, timeout=120)


def test_cpp_twin_refuses_a_bad_layers_line(tmp_path):
    r = _cpp_list(tmp_path, "layers r.png 2 m1 f1 m2 f2\n")
    assert r.returncode == 1 and "Invalid layers line" in r.stdout


def test_cpp_twin_reads_the_same_lines(tmp_path):
    """the C++ driver's list reader accepts what format_line writes (it then stops at the first input file, which does
    not exist) and refuses every layers line that parse_line refuses"""
    good = _cpp_list(tmp_path, "".join(c + "\n" for _, c, _ in LINES))
    assert good.returncode != 0 and "Invalid" not in good.stdout
    for bad in BAD_LAYERS:
        r = _cpp_list(tmp_path, bad + "\n")
        assert r.returncode == 1 and "Invalid layers line: " + bad in r.stdout


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
