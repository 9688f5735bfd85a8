"""Backward flow and occlusion maps at the host layer, no GPU: the optional list-line tokens (both twins), the
para_gen.py flag refusals and the exact --multseg merge rule."""
import os.path as osp
import subprocess
import sys

import numpy as np
import pytest

from arap_flow_amd import pipeline
from helpers import para_gen_flags as _parse

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))


def test_extra_tokens_parse_and_old_lines_keep_their_meaning(tmp_path):
    six = "r.png m.png c.txt f.flo w.png wm.png"
    (tmp_path / "l.txt").write_text("%s\n%s bwd=/a/b.flo occ=/a/o.png junk occ_bwd=/a/ob.png\n%s extra words\n" %
                                    (six, six, six))
    ex = pipeline.read_list_items(str(tmp_path / "l.txt"))
    assert [ln[:6] for ln in ex] == [tuple(six.split())] * 3
    assert [ln.extra for ln in ex] == [{}, dict(bwd="/a/b.flo", occ="/a/o.png", occ_bwd="/a/ob.png"), {}]
    assert pipeline.parse_extra(["occ=", "bwd", "x=y"]) == {}
    e = dict(occ="o.png", bwd="b.flo")
    assert pipeline.parse_extra(pipeline.extra_tokens(e)) == e


@pytest.mark.parametrize("cmd", ["py", "cpp"])
def test_warp_image_tokens_both_twins(tmp_path, cmd):
    """a bad trailing token is a usage error; good tokens get past parsing (here to the missing input file)"""
    from arap_flow_amd import build
    prog = [sys.executable, osp.join(ROOT, "warp_image.py")] if cmd == "py" else [build.build_host()[1]]
    five = [str(tmp_path / n) for n in ("i.png", "m.png", "f.flo", "w.png", "wm.png")]
    bad = subprocess.run(prog + five + ["nonsense"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 1 and "Invalid Input!" in bad.stdout
    few = subprocess.run(prog + five[:4], capture_output=True, text=True, timeout=120)
    assert few.returncode == 1 and "Invalid Input!" in few.stdout
    good = subprocess.run(prog + five + ["bwd=" + str(tmp_path / "b.flo"), "occ=" + str(tmp_path / "o.png")],
                          capture_output=True, text=True, timeout=120)
    assert good.returncode != 0 and "Invalid Input!" not in good.stdout


def test_para_gen_refusals():
    with pytest.raises(SystemExit):
        _parse(["--occ", "--multseg"])
    for flag in ("--occ", "--bwd_flow"):
        with pytest.raises(SystemExit):
            _parse([flag, "--arap_bin", "/usr/bin/true"])
    f = _parse(["--bwd_flow", "--multseg"])
    assert f.bwd_flow and f.multseg and not f.occ
    f = _parse(["--bwd_flow", "--occ", "--arap_bin", "%s %s" % (sys.executable, osp.join(ROOT, "arap_deform.py"))])
    assert f.bwd_flow and f.occ
    f = _parse(["--arap_bin", "/usr/bin/true"])                    # no new flag: a foreign binary as before
    assert not f.bwd_flow and not f.occ


def test_multseg_backward_merge_rule():
    H, W = 3, 4
    covers = np.zeros((3, H, W), bool)
    objects = np.zeros((3, H, W), bool)
    bwds = np.stack([np.full((H, W, 2), k + 1, np.float32) for k in range(3)])
    covers[0, 0, :] = True
    covers[1, 0, 1:3] = True
    covers[2, 0, 2] = True
    covers[1, 1, 0] = True
    objects[0, 2, 0] = True                # uncovered object of segment 0 -> revealed
    objects[2, 2, 3] = True                # ... of segment 2
    objects[1, 0, 0] = True                # covered: not revealed
    bwd, occ = pipeline.merge_backward(bwds, covers, objects)
    want_layer = np.array([[1, 2, 3, 1], [2, 0, 0, 0], [0, 0, 0, 0]])
    assert np.array_equal(bwd[..., 0], want_layer) and np.array_equal(bwd[..., 1], want_layer)
    want_occ = np.zeros((H, W), np.uint8)
    want_occ[2, 0] = want_occ[2, 3] = 255
    assert np.array_equal(occ, want_occ)
