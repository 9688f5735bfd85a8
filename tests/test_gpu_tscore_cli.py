"""GPU: the `chain` and `tscore` list lines through both arap_deform twins (list file and --serve) and track_score_gen.py
(child processes), against the numpy twins tests/tscore_ref.py on the files those runs read."""
import os
import os.path as osp
import subprocess
import sys

import numpy as np
import pytest

import tscore_ref as R
from arap_flow_amd import build, flo, pipeline, trk
from test_tscore_host import make_tree

pytestmark = pytest.mark.gpu
ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
F = np.float32


def _env():
    return dict(os.environ, HIP_VISIBLE_DEVICES=os.environ.get("HIP_VISIBLE_DEVICES", "0"))


def _run(args, cwd, stdin=None):
    r = subprocess.run(args, cwd=cwd, env=_env(), capture_output=True, text=True, timeout=600, input=stdin)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_chain_and_tscore_lines_all_three_hosts_equal_the_twins(tmp_path):
    """a chain line with and without bwd=, then tscore lines on what it wrote and on a tracker's file, under (1, 1) and
    under the benchmark's raster: list mode, --serve and arap_deform.py write the same bytes, the twins'"""
    out, est, gts = make_tree(tmp_path)
    p = lambda n: str(tmp_path / n)
    gt_file = str(out / "Tracks" / "a" / "00000.trk")
    g = gts[("a", "00000")]
    fwd = [str(est / "a" / ("00000_l%d.flo" % j)) for j in range(3)]
    bwd = [str(est / "a" / ("00000_b%d.flo" % j)) for j in range(3)]
    scale = tuple(float(v) for v in R.TAPVID_854x480)

    def items(tag):
        return [pipeline.ChainLine(gt_file, tuple(fwd), (), p(tag + "_c0.trk")),
                pipeline.ChainLine(gt_file, tuple(fwd), tuple(bwd), p(tag + "_c1.trk")),
                pipeline.TScoreLine(gt_file, p(tag + "_c0.trk"), (1.0, 1.0), p(tag + "_t0.txt")),         # reads the first line's output
                pipeline.TScoreLine(gt_file, p(tag + "_c1.trk"), scale, p(tag + "_t1.txt")),
                pipeline.TScoreLine(gt_file, str(est / "a" / "00000.trk"), scale, p(tag + "_t2.txt"))]
    text = lambda tag: "".join(pipeline.format_line(it) + "\n" for it in items(tag))
    cpp = build.build_host()[0]
    (tmp_path / "cpp.txt").write_text(text("cpp"))
    printed = _run([cpp, p("cpp.txt")], str(tmp_path))
    assert printed.count("Saved") == 5
    served = _run([cpp, "--serve"], str(tmp_path), stdin=text("srv"))
    assert all("Done " + it.out in served.splitlines() for it in items("srv"))
    (tmp_path / "py.txt").write_text(text("py"))
    _run([sys.executable, osp.join(ROOT, "arap_deform.py"), p("py.txt")], str(tmp_path))
    flows, back = np.stack([flo.flow_read(q) for q in fwd]), np.stack([flo.flow_read(q) for q in bwd])
    chains = [R.chain_ref(flows, g["pos"][0]), R.chain_ref(flows, g["pos"][0], back)]
    assert (chains[0][1] != chains[1][1]).any() and (chains[0][1] == 255).any() and (chains[1][1] == 0).any()
    tracker = trk.read(str(est / "a" / "00000.trk"))
    tables = [R.track_score_ref(g["pos"], g["occ"], *chains[0]), R.track_score_ref(g["pos"], g["occ"], *chains[1], scale),
              R.track_score_ref(g["pos"], g["occ"], tracker["pos"], tracker["occ"], scale)]
    assert all(t[1:, 0, R.GT_VIS].min() > 0 for t in tables)
    for tag in ("cpp", "srv", "py"):
        for k in range(2):
            got = trk.read(p("%s_c%d.trk" % (tag, k)))
            assert (got["W"], got["H"]) == (g["W"], g["H"]) and got["pos"].shape == (4, 40, 2)
            assert np.array_equal(got["pos"], chains[k][0]) and np.array_equal(got["occ"], chains[k][1]), (tag, k)
        for k in range(3):
            assert open(p("%s_t%d.txt" % (tag, k))).read() == pipeline.format_track_score(tables[k]), (tag, k)
    # files that do not agree are an error of that line, at run time
    bad = [pipeline.TScoreLine(gt_file, str(out / "Tracks" / "a" / "00001.trk"), (1.0, 1.0), p("bad.txt")),        # F differs
           pipeline.ChainLine(gt_file, (str(est / "a" / "00000_l0.flo"), p("small.flo")), (), p("bad.trk"))]
    flo.flow_write(p("small.flo"), flows[0][:-1])
    for it in bad:
        (tmp_path / "bad.list").write_text(pipeline.format_line(it) + "\n")
        assert subprocess.run([cpp, p("bad.list")], cwd=str(tmp_path), env=_env(), capture_output=True).returncode == 1
        assert not osp.exists(it.out)


@pytest.mark.parametrize("from_flows", [False, True], ids=["tracks", "from_flows"])
def test_track_score_gen_over_a_synthetic_tree(tmp_path, from_flows):
    """two track files with an estimate and one without: the per-file tables are the twins', track_score.txt is their
    pooled table, the third file is listed as missing"""
    out, est, gts = make_tree(tmp_path)
    printed = _run([sys.executable, osp.join(ROOT, "track_score_gen.py"), "--data", str(out), "--est", str(est), "--tapvid"] +
                   (["--from_flows"] if from_flows else []), str(tmp_path))
    assert "2 track files scored, 1 without an estimate" in printed and "reappeared" in printed
    scale = (float(F(256) / F(12)), float(F(256) / F(9)))
    tables = []
    for seq in "ab":
        g = gts[(seq, "00000")]
        if from_flows:
            nf = len(g["pos"])
            flows = np.stack([flo.flow_read(str(est / seq / ("00000_l%d.flo" % j))) for j in range(nf - 1)])
            back = np.stack([flo.flow_read(str(est / seq / ("00000_b%d.flo" % j))) for j in range(nf - 1)]) if seq == "a" else None
            pos, occ = R.chain_ref(flows, g["pos"][0], back)
            e = trk.read(str(out / "TracksEst" / seq / "00000.trk"))
            assert np.array_equal(e["pos"], pos) and np.array_equal(e["occ"], occ)
        else:
            e = trk.read(str(est / seq / "00000.trk"))
        ref = R.track_score_ref(g["pos"], g["occ"], e["pos"], e["occ"], scale)
        assert open(out / "TrackScore" / seq / "00000.txt").read() == pipeline.format_track_score(ref), seq
        tables.append(ref)
    pooled = pipeline.add_track_scores(tables)
    assert pooled.shape == (4, 3, 16) and pooled[1:, 0, R.GT_VIS].min() > 0
    assert open(out / "track_score.txt").read() == pipeline.format_track_score(pooled)
    assert open(out / "track_score_missing.list").read() == str(out / "Tracks" / "a" / "00001.trk") + "\n"
