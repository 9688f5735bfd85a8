"""CPU: segment maps (DESIGN.md "Segment maps").  The numpy twin tests/seg_ref.py against its per-pixel statement and
against cases worked by hand; the `seg` list line in Python and in C++ (host/list_line.h through line_tool); para_gen.py
--seg with a stand-in worker (hand-out order, list contents, refusals, --resume); the new entry points of the library."""
import json
import os
import os.path as osp
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import bg_ref
import seg_ref
from arap_flow_amd import capi, pipeline

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
F = np.float32
FAR = seg_ref.FAR


# ---- the twin -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,moving,tau,radius", [(1, False, 1.0, 3), (3, True, 1.0, 16), (3, False, 0.0, 0), (1, True, 1e30, 1)])
def test_twin_equals_the_loop_statement(n, moving, tau, radius):
    W, H = 23, 11
    masks, flows, _, _ = seg_ref.seg_case(W, H, n, seed=n)
    G = Ginv = None
    if moving:
        M1 = bg_ref.similarity(3.0, 1.02, (1.5, -0.5), (W / 2, H / 2))
        M2 = bg_ref.similarity(-2.0, 0.97, (0.0, 1.0), (W / 2, H / 2))
        G, Ginv = (np.asarray(g, F) for g in bg_ref.maps_f64(M1, M2))
    a, b = seg_ref.seg_ref(masks, flows, tau, radius, G, Ginv), seg_ref.seg_loops(masks, flows, tau, radius, G, Ginv)
    for k in seg_ref.OUTPUTS:
        assert a[k].dtype == b[k].dtype and (a[k] == b[k]).all(), k
    assert (a["mb1"] != 0).any() and (a["dist1"] == 0).any()
    if tau == 1.0:
        assert (a["mb1"] == 0).any() and (a["mb2"] != 0).any()


def test_distance_by_hand():
    W, H = 9, 7
    ys, xs = np.mgrid[0:H, 0:W]
    for radius in (0, 1, 3, 254):
        mb = np.zeros((H, W), np.uint8)
        mb[0, W - 1] = 255                          # one boundary pixel in a corner: d2 = dx^2 + dy^2 where <= radius^2
        d2 = (xs - (W - 1)) ** 2 + ys ** 2
        want = np.where(d2 <= radius * radius, d2, FAR).astype(np.uint16)
        assert (seg_ref.distances(mb, radius) == want).all()
        assert (seg_ref.distances(np.zeros((H, W), np.uint8), radius) == FAR).all()         # no boundary at all
        assert (seg_ref.distances(np.full((H, W), 255, np.uint8), radius) == 0).all()       # every pixel a boundary
    mb = np.zeros((H, W), np.uint8)
    mb[3, 2] = mb[5, 8] = 255
    d = seg_ref.distances(mb, 0)                    # radius 0: the boundary itself, or the sentinel
    assert (d == np.where(mb != 0, 0, FAR)).all()
    assert (pipeline.seg_dist_png(np.array([0, 1, 3, 4, 8, 9, 64515, 64516, FAR], np.uint16)) ==
            [0, 1, 1, 2, 2, 3, 253, 254, 255]).all()


def test_boundaries_are_symmetric_and_catch_non_finite():
    rng = np.random.default_rng(3)
    flow = rng.normal(size=(11, 13, 2)).astype(F) * F(0.8)
    flow[4, 5, 1] = np.nan
    flow[8, 2, 0] = np.inf
    for tau in (0.0, 0.5, 1.0, 1e30):
        mb = seg_ref.boundaries(flow, tau) != 0
        with np.errstate(all="ignore"):
            tau2 = F(tau) * F(tau)
            for a, b in ((np.s_[:, 1:], np.s_[:, :-1]), (np.s_[1:, :], np.s_[:-1, :])):
                d = flow[a] - flow[b]
                jump = ~(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] <= tau2)
                assert (mb[a][jump] & mb[b][jump]).all()            # both sides of every flagged pair
        assert mb[4, 5] and mb[4, 4] and mb[3, 5] and mb[5, 5] and mb[4, 6]         # a NaN difference is never <= tau2
        if tau == 1e30:                             # tau * tau overflows to +inf: inf <= inf holds, only the NaN is left
            assert mb.sum() == 5
        else:                                       # a finite tau2: the infinite difference is a jump too
            assert mb[8, 2] and mb[8, 3] and mb[7, 2]
    flat = np.zeros((5, 6, 2), F)
    assert not seg_ref.boundaries(flat, 0.0).any()                  # d2 = 0 <= 0: a constant flow has no boundary at tau = 0


# ---- the seg line: host/list_line.h against pipeline.parse_line ---------------------------------------------------------
_M = "1,0,0,0,1,0,1.01,0.02,3,-0.02,1.01,-2.5"
_S = "seg 1 m1 f1"
GOOD = [
    _S + " s=1,140 idx1=A", _S + " mb2=B s=0.5,16 m=" + _M + " idx1=A dist2=C",           # done = B: the first output on the line
    _S + " s=0,0 dist1=C", "seg 2 m1 f1 m2 f2 s=1e-3,254 m=" + _M + " idx1=A idx2=B mb1=C mb2=D dist1=E dist2=G",
    _S + " s=0.100000001,8 dist2=D mb2=B", _S + " m=" + _M.replace("-2.5", "1e-3") + " s=2,5 idx2=B",
]
BAD = [
    _S + " s=1,140", _S + " idx1=A", _S + " m=" + _M + " idx1=A",                          # no output; no s=
    _S + " s=1,140 idx1=A foo=B", _S + " s=1,140 idx1=A rgb2=O",                           # unknown keys
    _S + " s=1,140 idx1=", _S + " s= idx1=A", _S + " s=1,140 idx1", _S + " s=1,140 m= idx1=A",       # empty values, a missing `=`
    _S + " s=1 idx1=A", _S + " s=1,140,1 idx1=A", _S + " s=,140 idx1=A", _S + " s=1, idx1=A",         # not two numbers
    _S + " s=1,255 idx1=A", _S + " s=1,14.0 idx1=A", _S + " s=1,-1 idx1=A", _S + " s=1,x idx1=A",
    _S + " s=-0.5,9 idx1=A", _S + " s=nan,9 idx1=A", _S + " s=inf,9 idx1=A", _S + " s=1e39,9 idx1=A", _S + " s=x,9 idx1=A",
    _S + " s=1,9 m=" + _M + ",4 idx1=A", _S + " s=1,9 m=" + _M[:-5] + " idx1=A",           # 13 and 11 numbers
    _S + " s=1,9 m=" + _M.replace("1.01", "nan") + " idx1=A", _S + " s=1,9 m=" + _M.replace("1.01", "1e39") + " idx1=A",
    _S + " s=1,9 m=" + _M.replace("1.01", "x") + " idx1=A",
    _S + " s=1,9 idx1=A idx1=B", _S + " s=1,9 s=1,9 idx1=A", _S + " s=1,9 m=" + _M + " m=" + _M + " idx1=A",     # repeated keys
    "seg 0 s=1,9 idx1=A", "seg 256 s=1,9 idx1=A", "seg x m1 f1 s=1,9 idx1=A", "seg 2 m1 f1 m2",
    "seg 2 m1 f1 s=1,9 idx1=A",                                                          # a token where a path is expected
    "seg",
]


@pytest.fixture(scope="module")
def bins():
    from arap_flow_amd import build
    return {osp.basename(o): o for o in build.build_host()}


def test_seg_line_round_trip():
    item = pipeline.SegLine([("m1", "f1"), ("m2", "f2")], 0.1, 140, tuple(float(F(v)) for v in _M.split(",")),
                            dict(dist2="D", idx1="A"))
    text = pipeline.format_line(item)
    back = pipeline.parse_line(text)
    assert back.tau == float(F(0.1)) and back.radius == 140 and back.m == item.m and back.layers == item.layers
    assert back.out == dict(idx1="A", dist2="D")
    assert pipeline.format_line(back) == text and pipeline.done_token(back) == "A"
    assert pipeline.done_token(pipeline.parse_line(GOOD[1])) == "B"
    plain = pipeline.parse_line(GOOD[0])
    assert plain.m == () and " m=" not in pipeline.format_line(plain)       # no m=: a static background, and none written
    for line in GOOD:
        assert isinstance(pipeline.parse_line(line), pipeline.SegLine)
        assert pipeline.parse_line(pipeline.format_line(pipeline.parse_line(line))) == pipeline.parse_line(line)


def test_seg_line_parser_equals_python_twin(bins):
    """every line through line_tool in one process: a good one comes back as format_line(parse_line(line)) + its done
    token, a bad one as BAD after the grammar's own message -- and Python refuses exactly those"""
    corpus = GOOD + BAD
    r = subprocess.run([bins["line_tool"]], input="".join(c + "\n" for c in corpus), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")[:-1]
    got = [ln for ln in lines if not ln.startswith("Invalid")]
    assert len(got) == len(corpus)
    assert [ln for ln in lines if ln.startswith("Invalid")] == ["Invalid seg line: " + b for b in BAD]
    for line, g in zip(GOOD, got):
        item = pipeline.parse_line(line)
        assert g == pipeline.format_line(item) + " done=" + pipeline.done_token(item), line
    assert got[1].endswith(" done=B") and got[0].endswith(" done=A") and got[2].endswith(" done=C")
    for line, g in zip(BAD, got[len(GOOD):]):
        assert g == "BAD", line
        with pytest.raises(ValueError):
            pipeline.parse_line(line)


def test_arap_deform_refuses_a_bad_seg_line_before_any_gpu_call(bins, tmp_path):
    lst = tmp_path / "l.txt"
    lst.write_text("a b c d e f\n" + BAD[13] + "\n")
    r = subprocess.run([bins["arap_deform"], str(lst)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "Invalid seg line: " + BAD[13] + "\n"
    r = subprocess.run([sys.executable, osp.join(ROOT, "arap_deform.py"), str(lst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "seg line" in r.stdout


# ---- para_gen --seg with a stand-in worker ------------------------------------------------------------------------------
FAKE_WORKER = r'''
import os, shutil, sys
# stand-in for arap_deform (no GPU): a solve line writes the files para_gen expects; a seg line REFUSES to run (exit 3)
# unless every file it names is there already, then writes its outputs; a bg line writes its flow; every line is logged
import numpy as np
from PIL import Image
sys.path.insert(0, %r)
from arap_flow_amd import flo as F, pipeline
LOG = %r
def run(line):
    item = pipeline.parse_line(line)
    with open(LOG, "a") as log:
        log.write(line.rstrip("\n") + "\n")
    if isinstance(item, pipeline.SegLine):
        for q in [q for pair in item.layers for q in pair]:
            if not os.path.exists(q):
                print("seg line before its inputs: " + q, flush=True)
                sys.exit(3)
        m = np.array(Image.open(item.layers[0][0]).convert("RGB"))[..., 0]
        for k in item.out:
            Image.fromarray(np.full(m.shape, 7, np.uint8), "L").save(item.out[k])
        return
    if isinstance(item, pipeline.BgLine):
        shutil.copy(item.flow, item.out[2])              # (out[1] is the pair's second frame itself, composited in place)
        return
    m = np.array(Image.open(item.mask).convert("RGB"))[..., 0]
    F.flow_write(item.flow, np.zeros(m.shape + (2,), np.float32))
    shutil.copy(item.rgb, item.out_rgb)
    Image.fromarray(m == 0).save(item.out_mask)
    for k in ("bwd",):
        if k in item.extra:
            F.flow_write(item.extra[k], np.zeros(m.shape + (2,), np.float32))
    for k in ("occ", "occ_bwd"):
        if k in item.extra:
            Image.fromarray(np.zeros(m.shape, np.uint8), "L").save(item.extra[k])
if sys.argv[1] == "--serve":
    print("Ready", flush=True)
    for line in sys.stdin:
        run(line)
        print("Done " + pipeline.done_token(pipeline.parse_line(line)), flush=True)
else:
    for l in open(sys.argv[1]).read().splitlines():
        if l.strip(): run(l)
'''
SEG_DIRS = dict(idx1="Index1", idx2="Index2", mb1="MB", mb2="MBBwd", dist1="MBDist", dist2="MBDistBwd")


def _seg_run(tmp_path, extra, worker, seg=()):
    sys.path.insert(0, ROOT)
    import para_gen
    from test_pipeline_host import _tiny_tree
    if not (tmp_path / "in").exists():
        _tiny_tree(tmp_path, nframes=4, seqs=("a", "b"))
    inp, mdir = tmp_path / "in", tmp_path / "matches"
    if not (tmp_path / "bgs").exists():
        os.makedirs(tmp_path / "bgs")
        Image.fromarray(np.random.default_rng(1).integers(0, 256, (50, 80, 3)).astype(np.uint8)).save(tmp_path / "bgs" / "b.png")
    fake, log = tmp_path / "fake_arap.py", tmp_path / "lines.log"
    if log.exists():
        log.unlink()
    fake.write_text(FAKE_WORKER % (ROOT, str(log)))
    outp = tmp_path / "out"
    own = "%s %s" % (sys.executable, osp.join(ROOT, "arap_deform.py"))
    flags = para_gen.parse(["--input", str(inp), "--output", str(outp), "--gpu", "0", "1", "--matches", str(mdir), "--worker", worker,
                            "--arap_bin", own, "--narap", "3", "--jobs", "2"] + extra + ["--seg"] + list(seg))
    flags.arap_bin = "%s %s" % (sys.executable, fake)          # (the flags are checked against this repository's driver)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        out = para_gen.main(flags)
    finally:
        os.chdir(cwd)
    return outp, out, [pipeline.parse_line(ln) for ln in (log.read_text().splitlines() if log.exists() else [])]


@pytest.mark.parametrize("worker,multseg,motion", [("serve", False, False), ("serve", True, True), ("batch", True, False)])
def test_para_gen_seg_with_a_stand_in_worker(tmp_path, worker, multseg, motion):
    """plain (no --bg_dir at all), and --multseg with and without --bg_motion"""
    extra = (["--multseg"] if multseg else []) + (["--bg_dir", str(tmp_path / "bgs"), "--bg_motion"] if motion else [])
    outp, out, lines = _seg_run(tmp_path, extra, worker, seg=("0.5", "16") if motion else ())
    assert len(out) == 6                                                    # 2 sequences x 3 pairs
    seg = [it for it in lines if isinstance(it, pipeline.SegLine)]
    solves = [it for it in lines if isinstance(it, pipeline.SolveLine)]
    bgs = [it for it in lines if isinstance(it, pipeline.BgLine)]
    assert len(seg) == 6 and len(solves) == (12 if multseg else 6) and len(bgs) == (6 if motion else 0)
    # a seg line names the frame's solves (the stand-in refuses one whose flows are not written yet: the run got here)
    assert sorted(f for it in seg for _, f in it.layers) == sorted(s.flow for s in solves)
    assert sorted(m for it in seg for m, _ in it.layers) == sorted(s.mask for s in solves)
    assert all(len(it.layers) == (2 if multseg else 1) and list(it.out) == list(SEG_DIRS) for it in seg)
    assert all((it.tau, it.radius) == ((0.5, 16) if motion else (1.0, 140)) for it in seg)
    flow_of = lambda it: it.out["idx1"].replace(osp.sep + "Index1" + osp.sep, osp.sep + "Flow" + osp.sep)[:-4] + ".flo"
    if motion:                                                              # the pair's own camera
        by_flow = {it.flow: it for it in bgs}
        assert all(it.m == by_flow[flow_of(it)].m and len(it.m) == 12 for it in seg)
        at = {id(it): k for k, it in enumerate(lines)}
        assert all(at[id(it)] < at[id(by_flow[flow_of(it)])] for it in seg)      # before the segments are merged and the bg line runs
    else:
        assert all(it.m == () for it in seg)
    st = json.load(open(outp / "arap_stats.json"))
    assert st["seg_done"] == 6 and st["frames_done"] == 6 and st["tex_done"] == 0 and st["blur_done"] == 0
    for pair in out:                                                        # six maps beside every listed pair, named like its flow
        flow = pair.split(" ")[2]
        for k, d in SEG_DIRS.items():
            q = flow.replace(osp.sep + "Flow" + osp.sep, osp.sep + d + osp.sep)[:-4] + ".png"
            assert (np.array(Image.open(q)) == 7).all(), q
    if multseg:                                                             # per-segment files were merged and removed
        assert not [f for f in os.listdir(outp / "Flow" / "a") if "_seg" in f]


def test_para_gen_seg_with_the_other_outputs(tmp_path):
    """together with --bwd_flow and --occ the solve lines keep their tokens and every pair still gets its seg line"""
    outp, out, lines = _seg_run(tmp_path, ["--bwd_flow", "--occ"], "serve")
    seg = [it for it in lines if isinstance(it, pipeline.SegLine)]
    solves = [it for it in lines if isinstance(it, pipeline.SolveLine)]
    assert len(out) == 6 and len(seg) == 6 and all({"bwd", "occ", "occ_bwd"} <= set(s.extra) for s in solves)


def test_para_gen_seg_resume(tmp_path):
    """--resume skips a pair only when its six maps exist too"""
    outp, out, lines = _seg_run(tmp_path, [], "serve")
    assert len(out) == 6
    gone = str(outp / "MBDistBwd" / osp.relpath(out[2].split(" ")[2], outp / "Flow"))[:-4] + ".png"
    os.remove(gone)
    outp, out2, lines = _seg_run(tmp_path, ["--resume"], "serve")
    seg = [it for it in lines if isinstance(it, pipeline.SegLine)]
    assert len(seg) == 1 and seg[0].out["dist2"] == gone and osp.exists(gone)
    outp, out3, lines = _seg_run(tmp_path, ["--resume"], "serve")
    assert lines == []                                                      # everything is there: nothing is handed out


def test_para_gen_without_seg_writes_nothing_of_it(tmp_path):
    sys.path.insert(0, ROOT)
    import helpers
    flags = helpers.para_gen_flags([])
    assert flags.seg is None
    assert helpers.para_gen_flags(["--seg"]).seg == (1.0, 140)
    assert helpers.para_gen_flags(["--seg", "0.1", "254", "--multseg", "--bg_dir", "b", "--bg_motion"]).seg == (float(F(0.1)), 254)
    import para_gen
    assert para_gen.scan(flags, str(tmp_path / "nothing"), str(tmp_path / "out")) == []
    from test_pipeline_host import _tiny_tree
    _tiny_tree(tmp_path, nframes=2, seqs=("a",))
    paths = para_gen.scan(flags, str(tmp_path / "in"), str(tmp_path / "out"))
    assert paths and not [k for e in paths for k in e if "seg" in k]
    with_seg = para_gen.scan(helpers.para_gen_flags(["--seg"]), str(tmp_path / "in"), str(tmp_path / "out"))
    assert sorted(k for k in with_seg[0] if k.endswith("_seg_gen")) == sorted(k + "_seg_gen" for k in SEG_DIRS)


def test_para_gen_refuses_seg(capsys):
    import helpers
    bg = ["--bg_dir", "b"]
    for extra in (["--mid", "2"], ["--multseg", "--mid_layers", "2"], bg + ["--retex"], bg + ["--blur", "0.5"], bg + ["--relight"],
                  bg + ["--bg_motion", "--mid", "2", "--mid_bg"], ["--arap_bin", "/bin/true"]):
        with pytest.raises(SystemExit):
            helpers.para_gen_flags(["--seg"] + extra)
        assert "--seg" in capsys.readouterr().err
    for seg in (["nan"], ["inf"], ["x"], ["1", "255"], ["1", "2.5"], ["1", "3", "4"]):
        with pytest.raises(SystemExit):
            helpers.para_gen_flags(["--seg"] + seg)
        assert "--seg" in capsys.readouterr().err


# ---- the library's new entry points -------------------------------------------------------------------------------------
def test_new_entry_points_exported():
    lib = capi.load()
    names = [s[0] for s in capi.SYMBOLS]
    for name in ("ArapFlow_SegMapsScratchBytes", "ArapFlow_SegMaps"):
        assert name in names and getattr(lib, name) is not None
    header = open(osp.join(ROOT, "include", "arap_opt.h")).read()
    assert "#define ARAPFLOW_SEG_MAX_RADIUS 254" in header and capi.SEG_MAX_RADIUS == pipeline.SEG_MAX_RADIUS == 254
    assert "ArapFlow_SegMaps(Opt_State* state" in header and "ArapFlow_SegMapsScratchBytes(unsigned W" in header
    # sizes the device call refuses have no scratch size (host only)
    for dims in ((0, 9, 3), (70, 0, 3), (70, 9, 0), (70, 9, 256), (1 << 16, 1 << 15, 1)):
        assert lib.ArapFlow_SegMapsScratchBytes(*dims) == 0
    up = lambda v: (v + 255) // 256 * 256
    N = 70 * 9
    assert lib.ArapFlow_SegMapsScratchBytes(70, 9, 1) == lib.ArapFlow_SegMapsScratchBytes(70, 9, 255) == 2 * up(8 * N) + 2 * up(N) + 256
