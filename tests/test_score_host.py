"""CPU: flow scoring (DESIGN.md "Flow scoring").  The `score` list line in Python and in C++ (host/list_line.h through
line_tool); the score file's text, pooling and summary; the band edges through the 8-bit distance file; score_gen.py with a
stand-in worker; the library's new entry point and the argument sets it refuses without a device."""
import ctypes as C
import os
import os.path as osp
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import score_ref
from arap_flow_amd import capi, flo, pipeline, scores

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
F = np.float32

# ---- the score line: host/list_line.h against pipeline.parse_line ---------------------------------------------------------
_S = "score g.flo e.flo"
GOOD = [
    _S + " out=T", _S + " occ=O out=T", _S + " out=T mask=M", _S + " skip=S dist=D occ=O mask=M out=T",
    _S + " dist=a=b out=T", "score Flow/a/00001.flo est/a/00001.flo dist=MBDist/a/00001.png out=Score/a/00001.txt",
]
BAD = [
    _S, _S + " occ=O", "score g.flo out=T", "score out=T", "score",                        # no out=; fewer than two paths
    _S + " foo=X out=T", _S + " out=T idx1=A", _S + " extra out=T",                        # unknown keys, a stray word
    _S + " occ= out=T", _S + " out=", _S + " occ out=T",                                   # empty values, a missing `=`
    _S + " out=T out=U", _S + " occ=O occ=O out=T", _S + " mask=M out=T mask=N",           # repeated keys
    "score g=1 e.flo out=T", "score g.flo e=1 out=T",                                      # a token where a path is expected
]


@pytest.fixture(scope="module")
def bins():
    from arap_flow_amd import build
    return {osp.basename(o): o for o in build.build_host()}


def test_score_line_round_trip():
    item = pipeline.ScoreLine("g.flo", "e.flo", dict(mask="M", occ="O"), "T")
    text = pipeline.format_line(item)
    assert text == "score g.flo e.flo occ=O mask=M out=T"
    back = pipeline.parse_line(text)
    assert isinstance(back, pipeline.ScoreLine) and back == item._replace(planes=dict(occ="O", mask="M"))
    assert pipeline.done_token(back) == "T" and pipeline.format_line(back) == text
    for line in GOOD:
        it = pipeline.parse_line(line)
        assert isinstance(it, pipeline.ScoreLine) and pipeline.parse_line(pipeline.format_line(it)) == it
    assert pipeline.parse_line(GOOD[4]).planes == dict(dist="a=b")                          # the first `=` splits


def test_score_line_parser_equals_python_twin(bins):
    """every line through line_tool in one process: a good one comes back as format_line(parse_line(line)) + its done
    token, a bad one as BAD after the grammar's own message -- and Python refuses exactly those"""
    corpus = GOOD + BAD
    r = subprocess.run([bins["line_tool"]], input="".join(c + "\n" for c in corpus), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")[:-1]
    got = [ln for ln in lines if not ln.startswith("Invalid")]
    assert len(got) == len(corpus)
    assert [ln for ln in lines if ln.startswith("Invalid")] == ["Invalid score line: " + b for b in BAD]
    for line, g in zip(GOOD, got):
        item = pipeline.parse_line(line)
        assert g == pipeline.format_line(item) + " done=" + pipeline.done_token(item), line
    assert got[0] == _S + " out=T done=T"
    for line, g in zip(BAD, got[len(GOOD):]):
        assert g == "BAD", line
        with pytest.raises(ValueError):
            pipeline.parse_line(line)


def test_arap_deform_refuses_a_bad_score_line_before_any_gpu_call(bins, tmp_path):
    lst = tmp_path / "l.txt"
    lst.write_text("a b c d e f\n" + BAD[5] + "\n")
    r = subprocess.run([bins["arap_deform"], str(lst)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "Invalid score line: " + BAD[5] + "\n"
    r = subprocess.run([sys.executable, osp.join(ROOT, "arap_deform.py"), str(lst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "score line" in r.stdout


# ---- the table as text, pooled, summarised ----------------------------------------------------------------------------------
def hand_table():
    t = np.zeros((10, 8), np.uint64)
    t[0] = [8, 8 * 4096 * 3 // 2, 6, 2, 1, 1, 0, 5 * 4096]          # 8 pixels, mean EPE 1.5
    t[1] = [6, 6 * 4096, 4, 0, 0, 0, 0, 2 * 4096]
    t[2] = [2, 6 * 4096, 2, 2, 1, 1, 0, 5 * 4096]
    t[6] = t[0]
    t[9, :2] = [3, 1]
    return t


def test_score_file_round_trip():
    t = hand_table()
    text = pipeline.format_score(t)
    lines = text.split("\n")
    assert lines[0] == "all count=8 sum=49152 n1=6 n3=2 n5=1 fl=1 nonfinite=0 max=20480"
    assert lines[3] == "d0-10 count=0 sum=0 n1=0 n3=0 n5=0 fl=0 nonfinite=0 max=0"
    assert lines[9] == "left_out skipped=3 gt_nonfinite=1" and lines[10] == "" and len(lines) == 11
    assert [ln.split(" ")[0] for ln in lines[:10]] == list(pipeline.SCORE_ROWS)
    back = pipeline.parse_score_file(text)
    assert back.dtype == np.uint64 and np.array_equal(back, t)
    big = t.copy()
    big[0, 1] = (1 << 64) - 1                                       # the whole range of a field survives the text
    assert np.array_equal(pipeline.parse_score_file(pipeline.format_score(big)), big)
    for broken in (text[:-1], text + "\n", text.replace("noc ", "nok "), text.replace("n3=", "n4="), text.replace("sum=49152", "sum=-1"),
                   text.replace("max=20480\n", "max=20480 more=1\n", 1), text.replace("skipped=3", "skipped=3.0")):
        with pytest.raises(ValueError):
            pipeline.parse_score_file(broken)


def test_add_scores_and_summary():
    a, b = hand_table(), hand_table()
    b[0] = b[6] = [2, 4096, 0, 0, 0, 0, 0, 3 * 4096 // 4]
    b[1], b[2] = b[0], 0
    b[9, :2] = [0, 5]
    s = pipeline.add_scores([a, b])
    assert s.dtype == np.uint64
    assert list(s[0]) == [10, 49152 + 4096, 6, 2, 1, 1, 0, 5 * 4096] and list(s[2]) == list(a[2]) and list(s[9]) == [3, 6, 0, 0, 0, 0, 0, 0]
    assert np.array_equal(pipeline.add_scores([a]), a) and np.array_equal(pipeline.add_scores([b, a]), s)
    assert not pipeline.add_scores([]).any()
    m = pipeline.score_summary(a)
    assert m["all"] == dict(count=8, epe=1.5, r1=0.75, r3=0.25, r5=0.125, fl=0.125)
    assert m["occ"]["epe"] == 3.0 and m["noc"]["epe"] == 1.0 and m["left_out"] == dict(skipped=3, gt_nonfinite=1)
    assert m["d0-10"]["count"] == 0 and np.isnan(m["d0-10"]["epe"]) and np.isnan(m["d0-10"]["fl"])
    assert list(m) == list(pipeline.SCORE_ROWS)
    # pooling is exact: the table of two frames side by side is the sum of theirs
    rng = np.random.default_rng(2)
    gt = (rng.normal(size=(2, 6, 7, 2)) * 20).astype(F)
    est = (gt + rng.normal(size=gt.shape) * 3).astype(F)
    occ = rng.integers(0, 2, (2, 6, 7)).astype(np.uint8)
    per = score_ref.score_ref(gt, est, occ=occ)["table"]
    both = score_ref.score_ref(np.concatenate(list(gt), 0), np.concatenate(list(est), 0), occ=np.concatenate(list(occ), 0))["table"][0]
    assert np.array_equal(pipeline.add_scores(per), both)


def test_the_distance_file_keeps_every_band():
    d2 = np.arange(65536, dtype=np.uint16)
    band = lambda d: (d >= 100).astype(int) + (d >= 3600) + (d >= 19600)
    back = pipeline.dist_from_png(pipeline.seg_dist_png(d2))
    assert back.dtype == np.uint16 and np.array_equal(band(back.astype(np.int64)), band(d2.astype(np.int64)))
    assert back[65535] == 65535 and back[0] == 0 and back[99] == 81 and back[100] == 100 and back[19599] == 139 * 139
    assert np.array_equal(pipeline.dist_from_png(np.array([0, 9, 10, 59, 60, 139, 140, 254, 255], np.uint8)),
                          [0, 81, 100, 3481, 3600, 19321, 19600, 64516, 65535])


def test_twin_by_hand():
    """four pixels worked by hand: exact, 3-4-5, a NaN estimate, a skipped one"""
    gt = np.array([[[0, 0], [3, 4], [30, 40], [1, 1]]], F)
    est = np.array([[[0, 0], [6, 8], [np.nan, 0], [9, 9]]], F)
    r = score_ref.score_ref(gt, est, occ=np.array([[0, 255, 0, 0]], np.uint8), dist=np.array([[99, 100, 19600, 0]], np.uint16),
                            skip=np.array([[0, 0, 0, 1]], np.uint8))
    t = r["table"][0]
    q5 = 5 * 4096
    assert list(t[0]) == [3, q5 + (1 << 24), 2, 2, 1, 2, 1, 1 << 24]
    assert list(t[1]) == [2, 1 << 24, 1, 1, 1, 1, 1, 1 << 24] and list(t[2]) == [1, q5, 1, 1, 0, 1, 0, q5]
    assert list(t[3]) == [1, 0, 0, 0, 0, 0, 0, 0] and list(t[4]) == list(t[2]) and not t[5].any()
    assert list(t[6]) == [2, q5, 1, 1, 0, 1, 0, q5] and not t[7].any() and t[8, 0] == 1 and list(t[9]) == [1, 0, 0, 0, 0, 0, 0, 0]
    assert r["err"][0, 0, 0] == 0 and r["err"][0, 0, 1] == 5 and np.isnan(r["err"][0, 0, 2]) and r["err"][0, 0, 3] == -1
    assert len(score_ref.contraction_pixels(16)) == 16


# ---- score_gen.py with a stand-in worker ------------------------------------------------------------------------------------
FAKE_WORKER = r'''
import sys
# stand-in for arap_deform --serve (no GPU): a score line's table comes from the numpy twin
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import score_ref
from arap_flow_amd import flo, pipeline
def run(line):
    it = pipeline.parse_line(line)
    plane = {k: pipeline.load_mask_red(p) for k, p in it.planes.items()}
    skip = None
    if "skip" in plane or "mask" in plane:
        skip = sum((plane[k] != 0).astype(np.uint8) for k in ("skip", "mask") if k in plane)
    dist = pipeline.dist_from_png(plane["dist"]) if "dist" in plane else None
    t = score_ref.score_ref(flo.flow_read(it.gt), flo.flow_read(it.est), plane.get("occ"), dist, skip)["table"][0]
    open(it.out, "w").write(pipeline.format_score(t))
    with open(%r, "a") as log:
        log.write(line)
print("Ready", flush=True)
for line in sys.stdin:
    run(line)
    print("Done " + pipeline.done_token(pipeline.parse_line(line)), flush=True)
'''


def _tree(tmp_path, full):
    """OUT with two pairs of sequence `a` and one of `b`; estimates for a/00000 and b/00000 only"""
    rng = np.random.default_rng(7)
    out, est = tmp_path / "out", tmp_path / "est"
    H, W = 6, 9
    flows = {}
    for seq, stem in (("a", "00000"), ("a", "00001"), ("b", "00000")):
        for d in ("Flow", "FlowFull", "inpMasks", "Occ", "OccFull", "MBDist"):
            os.makedirs(out / d / seq, exist_ok=True)
        gt = (rng.normal(size=(H, W, 2)) * 10).astype(F)
        flo.flow_write(str(out / "Flow" / seq / (stem + ".flo")), gt)
        flo.flow_write(str(out / "FlowFull" / seq / (stem + ".flo")), gt + F(1))
        mask = np.zeros((H, W, 3), np.uint8)
        mask[:, :3] = 255                                           # red != 0: not object
        Image.fromarray(mask).save(out / "inpMasks" / seq / (stem + ".png"))
        for d in ("Occ", "OccFull"):
            Image.fromarray((rng.integers(0, 2, (H, W)) * 255).astype(np.uint8), "L").save(out / d / seq / (stem + ".png"))
        if seq == "a":                                              # b has no distance file: the plane is left out there
            Image.fromarray(rng.integers(0, 256, (H, W)).astype(np.uint8), "L").save(out / "MBDist" / seq / (stem + ".png"))
        flows[(seq, stem)] = gt
        if stem == "00000":
            os.makedirs(est / seq, exist_ok=True)
            flo.flow_write(str(est / seq / (stem + ".flo")), (gt + rng.normal(size=gt.shape) * 2).astype(F))
    return out, est


@pytest.mark.parametrize("full", [False, True], ids=["objects", "full"])
def test_score_gen_with_a_stand_in_worker(tmp_path, full, capsys):
    sys.path.insert(0, ROOT)
    import score_gen
    out, est = _tree(tmp_path, full)
    fake, log = tmp_path / "fake.py", tmp_path / "lines.log"
    fake.write_text(FAKE_WORKER % (ROOT, osp.join(ROOT, "tests"), str(log)))
    own = "%s %s" % (sys.executable, osp.join(ROOT, "arap_deform.py"))
    flags = score_gen.parse(["--data", str(out), "--est", str(est), "--arap_bin", own, "--worker", "serve"] + (["--full"] if full else []))
    flags.arap_bin = "%s %s" % (sys.executable, fake)               # (the flags are checked against this repository's driver)
    pooled = score_gen.main(flags)
    lines = sorted(pipeline.parse_line(ln) for ln in log.read_text().splitlines())
    assert [(osp.basename(osp.dirname(it.gt)), sorted(it.planes)) for it in lines] == \
        [("a", sorted(["dist", "occ"] + ([] if full else ["mask"]))), ("b", sorted(["occ"] + ([] if full else ["mask"])))]
    gt_dir = "FlowFull" if full else "Flow"
    assert all(it.gt == str(out / gt_dir / s / "00000.flo") and it.planes["occ"] == str(out / ("OccFull" if full else "Occ") / s / "00000.png")
               for it, s in zip(lines, "ab"))
    tables = [pipeline.parse_score_file((out / "Score" / s / "00000.txt").read_text()) for s in "ab"]
    assert np.array_equal(pooled, pipeline.add_scores(tables))
    assert (out / "score.txt").read_text() == pipeline.format_score(pooled)
    assert (out / "score_missing.list").read_text() == str(out / gt_dir / "a" / "00001.flo") + "\n"
    assert int(pooled[0, 0]) == (2 * 6 * 6 if not full else 2 * 6 * 9) and int(pooled[9, 0]) == (2 * 6 * 3 if not full else 0)
    assert int(pooled[3:6, 0].sum()) <= 6 * 9 and tables[1][3:6].sum() == 0                  # b had no distance file
    printed = capsys.readouterr().out
    assert "2 pairs scored, 1 without an estimate" in printed and "s40+" in printed and "left out:" in printed


def test_score_gen_without_any_estimate(tmp_path, capsys):
    sys.path.insert(0, ROOT)
    import score_gen
    out, est = _tree(tmp_path, False)
    (out / "all_files.list").write_text("x y %s\nx y %s\n" % (out / "Flow" / "a" / "00001.flo", out / "Flow" / "b" / "00000.flo"))
    pooled = score_gen.main(score_gen.parse(["--data", str(out), "--est", str(tmp_path / "nothing")]))     # no worker is started
    assert not pooled.any() and (out / "score.txt").read_text() == pipeline.format_score(np.zeros((10, 8), np.uint64))
    assert (out / "score_missing.list").read_text().splitlines() == [str(out / "Flow" / "a" / "00001.flo"), str(out / "Flow" / "b" / "00000.flo")]
    with pytest.raises(SystemExit):
        score_gen.parse(["--data", str(out), "--est", str(est), "--arap_bin", "/bin/true"])


# ---- the library's new entry point ------------------------------------------------------------------------------------------
def test_new_entry_point_exported_and_refusals_without_a_device():
    lib = capi.load()
    names = [s[0] for s in capi.SYMBOLS]
    assert "ArapFlow_FlowScore" in names and lib.ArapFlow_FlowScore is not None
    header = open(osp.join(ROOT, "include", "arap_opt.h")).read()
    assert "#define ARAPFLOW_SCORE_ROWS 10" in header and "#define ARAPFLOW_SCORE_FIELDS 8" in header
    assert "int ArapFlow_FlowScore(Opt_State* state, unsigned W, unsigned H, unsigned n, const void* gt, const void* est," in header
    assert (capi.SCORE_ROWS, capi.SCORE_FIELDS) == (len(pipeline.SCORE_ROWS), len(pipeline.SCORE_FIELDS)) == (10, 8)
    src = open(osp.join(ROOT, "arap_flow_amd", "opt.py")).read()
    assert "from .scores import (SCORE_ROWS, SCORE_FIELDS," in src                          # opt's names are scores.py's
    assert scores.SCORE_ROWS == ("all", "noc", "occ", "d0-10", "d10-60", "d60-140", "s0-10", "s10-40", "s40+", "left_out")
    assert scores.SCORE_FIELDS == ("count", "sum", "n1", "n3", "n5", "fl", "nonfinite", "max")
    # refused before anything is read or launched: a stand-in for the state and the buffers is never dereferenced
    mem = C.create_string_buffer(4096)
    p = C.c_void_p(C.addressof(mem))
    at = lambda off: C.c_void_p(C.addressof(mem) + off)
    call = lambda state, W, H, n, gt, est, table, err=None: lib.ArapFlow_FlowScore(state, W, H, n, gt, est, None, None, None, table, err)
    assert call(None, 4, 4, 1, at(0), at(1024), at(2048)) == -1                         # a null state
    assert call(p, 4, 4, 1, None, at(1024), at(2048)) == -1 and call(p, 4, 4, 1, at(0), None, at(2048)) == -1
    assert call(p, 4, 4, 1, at(0), at(1024), None) == -1                                # null buffers
    assert call(p, 0, 4, 1, at(0), at(1024), at(2048)) == -1 and call(p, 4, 0, 1, at(0), at(1024), at(2048)) == -1
    assert call(p, 4, 4, 0, at(0), at(1024), at(2048)) == -1                            # zero sizes
    assert call(p, 1 << 16, 1 << 15, 1, at(0), at(1024), at(2048)) == -1                # W * H = 2^31
    assert call(p, 1 << 15, 1 << 15, 2, at(0), at(1024), at(2048)) == -1                # n * W * H = 2^31
    assert call(p, 0xffffffff, 0xffffffff, 0xffffffff, at(0), at(1024), at(2048)) == -1
    assert call(p, 4, 4, 1, at(0), at(1024), at(1024 + 64)) == -1                       # the table inside est
    assert call(p, 4, 4, 1, at(0), at(1024), at(2048), at(2048 + 8)) == -1              # err on the table
    assert not any(mem.raw)
