"""CPU: frame scoring (DESIGN.md "Frame scoring").  The `fscore` list line in Python and in C++ (host/list_line.h through
line_tool); the frame score file's text, pooling and summary; the numpy twin's own anchors and its two ways to the window
sums; the library's new entry point and the argument sets it refuses without a device."""
import ctypes as C
import math
import os.path as osp
import subprocess
import sys

import numpy as np
import pytest

import fscore_ref
from arap_flow_amd import capi, pipeline, scores

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
ONE = fscore_ref.ONE

# ---- the fscore line: host/list_line.h against pipeline.parse_line --------------------------------------------------------
_S = "fscore r.png e.png"
GOOD = [
    _S + " out=T", _S + " occ=O out=T", _S + " out=T obj=M", _S + " skip=S dist=D obj=M occ=O out=T",
    _S + " dist=a=b out=T", "fscore Mid/a/00001_m1.png est/a/00001_m1.png occ=MidOcc/a/00001_m1.png out=FrameScore/a/00001_m1.txt",
]
BAD = [
    _S, _S + " occ=O", "fscore r.png out=T", "fscore out=T", "fscore",                     # no out=; fewer than two paths
    _S + " foo=X out=T", _S + " out=T mask=A", _S + " extra out=T",                        # unknown keys, a stray word
    _S + " occ= out=T", _S + " out=", _S + " occ out=T",                                   # empty values, a missing `=`
    _S + " out=T out=U", _S + " occ=O occ=O out=T", _S + " obj=M out=T obj=N",             # repeated keys
    "fscore r=1 e.png out=T", "fscore r.png e=1 out=T",                                    # a token where a path is expected
]


@pytest.fixture(scope="module")
def bins():
    from arap_flow_amd import build
    return {osp.basename(o): o for o in build.build_host()}


def test_fscore_line_round_trip():
    item = pipeline.FScoreLine("r.png", "e.png", dict(obj="M", occ="O"), "T")
    text = pipeline.format_line(item)
    assert text == "fscore r.png e.png occ=O obj=M out=T" == pipeline.fscore_line(item)
    back = pipeline.parse_line(text)
    assert isinstance(back, pipeline.FScoreLine) and back == item._replace(planes=dict(occ="O", obj="M"))
    assert pipeline.done_token(back) == "T" and pipeline.format_line(back) == text
    for line in GOOD:
        it = pipeline.parse_line(line)
        assert isinstance(it, pipeline.FScoreLine) and pipeline.parse_line(pipeline.format_line(it)) == it
        assert pipeline.parse_fscore(line.split()) == it
    assert pipeline.parse_line(GOOD[4]).planes == dict(dist="a=b")                          # the first `=` splits
    assert pipeline.FSCORE_WORD == "fscore" and pipeline.FSCORE_KEYS == ("occ", "dist", "skip", "obj")
    for line in BAD:
        with pytest.raises(ValueError):
            pipeline.parse_line(line)


def test_fscore_line_parser_equals_python_twin(bins):
    """every line through line_tool in one process: a good one comes back as format_line(parse_line(line)) + its done
    token, a bad one as BAD after the grammar's own message -- and Python refuses exactly those"""
    corpus = GOOD + BAD
    r = subprocess.run([bins["line_tool"]], input="".join(c + "\n" for c in corpus), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")[:-1]
    got = [ln for ln in lines if not ln.startswith("Invalid")]
    assert len(got) == len(corpus)
    assert [ln for ln in lines if ln.startswith("Invalid")] == ["Invalid fscore line: " + b for b in BAD]
    for line, g in zip(GOOD, got):
        item = pipeline.parse_line(line)
        assert g == pipeline.format_line(item) + " done=" + pipeline.done_token(item), line
    assert got[0] == _S + " out=T done=T"
    assert got[len(GOOD):] == ["BAD"] * len(BAD)


def test_arap_deform_refuses_a_bad_fscore_line_before_any_gpu_call(bins, tmp_path):
    lst = tmp_path / "l.txt"
    lst.write_text("a b c d e f\n" + BAD[5] + "\n")
    r = subprocess.run([bins["arap_deform"], str(lst)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "Invalid fscore line: " + BAD[5] + "\n"
    r = subprocess.run([sys.executable, osp.join(ROOT, "arap_deform.py"), str(lst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "fscore line" in r.stdout


# ---- the table as text, pooled, summarised ----------------------------------------------------------------------------------
def hand_table():
    t = np.zeros((9, 7), np.uint64)
    t[0] = [100, 300, 60, 5, 10, 10 * ONE - 1048576, 1048576]      # psnr 10 log10(65025): mean squared error 1
    t[1] = [60, 0, 0, 0, 4, 4 * ONE, 0]                            # exact
    t[2] = [40, 300, 60, 5, 6, 6 * ONE - 1048576, 1048576]
    t[6] = [7, 21, 7, 1, 0, 0, 0]                                  # pixels without a window
    t[8, :2] = [3, 1]
    return t


def test_frame_score_file_round_trip():
    t = hand_table()
    text = pipeline.format_frame_score(t)
    lines = text.split("\n")
    assert lines[0] == "all count=100 sse=300 sad=60 max=5 windows=10 ssim_sum=19922944 ssim_worst=1048576"
    assert lines[3] == "d0-10 count=0 sse=0 sad=0 max=0 windows=0 ssim_sum=0 ssim_worst=0"
    assert lines[8] == "left_out pixels=3 windows=1" and lines[9] == "" and len(lines) == 10
    assert [ln.split(" ")[0] for ln in lines[:9]] == list(pipeline.FSCORE_ROWS)
    back = pipeline.parse_frame_score_file(text)
    assert back.dtype == np.uint64 and np.array_equal(back, t)
    big = t.copy()
    big[0, 1] = (1 << 64) - 1                                       # the whole range of a field survives the text
    assert np.array_equal(pipeline.parse_frame_score_file(pipeline.format_frame_score(big)), big)
    for broken in (text[:-1], text + "\n", text.replace("noc ", "nok "), text.replace("sad=", "sat="), text.replace("sse=300", "sse=-1", 1),
                   text.replace("ssim_worst=1048576\n", "ssim_worst=1048576 more=1\n", 1), text.replace("pixels=3", "pixels=3.0"),
                   text.replace("left_out pixels=3 windows=1", "left_out pixels=3"), ""):
        with pytest.raises(ValueError):
            pipeline.parse_frame_score_file(broken)


def test_summary_of_hand_made_tables():
    m = pipeline.frame_score_summary(hand_table())
    assert list(m) == list(pipeline.FSCORE_ROWS)
    assert m["all"]["psnr"] == pytest.approx(10 * math.log10(65025.0), abs=1e-12) and m["all"]["mae"] == 0.2
    assert m["all"]["ssim"] == pytest.approx(0.9, abs=1e-12) and m["all"]["ssim_min"] == 0.0
    assert m["noc"]["psnr"] == float("inf") and m["noc"]["mae"] == 0 and m["noc"]["ssim"] == 1.0 and m["noc"]["ssim_min"] == 1.0
    assert all(math.isnan(m["d0-10"][k]) for k in ("psnr", "mae", "ssim", "ssim_min")) and m["d0-10"]["count"] == 0
    assert m["obj"]["mae"] == pytest.approx(1 / 3) and math.isnan(m["obj"]["ssim"]) and math.isnan(m["obj"]["ssim_min"])
    assert m["left_out"] == dict(pixels=3, windows=1)


def test_pooling_two_tables_equals_the_table_of_both_frames():
    a, b = hand_table(), hand_table()
    b[0] = [5, 7, 3, 9, 2, 2 * ONE - 10, 7]
    b[8, :2] = [0, 5]
    s = pipeline.add_frame_scores([a, b])
    assert s.dtype == np.uint64 and list(s[0]) == [105, 307, 63, 9, 12, 12 * ONE - 1048586, 1048576] and list(s[8, :2]) == [3, 6]
    assert np.array_equal(pipeline.add_frame_scores([a]), a) and np.array_equal(pipeline.add_frame_scores([b, a]), s)
    assert not pipeline.add_frame_scores([]).any()
    # pooling is exact: the twin's table of two frames, pooled over the frames, against per-frame tables pooled
    rng = np.random.default_rng(2)
    ref = rng.integers(0, 256, (2, 11, 13, 3)).astype(np.uint8)
    est = np.clip(ref.astype(int) + rng.integers(-30, 31, ref.shape), 0, 255).astype(np.uint8)
    planes = dict(occ=rng.integers(0, 2, (2, 11, 13)).astype(np.uint8), dist=rng.integers(0, 30000, (2, 11, 13)).astype(np.uint16),
                  skip=(rng.random((2, 11, 13)) < 0.1).astype(np.uint8), obj=rng.integers(0, 2, (2, 11, 13)).astype(np.uint8) * 255)
    stacked = fscore_ref.fscore_ref(ref, est, **planes)["table"]
    singles = [fscore_ref.fscore_ref(ref[k], est[k], **{key: v[k] for key, v in planes.items()})["table"][0] for k in range(2)]
    assert np.array_equal(stacked[0], singles[0]) and np.array_equal(stacked[1], singles[1])
    pooled = pipeline.add_frame_scores(singles)
    want = stacked.sum(axis=0)
    want[:8, [3, 6]] = stacked[:, :8][:, :, [3, 6]].max(axis=0)
    assert np.array_equal(pooled, want) and pooled[0, 0] + pooled[8, 0] == 2 * 11 * 13 and pooled[0, 4] + pooled[8, 1] == 2 * 4 * 6


# ---- the twin's own anchors ---------------------------------------------------------------------------------------------------
def test_twin_anchors():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (12, 17, 3)).astype(np.uint8)
    r = fscore_ref.fscore_ref(a, a)
    assert (r["q"] == ONE).all() and r["q"].shape == (1, 5, 10) and ONE == 1 << 21
    assert list(r["table"][0, 0]) == [12 * 17, 0, 0, 0, 50, 50 * ONE, 0]
    assert (r["ssim"][0, 3:8, 3:13] == 1).all() and (np.delete(r["ssim"][0], np.s_[3:8], 0) == -2).all()
    z = np.zeros((8, 8, 3), np.uint8)
    r = fscore_ref.fscore_ref(z, z + np.uint8(255))
    assert r["q"].tolist() == [[[1048578]]]
    assert list(r["table"][0, 0]) == [64, 64 * 195075, 64 * 765, 255, 1, 1048578, ONE - 1048578]
    ck = ((np.indices((9, 10)).sum(axis=0) & 1) * 255).astype(np.uint8)[..., None].repeat(3, axis=-1)
    r = fscore_ref.fscore_ref(ck, 255 - ck)
    assert (r["ssim"][0, 3:5, 3:6] < -0.99).all() and (r["ssim"][0, 3:5, 3:6] > -1).all()
    assert np.array_equal(fscore_ref.luma(np.array([[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255]])), [255, 0, 77, 149, 29])    # (150 * 255 + 128) >> 8 = 149
    # the four integers of the extremes fit int32 (ssim_terms asserts it): all-255 against all-255, against all-0
    for lo, hi in ((255, 255), (0, 255), (255, 0)):
        fscore_ref.fscore_ref(z + np.uint8(lo), z + np.uint8(hi))
    with pytest.raises(AssertionError):
        fscore_ref.ssim_terms(*(np.array([v], np.int64) for v in (40000, 40000, 64 * 2 * 40000 * 625, 64 * 40000 * 625)))
    # no window: tables of pixels only
    r = fscore_ref.fscore_ref(a[:7], a[:7][:, ::-1])
    assert r["q"] is None and r["table"][0, 0, 0] == 7 * 17 and not r["table"][0, :, 4:].any() and (r["ssim"] == -2).all()


def test_cumulative_and_direct_window_sums_agree():
    rng = np.random.default_rng(4)
    ref = rng.integers(0, 256, (2, 13, 19, 3)).astype(np.uint8)
    est = np.clip(ref.astype(int) + rng.integers(-60, 61, ref.shape), 0, 255).astype(np.uint8)
    skip = (rng.random((2, 13, 19)) < 0.2).astype(np.uint8)
    fast = fscore_ref.fscore_ref(ref, est, skip=skip)
    slow = fscore_ref.fscore_ref(ref, est, skip=skip, sums=fscore_ref.window_sums_direct)
    assert np.array_equal(fast["table"], slow["table"]) and np.array_equal(fast["q"], slow["q"])
    assert np.array_equal(fast["ssim"].view(np.uint32), slow["ssim"].view(np.uint32))
    assert fast["q"].min() < ONE and fast["table"][0, 8, 1] > 0
    a, b = fscore_ref.luma(ref), fscore_ref.luma(est)
    for x, y in zip(fscore_ref.window_sums(a, b), fscore_ref.window_sums_direct(a, b)):
        assert np.array_equal(x, y)
    assert fscore_ref.window_sums(a, b)[0][1, 2, 5] == a[1, 2:10, 5:13].sum()


# ---- the library's new entry point ------------------------------------------------------------------------------------------
def test_new_entry_point_exported_and_refusals_without_a_device():
    lib = capi.load()
    names = [s[0] for s in capi.SYMBOLS]
    assert "ArapFlow_FrameScore" in names and lib.ArapFlow_FrameScore is not None
    header = open(osp.join(ROOT, "include", "arap_opt.h")).read()
    assert "#define ARAPFLOW_FSCORE_ROWS 9" in header and "#define ARAPFLOW_FSCORE_FIELDS 7" in header
    assert "int ArapFlow_FrameScore(Opt_State* state, unsigned W, unsigned H, unsigned n, const void* ref, const void* est," in header
    assert (capi.FSCORE_ROWS, capi.FSCORE_FIELDS) == (len(pipeline.FSCORE_ROWS), len(pipeline.FSCORE_FIELDS)) == (9, 7)
    src = open(osp.join(ROOT, "arap_flow_amd", "opt.py")).read()
    assert "from .scores import (SCORE_ROWS, SCORE_FIELDS, FSCORE_ROWS, FSCORE_FIELDS," in src          # opt's names are scores.py's
    assert scores.FSCORE_ROWS == ("all", "noc", "occ", "d0-10", "d10-60", "d60-140", "obj", "bg", "left_out")
    assert scores.FSCORE_FIELDS == ("count", "sse", "sad", "max", "windows", "ssim_sum", "ssim_worst")
    # refused before anything is read or launched: a stand-in for the state and the buffers is never dereferenced
    mem = C.create_string_buffer(4096)
    p = C.c_void_p(C.addressof(mem))
    at = lambda off: C.c_void_p(C.addressof(mem) + off)
    call = lambda state, W, H, n, ref, est, table, ssim=None: lib.ArapFlow_FrameScore(state, W, H, n, ref, est, None, None, None, None, table, ssim)
    assert call(None, 4, 4, 1, at(0), at(1024), at(2048)) == -1                         # a null state
    assert call(p, 4, 4, 1, None, at(1024), at(2048)) == -1 and call(p, 4, 4, 1, at(0), None, at(2048)) == -1
    assert call(p, 4, 4, 1, at(0), at(1024), None) == -1                                # null buffers
    assert call(p, 0, 4, 1, at(0), at(1024), at(2048)) == -1 and call(p, 4, 0, 1, at(0), at(1024), at(2048)) == -1
    assert call(p, 4, 4, 0, at(0), at(1024), at(2048)) == -1                            # zero sizes
    assert call(p, 1 << 16, 1 << 15, 1, at(0), at(1024), at(2048)) == -1                # W * H = 2^31
    assert call(p, 1 << 15, 1 << 15, 2, at(0), at(1024), at(2048)) == -1                # n * W * H = 2^31
    assert call(p, 0xffffffff, 0xffffffff, 0xffffffff, at(0), at(1024), at(2048)) == -1
    assert call(p, 4, 4, 1, at(0), at(1024), at(1024 + 40)) == -1                       # the table starts inside est
    assert call(p, 4, 4, 1, at(0), at(1024), at(2048), at(2048 + 8)) == -1              # ssim on the table
    assert call(p, 4, 4, 1, at(0), at(1024), at(2048), at(1024 - 60)) == -1             # ssim's last bytes on est
    assert not any(mem.raw)
