"""CPU: map scoring (DESIGN.md "Map scoring").  The numpy twin against the definitions as plain loops and on hand-worked
cases; the summaries on worked tables; the `lscore` and `mscore` list lines in Python and in C++ (host/list_line.h through
line_tool); the two files' text, round trips and pooling; the library's new entry points and the argument sets they refuse
without a device."""
import ctypes as C
import os.path as osp
import subprocess
import sys

import numpy as np
import pytest

import mscore_ref
from arap_flow_amd import capi, pipeline, scores

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
U8 = np.uint8


@pytest.fixture(scope="module")
def bins():
    from arap_flow_amd import build
    return {osp.basename(o): o for o in build.build_host()}


# ---- the twin ------------------------------------------------------------------------------------------------------------------
def test_twin_equals_the_plain_loops_at_23x11():
    rng = np.random.default_rng(5)
    W, H, L = 23, 11, 3
    gt = np.kron(rng.integers(0, 5, (3, 6)), np.ones((4, 4), int))[:H, :W].astype(U8)          # blocks of labels 0..4
    est = np.where(rng.random((H, W)) < 0.2, rng.integers(0, 6, (H, W)), np.roll(gt, 1, axis=1)).astype(U8)
    skip = (rng.random((H, W)) < 0.15).astype(U8) * 7
    for s in (None, skip):
        for radius in (0, 1, 3):
            t = mscore_ref.label_ref(gt, est, L, radius, s)["table"][0]
            assert t.tolist() == mscore_ref.label_loops(gt, est, L, radius, s)
    assert t[0, 3] > 0 and t[0, 4] > 0 and (t[1:, 5] > 0).all()
    t = mscore_ref.label_ref(gt, est, L, 0)["table"][0]
    assert (t[1:, 5] < t[1:, 3]).any() and (t[1:, 6] < t[1:, 4]).any()          # the case has misses for a radius to mend
    occ = (gt > 2).astype(U8) * 255
    score = rng.choice(np.array([0, 63, 64, 65, 200, 255], U8), size=(H, W))
    for s in (None, skip):
        r = mscore_ref.map_ref(occ, score, s, (64, 65, 255), 2)
        hist, mt = mscore_ref.map_loops(occ, score, s, (64, 65, 255), 2)
        assert r["hist"][0].tolist() == hist and r["match"][0].tolist() == mt
    assert int(r["hist"].sum()) + int((skip != 0).sum()) == W * H


def test_bmap_of_a_one_pixel_object_in_each_corner():
    """the edge rules differ there: a pixel sees its right, lower and lower-right neighbours only"""
    def b(y, x):
        m = np.zeros((4, 5), bool)
        m[y, x] = True
        return sorted(map(tuple, np.argwhere(mscore_ref.bmap(m)).tolist()))
    assert b(0, 0) == [(0, 0)]                                       # nothing looks back at it
    assert b(0, 4) == [(0, 3), (0, 4)]                               # its left neighbour, and itself looking down
    assert b(3, 0) == [(2, 0), (3, 0)]                               # the pixel above, and itself looking right
    assert b(3, 4) == [(2, 3), (2, 4), (3, 3)]                       # the bottom-right pixel itself is never boundary
    assert b(1, 2) == [(0, 1), (0, 2), (1, 1), (1, 2)]
    assert mscore_ref.bmap_loops(np.eye(4, 5, dtype=bool).tolist()) == mscore_ref.bmap(np.eye(4, 5, dtype=bool)).tolist()


def test_labels_present_on_one_side_only_and_the_zero_conventions():
    gt = np.zeros((6, 8), U8)
    est = np.zeros((6, 8), U8)
    gt[1:3, 1:3] = 1                     # label 1 only in gt
    est[3:5, 4:7] = 2                    # label 2 only in est; label 3 in neither
    # bmap of the 2 x 2 block: 5 pixels above and left of it that look at it, 3 of its own that look out; of the 2 x 3: 6 + 4
    t = mscore_ref.label_ref(gt, est, 3, 1)["table"][0]
    assert t[1].tolist() == [4, 0, 0, 8, 0, 0, 0, 0] and t[2, :5].tolist() == [0, 6, 0, 0, 10] and not t[3].any()
    assert t[0].tolist() == [48, 0, 38, 0, 0, 0, 0, 0]
    s = pipeline.label_score_summary(t)
    assert (s["labels"][1]["J"], s["labels"][1]["P"], s["labels"][1]["R"], s["labels"][1]["F"]) == (0.0, 1.0, 0.0, 0.0)
    assert (s["labels"][2]["J"], s["labels"][2]["P"], s["labels"][2]["R"], s["labels"][2]["F"]) == (0.0, 0.0, 1.0, 0.0)
    assert s["labels"][3] == dict(J=1.0, P=1.0, R=1.0, F=1.0)        # an empty union
    assert s["J"] == 1 / 3 and s["F"] == 1 / 3 and s["JF"] == 1 / 3 and s["frame"]["equal"] == 38


def test_radius_zero_a_perfect_estimate_and_a_skipped_only_match():
    gt = np.zeros((7, 9), U8)
    gt[2:5, 2:6] = 1
    est = np.roll(gt, 1, axis=1)
    t0 = mscore_ref.label_ref(gt, est, 1, 0)["table"][0, 1]
    t1 = mscore_ref.label_ref(gt, est, 1, 1)["table"][0, 1]
    assert t0[3] == t1[3] == t0[4] and 0 < t0[5] < t0[3] and t1[5] == t1[3] and t1[6] == t1[4]    # radius 0: the same pixel
    p = mscore_ref.label_ref(gt, gt, 1, 0)["table"][0]
    assert p[1, 0] == p[1, 1] == p[1, 2] == 12 and p[1, 3] == p[1, 4] == p[1, 5] == p[1, 6] > 0 and p[0, 2] == 63
    s = pipeline.label_score_summary(p)
    assert s["J"] == s["F"] == s["JF"] == 1.0
    # two single boundary pixels two apart; skipping the estimate's removes the only match of the ground truth's
    g = np.zeros((5, 9), U8)
    e = np.zeros((5, 9), U8)
    g[2, 2] = 255
    e[2, 4] = 255
    e[0, 8] = 255
    skip = np.zeros((5, 9), U8)
    assert mscore_ref.map_ref(g, e, None, (128,), 2)["match"][0, 0].tolist() == [1, 2, 1, 1]
    skip[2, 4] = 1
    assert mscore_ref.map_ref(g, e, skip, (128,), 2)["match"][0, 0].tolist() == [1, 1, 0, 0]
    assert mscore_ref.map_ref(g, e, None, (128,), 1)["match"][0, 0].tolist() == [1, 2, 0, 0]


def test_a_threshold_below_at_and_above_a_value():
    g = np.array([[255, 0, 255, 0]], U8)
    e = np.array([[100, 100, 99, 101]], U8)
    r = mscore_ref.map_ref(g, e, None, (99, 100, 101), 0)
    assert r["match"][0].tolist() == [[2, 4, 2, 2], [2, 3, 1, 1], [2, 1, 0, 0]]
    assert r["hist"][0, 1, 99] == r["hist"][0, 1, 100] == r["hist"][0, 0, 100] == r["hist"][0, 0, 101] == 1 and r["hist"].sum() == 4


# ---- summaries -------------------------------------------------------------------------------------------------------------------
def test_ap_and_best_f_of_a_worked_histogram():
    hist = np.zeros((2, 256), np.uint64)
    hist[1, 200], hist[1, 100], hist[1, 0] = 2, 1, 1             # 4 positives: two sure, one weak, one missed
    hist[0, 150], hist[0, 0] = 1, 5                              # one false alarm between them
    s = pipeline.map_score_summary(dict(hist=hist, thr=(128,), match=[[4, 3, 2, 3]]))
    assert (s["pos"], s["neg"]) == (4, 6)
    assert s["P"][201] == 1.0 and s["R"][201] == 0.0             # nothing predicted
    assert s["P"][200] == 1.0 and s["R"][200] == 0.5 and s["P"][150] == 2 / 3 and s["R"][150] == 0.5
    assert s["P"][100] == 0.75 and s["R"][100] == 0.75 and s["P"][1] == 0.75
    # AP: recall rises by 0.5 at t = 200 (P = 1) and by 0.25 at t = 100 (P = 0.75)
    assert s["ap"] == 0.5 * 1.0 + 0.25 * 0.75
    assert s["best_f"] == 0.75 and s["best_t"] == 1 and s["f128"] == 2 * (2 / 3) * 0.5 / (2 / 3 + 0.5)
    assert s["match"] == {128: dict(P=1.0, R=0.5, F=2 * 0.5 / 1.5)}
    perfect = np.zeros((2, 256), np.uint64)
    perfect[1, 255], perfect[0, 0] = 7, 9
    s = pipeline.map_score_summary(dict(hist=perfect, thr=(), match=[]))
    assert s["ap"] == 1.0 and s["best_f"] == 1.0 and s["f128"] == 1.0 and s["match"] == {}
    conv = pipeline.map_score_summary(dict(hist=perfect, thr=(1, 2, 3), match=[[3, 0, 0, 0], [0, 3, 0, 0], [0, 0, 0, 0]]))["match"]
    assert conv == {1: dict(P=1.0, R=0.0, F=0.0), 2: dict(P=0.0, R=1.0, F=0.0), 3: dict(P=1.0, R=1.0, F=1.0)}


# ---- the two lines: host/list_line.h against pipeline.parse_line ----------------------------------------------------------------
_L, _M = "lscore g.png e.png", "mscore g.png e.png"
GOOD = [
    _L + " l=3 r=8 out=T", _L + " out=T r=0 l=255", _L + " l=1 r=254 skip=S out=T", _L + " skip=a=b l=2 r=1 out=T",
    "lscore Index2/a/00001.png est/Index2/a/00001.png l=2 r=8 out=MapScore/Index2/a/00001.txt",
    _M + " out=T", _M + " skip=S out=T", _M + " t=64,128,192 r=8 out=T", _M + " r=0 t=1 out=T skip=S",
    _M + " t=1,2,3,4,5,6,7,255 r=254 out=T", _M + " t=7,7 r=1 out=T",
]
BAD_L = [
    _L, _L + " l=3 r=8", "lscore g.png l=3 r=8 out=T", "lscore", _L + " l=3 out=T", _L + " r=8 out=T",        # no out=, l=, r=; one path
    _L + " l=0 r=8 out=T", _L + " l=256 r=8 out=T", _L + " l=3 r=255 out=T", _L + " l=-1 r=8 out=T", _L + " l=3 r=1.0 out=T",
    _L + " l=+3 r=8 out=T", _L + " l=3 r=8 t=5 out=T", _L + " l=3 r=8 foo=1 out=T", _L + " l=3 r=8 extra out=T",
    _L + " l= r=8 out=T", _L + " l=3 r=8 out=", _L + " l=3 r=8 skip= out=T",
    _L + " l=3 l=3 r=8 out=T", _L + " l=3 r=8 out=T out=U", _L + " l=3 r=8 skip=S skip=S out=T",
    "lscore g=1 e.png l=3 r=8 out=T", "lscore g.png e=1 l=3 r=8 out=T",
]
BAD_M = [
    _M, "mscore g.png out=T", "mscore", _M + " t=64 out=T", _M + " r=8 out=T",                                  # t= without r= and the reverse
    _M + " t=0 r=8 out=T", _M + " t=256 r=8 out=T", _M + " t=64, r=8 out=T", _M + " t=,64 r=8 out=T", _M + " t=64,,65 r=8 out=T",
    _M + " t=1,2,3,4,5,6,7,8,9 r=8 out=T", _M + " t=64 r=255 out=T", _M + " t=6.4 r=8 out=T", _M + " t=64 r=-1 out=T",
    _M + " l=3 out=T", _M + " foo=1 out=T", _M + " extra out=T", _M + " t= r=8 out=T", _M + " t=64 r= out=T", _M + " out=",
    _M + " out=T out=U", _M + " t=64 t=65 r=8 out=T", _M + " t=64 r=8 r=8 out=T", "mscore g=1 e.png out=T", "mscore g.png e=1 out=T",
]


def test_line_round_trips():
    item = pipeline.LScoreLine("g.png", "e.png", 3, 8, None, "T")
    assert pipeline.format_line(item) == _L + " l=3 r=8 out=T" == pipeline.lscore_line(item)
    assert pipeline.parse_line(GOOD[1]) == item._replace(L=255, radius=0)
    assert pipeline.parse_line(GOOD[3]).skip == "a=b"                                       # the first `=` splits
    m = pipeline.MScoreLine("g.png", "e.png", (64, 128, 192), 8, None, "T")
    assert pipeline.format_line(m) == _M + " t=64,128,192 r=8 out=T" == pipeline.mscore_line(m)
    assert pipeline.parse_line(_M + " out=T") == pipeline.MScoreLine("g.png", "e.png", (), None, None, "T")
    assert pipeline.format_line(pipeline.parse_line(GOOD[8])) == _M + " t=1 r=0 skip=S out=T"
    for line in GOOD:
        it = pipeline.parse_line(line)
        assert isinstance(it, (pipeline.LScoreLine, pipeline.MScoreLine))
        assert pipeline.parse_line(pipeline.format_line(it)) == it and pipeline.done_token(it) == it.out
    assert (pipeline.LSCORE_WORD, pipeline.MSCORE_WORD, pipeline.MSCORE_MAX_THR) == ("lscore", "mscore", 8)
    for line in BAD_L + BAD_M:
        with pytest.raises(ValueError):
            pipeline.parse_line(line)


def test_line_parser_equals_python_twin(bins):
    """every line through line_tool in one process: a good one comes back as format_line(parse_line(line)) + its done
    token, a bad one as BAD after the grammar's own message -- and Python refuses exactly those"""
    corpus = GOOD + BAD_L + BAD_M
    r = subprocess.run([bins["line_tool"]], input="".join(c + "\n" for c in corpus), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")[:-1]
    got = [ln for ln in lines if not ln.startswith("Invalid")]
    assert len(got) == len(corpus)
    assert [ln for ln in lines if ln.startswith("Invalid")] == \
        ["Invalid lscore line: " + b for b in BAD_L] + ["Invalid mscore line: " + b for b in BAD_M]
    for line, g in zip(GOOD, got):
        item = pipeline.parse_line(line)
        assert g == pipeline.format_line(item) + " done=" + pipeline.done_token(item), line
    assert got[0] == _L + " l=3 r=8 out=T done=T" and got[5] == _M + " out=T done=T"
    assert got[len(GOOD):] == ["BAD"] * (len(BAD_L) + len(BAD_M))


@pytest.mark.parametrize("bad,word", [(BAD_L[6], "lscore"), (BAD_M[3], "mscore")])
def test_arap_deform_refuses_a_bad_line_before_any_gpu_call(bins, tmp_path, bad, word):
    lst = tmp_path / "l.txt"
    lst.write_text("a b c d e f\n" + bad + "\n")
    r = subprocess.run([bins["arap_deform"], str(lst)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "Invalid %s line: %s\n" % (word, bad)
    r = subprocess.run([sys.executable, osp.join(ROOT, "arap_deform.py"), str(lst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and word + " line" in r.stdout


# ---- the files: text, round trip, pooling ------------------------------------------------------------------------------------
def test_label_score_file_round_trip_and_pooling_with_different_L():
    a = np.zeros((3, 8), np.uint64)
    a[0, :5] = [40, 2, 30, 1, 0]
    a[1, :7] = [10, 12, 9, 6, 7, 5, 6]
    a[2, :7] = [(1 << 63) + 5, 0, 0, 3, 0, 0, 0]
    text = pipeline.format_label_score(a)
    assert text == ("frame counted=40 skipped=2 equal=30 gt_above=1 est_above=0\n"
                    "label 1 gt=10 est=12 inter=9 gt_b=6 est_b=7 gt_hit=5 est_hit=6\n"
                    "label 2 gt=9223372036854775813 est=0 inter=0 gt_b=3 est_b=0 gt_hit=0 est_hit=0\n")
    assert np.array_equal(pipeline.parse_label_score_file(text), a)
    for bad in (text[:-1], text + "\n", text.replace("label 2", "label 3"), text.replace("equal", "same"), text.replace("=12", "=-12"),
                text.replace("gt=10 ", ""), "frame counted=1 skipped=0 equal=1 gt_above=0 est_above=0\n"):
        with pytest.raises(ValueError):
            pipeline.parse_label_score_file(bad)
    b = np.zeros((2, 8), np.uint64)
    b[0, :5] = [10, 0, 10, 0, 0]
    b[1, :7] = [4, 4, 4, 3, 3, 3, 3]
    pooled = pipeline.add_label_scores([a, b])
    want = a.copy()
    want[:2] += b
    assert pooled.dtype == np.uint64 and np.array_equal(pooled, want) and np.array_equal(pipeline.add_label_scores([b, a]), want)
    # pooling is the table of both maps together
    rng = np.random.default_rng(1)
    g, e = rng.integers(0, 3, (2, 9, 12)).astype(U8), rng.integers(0, 3, (2, 9, 12)).astype(U8)
    t = mscore_ref.label_ref(g, e, 2, 2)["table"]
    both = mscore_ref.label_ref(np.concatenate([g[0], np.zeros((3, 12), U8), g[1]]), np.concatenate([e[0], np.zeros((3, 12), U8), e[1]]), 2, 2)
    assert np.array_equal(pipeline.add_label_scores(t)[1:, :3], both["table"][0, 1:, :3])
    assert mscore_ref.label_text(g[0], e[0], 2, 2) == pipeline.format_label_score(t[0])


def test_map_score_file_round_trip_and_pooling():
    rng = np.random.default_rng(2)
    g = (rng.random((2, 7, 10)) < 0.3).astype(U8) * 255
    e = rng.integers(0, 256, (2, 7, 10)).astype(U8)
    r = mscore_ref.map_ref(g, e, None, (64, 200), 1)
    scores = [dict(hist=r["hist"][i], thr=(64, 200), match=r["match"][i]) for i in range(2)]
    text = pipeline.format_map_score(scores[0])
    assert text == mscore_ref.map_text(g[0], e[0], None, (64, 200), 1)
    lines = text.split("\n")
    assert len(lines) == 5 and lines[0].startswith("neg ") and lines[1].startswith("pos ") and lines[2].startswith("match thr=64 a=")
    back = pipeline.parse_map_score_file(text)
    assert np.array_equal(back["hist"], scores[0]["hist"]) and back["thr"] == (64, 200) and np.array_equal(back["match"], scores[0]["match"])
    plain = pipeline.format_map_score(dict(hist=r["hist"][0], thr=(), match=np.zeros((0, 4), np.uint64)))
    assert plain == "\n".join(lines[:2]) + "\n" and pipeline.parse_map_score_file(plain)["thr"] == ()
    for bad in (text[:-1], text + "\n", text.replace("neg ", "neg 1 ", 1), text.replace("thr=64", "thr=0"), text.replace("a_hit", "hit"),
                text.replace("pos ", "Pos "), lines[0] + "\n"):
        with pytest.raises(ValueError):
            pipeline.parse_map_score_file(bad)
    pooled = pipeline.add_map_scores(scores)
    assert np.array_equal(pooled["hist"], r["hist"].sum(axis=0)) and np.array_equal(pooled["match"], r["match"].sum(axis=0))
    both = mscore_ref.map_ref(np.concatenate([g[0], np.zeros((3, 10), U8), g[1]]), np.concatenate([e[0], np.zeros((3, 10), U8), e[1]]))
    both["hist"][0, 0, 0] -= 30                                     # the spacer rows
    assert np.array_equal(pooled["hist"], both["hist"][0])
    with pytest.raises(ValueError):
        pipeline.add_map_scores([scores[0], dict(scores[1], thr=(64, 201))])


# ---- the library's new entry points ------------------------------------------------------------------------------------------
def test_new_entry_points_exported_and_refusals_without_a_device():
    lib = capi.load()
    names = [s[0] for s in capi.SYMBOLS]
    for name in ("ArapFlow_LabelScore", "ArapFlow_MapScore", "ArapFlow_MapScoreScratchBytes"):
        assert name in names and getattr(lib, name) is not None
    header = open(osp.join(ROOT, "include", "arap_opt.h")).read()
    assert "#define ARAPFLOW_LSCORE_FIELDS 8" in header and "#define ARAPFLOW_MSCORE_MAX_THR 8" in header
    assert "int ArapFlow_LabelScore(Opt_State* state, unsigned W, unsigned H, unsigned n, unsigned L, unsigned radius," in header
    assert "int ArapFlow_MapScore(Opt_State* state, unsigned W, unsigned H, unsigned n, const void* gt, const void* est," in header
    assert (capi.LSCORE_FIELDS, capi.MSCORE_MAX_THR) == (8, pipeline.MSCORE_MAX_THR) == (len(pipeline.LSCORE_FIELDS) + 1, 8)
    src = open(osp.join(ROOT, "arap_flow_amd", "opt.py")).read()
    assert "LSCORE_TABLE_FIELDS as LSCORE_FIELDS," in src                                   # opt's name is scores.py's table row
    assert scores.LSCORE_TABLE_FIELDS == ("gt", "est", "inter", "gt_b", "est_b", "gt_hit", "est_hit", "zero")
    # the scratch: 7 bytes a pixel in five parts of 256-byte steps, whatever n; 0 for sizes the calls refuse
    up = lambda v: (v + 255) // 256 * 256
    for W, H in ((5, 3), (854, 480), (256, 1), (257, 1)):
        assert lib.ArapFlow_MapScoreScratchBytes(W, H) == 3 * up(W * H) + 2 * up(2 * W * H)
    assert lib.ArapFlow_MapScoreScratchBytes(0, 4) == lib.ArapFlow_MapScoreScratchBytes(4, 0) == 0
    assert lib.ArapFlow_MapScoreScratchBytes(1 << 16, 1 << 15) == 0 and lib.ArapFlow_MapScoreScratchBytes(46340, 46340) > 0
    # refused before anything is read or launched: a stand-in for the state and the buffers is never dereferenced
    mem = C.create_string_buffer(16384)
    p = C.c_void_p(C.addressof(mem))
    at = lambda off: C.c_void_p(C.addressof(mem) + off)
    GT, EST, SKIP, OUT, MATCH, SCR = at(0), at(256), at(512), at(1024), at(1024 + 4096), at(8192)      # 4 x 4 maps, L <= 3, m <= 8
    assert lib.ArapFlow_MapScoreScratchBytes(4, 4) == 1280

    def label(state=p, W=4, H=4, n=1, L=3, radius=8, gt=GT, est=EST, skip=SKIP, table=OUT, scratch=SCR):
        return lib.ArapFlow_LabelScore(state, W, H, n, L, radius, gt, est, skip, table, scratch)

    def maps(state=p, W=4, H=4, n=1, gt=GT, est=EST, skip=SKIP, thr=(64, 128), radius=8, hist=OUT, match=MATCH, scratch=SCR, m=None):
        arr = (C.c_uint * len(thr))(*thr) if thr is not None and len(thr) else None
        return lib.ArapFlow_MapScore(state, W, H, n, gt, est, skip, len(thr or ()) if m is None else m, arr, radius, hist, match, scratch)

    for call in (label, maps):
        assert call(state=None) == -1 and call(gt=None) == -1 and call(est=None) == -1                  # a null state, gt, est
        assert call(n=0) == -1 and call(W=0) == -1 and call(H=0) == -1                                  # zero sizes
        assert call(W=1 << 16, H=1 << 15) == -1 and call(W=1 << 15, H=1 << 15, n=2) == -1               # (n) W H = 2^31
        assert call(W=0xffffffff, H=0xffffffff, n=0xffffffff) == -1
        assert call(radius=255) == -1 and call(radius=0xffffffff) == -1
        assert call(scratch=at(512 + 8)) == -1 and call(scratch=at(1024 + 64)) == -1                    # the scratch on skip, on the output
        assert call(gt=at(8192 + 1279)) == -1                                                           # by one byte
    assert label(table=None) == -1 and label(scratch=None) == -1 and label(L=0) == -1 and label(L=256) == -1
    assert label(table=at(256 + 8)) == -1 and label(table=at(1024), skip=at(1024 + 255)) == -1 and label(L=255, table=at(16)) == -1
    assert maps(hist=None) == -1 and maps(m=9, thr=(1,) * 9) == -1 and maps(thr=(64, 0)) == -1 and maps(thr=(256,)) == -1
    assert maps(thr=None, m=1) == -1 and maps(match=None) == -1 and maps(scratch=None) == -1            # m > 0 without them
    assert maps(hist=at(8)) == -1 and maps(match=at(1024 + 4096 - 8)) == -1 and maps(match=at(8192 - 8)) == -1
    assert maps(hist=at(8192 + 1280 - 8)) == -1
    assert not any(mem.raw)


# ---- map_score_gen.py with a stand-in worker ---------------------------------------------------------------------------------
FAKE_WORKER = r'''
import sys
# stand-in for arap_deform --serve (no GPU): the file of an lscore / mscore line comes from the numpy twin
sys.path.insert(0, %r); sys.path.insert(0, %r)
import mscore_ref
from arap_flow_amd import pipeline
def run(line):
    it = pipeline.parse_line(line)
    gt, est = pipeline.load_mask_red(it.gt), pipeline.load_mask_red(it.est)
    skip = pipeline.load_mask_red(it.skip) if it.skip else None
    if isinstance(it, pipeline.LScoreLine):
        text = mscore_ref.label_text(gt, est, it.L, it.radius, skip)
    else:
        text = mscore_ref.map_text(gt, est, skip, it.thr, it.radius or 0)
    open(it.out, "w").write(text)
    with open(%r, "a") as log:
        log.write(line)
print("Ready", flush=True)
for line in sys.stdin:
    run(line)
    print("Done " + pipeline.done_token(pipeline.parse_line(line)), flush=True)
'''
MAP_DIRS = ("Occ", "OccBwd", "OccFull", "OccBwdFull", "MB", "MBBwd", "Index1", "Index2")


def _tree(tmp_path):
    """OUT with two pairs of sequence `a` (a fold map for the first) and one of `b`; estimates for a/00000 and b/00000 only,
    the index maps' exact, the others' noisy"""
    from PIL import Image
    rng = np.random.default_rng(11)
    out, est = tmp_path / "out", tmp_path / "est"
    H, W = 6, 9
    for seq, stem in (("a", "00000"), ("a", "00001"), ("b", "00000")):
        idx1 = np.zeros((H, W), U8)
        idx1[1:4, 1:4] = 1
        if seq == "a":
            idx1[3:5, 5:8] = 2
        maps = dict(Index1=idx1, Index2=np.roll(idx1, 1, axis=1))
        for d in MAP_DIRS[:6]:
            maps[d] = (rng.random((H, W)) < 0.3).astype(U8) * 255
        for d, m in maps.items():
            (out / d / seq).mkdir(parents=True, exist_ok=True)
            Image.fromarray(m, "L").save(out / d / seq / (stem + ".png"))
            if stem == "00000":
                (est / d / seq).mkdir(parents=True, exist_ok=True)
                e = m if d.startswith("Index") else np.where(m != 0, rng.integers(100, 256, m.shape), rng.integers(0, 140, m.shape)).astype(U8)
                Image.fromarray(e, "L").save(est / d / seq / (stem + ".png"))
        if (seq, stem) == ("a", "00000"):
            (out / "Fold" / seq).mkdir(parents=True)
            Image.fromarray((rng.random((H, W)) < 0.2).astype(U8) * 255, "L").save(out / "Fold" / seq / (stem + ".png"))
    return out, est


def _gen(tmp_path, args):
    sys.path.insert(0, ROOT)
    import map_score_gen
    fake, log = tmp_path / "fake.py", tmp_path / "lines.log"
    fake.write_text(FAKE_WORKER % (ROOT, osp.join(ROOT, "tests"), str(log)))
    own = "%s %s" % (sys.executable, osp.join(ROOT, "arap_deform.py"))
    flags = map_score_gen.parse(args + ["--arap_bin", own, "--worker", "serve"])
    flags.arap_bin = "%s %s" % (sys.executable, fake)               # (the flags are checked against this repository's driver)
    pooled = map_score_gen.main(flags)
    return pooled, sorted((pipeline.parse_line(ln) for ln in log.read_text().splitlines()), key=lambda it: it.out)


@pytest.mark.parametrize("full", [False, True], ids=["objects", "full"])
def test_map_score_gen_with_a_stand_in_worker(tmp_path, full, capsys):
    out, est = _tree(tmp_path)
    pooled, lines = _gen(tmp_path, ["--data", str(out), "--est", str(est)] + (["--full"] if full else []))
    occ = ("OccFull", "OccBwdFull") if full else ("Occ", "OccBwd")
    dirs = sorted(occ + MAP_DIRS[4:])
    assert [osp.relpath(it.out, out / "MapScore") for it in lines] == [osp.join(d, s, "00000.txt") for d in dirs for s in "ab"]
    assert list(pooled) == list(occ + MAP_DIRS[4:])
    by = {osp.relpath(it.out, out / "MapScore"): it for it in lines}
    for d in dirs:
        a, b = by[osp.join(d, "a", "00000.txt")], by[osp.join(d, "b", "00000.txt")]
        assert a.gt == str(out / d / "a" / "00000.png") and a.est == str(est / d / "a" / "00000.png")
        first = d in ("Occ", "OccFull", "MB", "Index1")
        assert a.skip == (str(out / "Fold" / "a" / "00000.png") if first else None) and b.skip is None     # b has no fold map
        if d.startswith("Index"):
            assert (a.L, a.radius, b.L, b.radius) == (2, 1, 1, 1)            # the largest label; ceil(0.008 * sqrt(117))
        else:
            assert (a.thr, a.radius) == (((64, 128, 192), 1) if d.startswith("MB") else ((), None))
    gt_missing = [str(out / d / "a" / "00001.png") for d in occ + MAP_DIRS[4:]]
    assert (out / "map_score_missing.list").read_text().splitlines() == gt_missing
    text = (out / "map_score.txt").read_text()
    assert text.startswith("[%s]\nneg " % occ[0]) and "[Index2]\nframe counted=108 skipped=0 equal=108 " in text
    assert pooled["Index2"].shape == (3, 8) and pooled["Index2"][1, 0] == 18 and pooled["Index2"][2, 0] == 6      # L = 2 and L = 1 pooled
    s = pipeline.label_score_summary(pooled["Index1"])
    assert s["J"] == s["F"] == 1.0 and int(pooled["Index1"][0, 1]) > 0                                           # exact; some pixels folded
    m = pipeline.map_score_summary(pooled["MB"])
    assert sorted(m["match"]) == [64, 128, 192] and 0 < m["ap"] <= 1 and m["match"][192]["P"] == 1.0
    printed = capsys.readouterr().out
    assert "12 maps scored, 6 without an estimate" in printed and "J&F 1.000000 pooled" in printed and "thr 128" in printed


def test_map_score_gen_ceiling_floor_and_flags(tmp_path, capsys):
    out, est = _tree(tmp_path)
    pooled, lines = _gen(tmp_path, ["--data", str(out), "--est", str(out), "--radius", "3", "--thr", "200"])      # the ceiling
    assert len(lines) == 18 and (out / "map_score_missing.list").read_text() == ""
    assert all(it.radius == 3 for it in lines if isinstance(it, pipeline.LScoreLine) or it.thr) and by_thr(lines) == {(), (200,)}
    for d, p in pooled.items():
        s = pipeline.label_score_summary(p) if d.startswith("Index") else pipeline.map_score_summary(p)
        assert (s["J"], s["F"]) == (1.0, 1.0) if d.startswith("Index") else (s["ap"], s["best_f"]) == (1.0, 1.0)
    (tmp_path / "lines.log").unlink()
    pooled, lines = _gen(tmp_path, ["--data", str(out), "--baseline", "still"])                                   # the floor
    assert list(pooled) == ["Index2"] and len(lines) == 3
    assert all(it.gt == it.est.replace("Index1", "Index2") and "Index1" in it.est and it.skip is None for it in lines)
    s = pipeline.label_score_summary(pooled["Index2"])
    assert 0 < s["J"] < 1 and s["labels"][1]["J"] == 2 / 4                                                        # moved by one of three columns
    import map_score_gen
    assert map_score_gen.davis_radius(854, 480) == 8 and map_score_gen.davis_radius(9, 6) == 1
    for bad in (["--data", "x"], ["--data", "x", "--est", "y", "--baseline", "still"], ["--data", "x", "--est", "y", "--thr", "0"],
                ["--data", "x", "--est", "y", "--thr", "1,2,3,4,5,6,7,8,9"], ["--data", "x", "--est", "y", "--radius", "255"],
                ["--data", "x", "--est", "y", "--arap_bin", "/bin/true"]):
        with pytest.raises(SystemExit):
            map_score_gen.parse(bad)
    capsys.readouterr()


def by_thr(lines):
    return {it.thr for it in lines if isinstance(it, pipeline.MScoreLine)}
