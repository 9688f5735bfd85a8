"""CPU-only: track scoring and flow chaining (DESIGN.md "Track scoring") without a device -- the numpy twin
tests/tscore_ref.py against a hand-computed table, its identities, the pooling of tables, the summary against the
formulas, the score file format, both list lines through both grammars, the library's refusals before any device call,
track_score_gen.py with a stand-in worker."""
import ctypes as C
import os
import os.path as osp
import subprocess
import sys

import numpy as np
import pytest

import tscore_ref as R
from arap_flow_amd import capi, flo, opt, pipeline, trk

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
F = np.float32
CAP = 1 << 24


# ---- the twin -----------------------------------------------------------------------------------------------------------------
def six_points():
    """six points, four frames, the ground truth at the origin, the estimate a fixed offset away:
         k   offset    e2    q        gt_occ           est_occ
         0   (.5, 0)   .25   2048     0 0 0 0          0 0 0 0        tracked throughout
         1   (3, 4)    25    20480    0 255 0 0        0 0 0 255      hidden in frame 1: reappeared in 2 and 3
         2   (1, 0)    1     4096     0 0 0 0          0 255 0 0      exactly on the 1 px threshold: not within it
         3   (0, 0)                   255 0 0 0        0 0 0 0        an invalid query
         4   (nan, 0)  nan   2^24     0 0 255 0        0 0 0 0        tracked in 1, hidden in 2, reappeared in 3
         5   (20, 0)   400   81920    0 0 0 0          0 0 0 0        beyond every threshold"""
    off = np.array([[0.5, 0], [3, 4], [1, 0], [0, 0], [np.nan, 0], [20, 0]], F)
    gt_occ = np.array([[0, 0, 0, 0], [0, 255, 0, 0], [0, 0, 0, 0], [255, 0, 0, 0], [0, 0, 255, 0], [0, 0, 0, 0]], np.uint8).T.copy()
    est_occ = np.array([[0, 0, 0, 0], [0, 0, 0, 255], [0, 255, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]], np.uint8).T.copy()
    gt_pos = np.zeros((4, 6, 2), F)
    return gt_pos, gt_occ, gt_pos + off[None], est_occ


def test_twin_equals_a_hand_computed_table():
    t = R.track_score_ref(*six_points())
    assert t.shape == (4, 3, 16) and t.dtype == np.uint64
    row = lambda f, c: [int(v) for v in t[f, c]]
    zero = [0] * 16
    #                    count gt est agree  within_1..16      tp_1..16          sum               max
    assert row(0, 0) == [5, 1] + [0] * 14 and row(0, 1) == zero and row(0, 2) == zero
    s1 = 2048 + 4096 + CAP + 81920
    assert row(1, 0) == [5, 4, 4, 3, 1, 2, 2, 2, 2, 1, 1, 1, 1, 1, s1, CAP]
    assert row(1, 1) == [4, 4, 3, 3, 1, 2, 2, 2, 2, 1, 1, 1, 1, 1, s1, CAP] and row(1, 2) == zero
    assert row(2, 0) == [5, 4, 5, 4, 1, 2, 2, 3, 3, 1, 2, 2, 3, 3, 2048 + 20480 + 4096 + 81920, 81920]
    assert row(2, 1) == [3, 3, 3, 3, 1, 2, 2, 2, 2, 1, 2, 2, 2, 2, 2048 + 4096 + 81920, 81920]
    assert row(2, 2) == [1, 1, 1, 1, 0, 0, 0, 1, 1, 0, 0, 0, 1, 1, 20480, 20480]
    assert row(3, 0) == [5, 5, 4, 4, 1, 2, 2, 3, 3, 1, 2, 2, 2, 2, 2048 + 20480 + 4096 + CAP + 81920, CAP]
    assert row(3, 1) == [3, 3, 3, 3, 1, 2, 2, 2, 2, 1, 2, 2, 2, 2, 2048 + 4096 + 81920, 81920]
    assert row(3, 2) == [2, 2, 1, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 20480 + CAP, CAP]


def test_an_estimate_equal_to_the_ground_truth():
    gt_pos, gt_occ, _, _ = R.random_case(6, 300, 4)
    t = R.track_score_ref(gt_pos, gt_occ, gt_pos, gt_occ)
    assert (t[1:, :, R.AGREE] == t[1:, :, R.COUNT]).all() and (t[1:, :, R.SUM] == 0).all() and (t[1:, :, R.MAX] == 0).all()
    assert (t[1:, :, R.WITHIN] == t[1:, :, R.GT_VIS]).all() and (t[1:, :, R.TP] == t[1:, :, R.GT_VIS]).all()
    assert t[1:, 0, R.GT_VIS].min() > 0 and t[2:, 2, R.COUNT].min() > 0


def test_crafted_case_reaches_every_field_and_sits_on_every_threshold():
    for scale in ((1, 1), R.TAPVID_854x480):
        gt_pos, gt_occ, est_pos, est_occ = R.crafted_case(scale)
        t = R.track_score_ref(gt_pos, gt_occ, est_pos, est_occ, scale)
        assert (t[1:].sum(axis=0) > 0).all() and (t[0, 0, :2] > 0).all() and not t[0].ravel()[2:].any()
        e2, q = R.point_terms(gt_pos, est_pos, scale)
        for x in R.X:
            assert (e2[1:] == F(x * x)).any() and (e2[1:] == R.ulp(F(x * x), -1)).any()
            on, below = R.threshold_offsets(x, scale)
            one = lambda d: R.track_score_ref(np.zeros((2, 1, 2), F), np.zeros((2, 1), np.uint8), np.stack([d, d])[:, None],
                                              np.zeros((2, 1), np.uint8), scale)[1, 0]
            k = R.X.index(x)
            assert one(on)[R.WITHIN + k] == 0 and one(below)[R.WITHIN + k] == 1        # strict <
            assert one(on)[R.SUM] == x * 4096
        assert np.isnan(e2).any() and np.isinf(e2).any() and (q == CAP).any()
    assert not float(R.TAPVID_854x480[0] * F(2.0 ** 20)).is_integer()                 # the second scale is not dyadic


def test_pooling_is_exact():
    """the points split in two, and tables of different F: the pooled table is the table of all the points together"""
    c = R.random_case(7, 500, 2)
    whole = R.track_score_ref(*c)
    a, b = R.track_score_ref(*[x[:, :123] for x in c]), R.track_score_ref(*[x[:, 123:] for x in c])
    assert np.array_equal(pipeline.add_track_scores([a, b]), whole)
    assert np.array_equal(pipeline.add_track_scores([b, a, np.zeros((3, 3, 16), np.uint64)]), whole)
    short = R.track_score_ref(*[x[:4, 123:] for x in c])          # the second half seen for four frames only
    pooled = pipeline.add_track_scores([a, short])
    assert pooled.shape == whole.shape and np.array_equal(pooled[4:], a[4:])
    assert np.array_equal(pooled[:4], pipeline.add_track_scores([a[:4], short]))
    assert np.array_equal(pooled[:4, :, :R.MAX], whole[:4, :, :R.MAX])
    assert np.array_equal(pipeline.add_track_scores([a]), a)


def test_summary_equals_the_formulas():
    t = R.track_score_ref(*six_points())
    s = pipeline.track_score_summary(t)
    assert (s["valid"], s["invalid"]) == (5, 1) and len(s["frames"]) == 3
    f2 = s["frames"][1]                                         # frame 2, class all: the hand-computed row above
    assert f2["count"] == 5 and f2["gt_vis"] == 4 and f2["oa"] == 4 / 5
    assert [f2["d_%d" % x] for x in R.X] == [1 / 4, 2 / 4, 2 / 4, 3 / 4, 3 / 4]
    assert [f2["j_%d" % x] for x in R.X] == [1 / 8, 2 / 7, 2 / 7, 3 / 6, 3 / 6]         # tp / (gt_vis + est_vis - tp)
    assert f2["d_avg"] == sum([1 / 4, 2 / 4, 2 / 4, 3 / 4, 3 / 4]) / 5 and f2["aj"] == sum([1 / 8, 2 / 7, 2 / 7, 3 / 6, 3 / 6]) / 5
    assert f2["err"] == (2048 + 20480 + 4096 + 81920) / 4096 / 4
    re = s["reappeared"]                                        # frames 2 and 3 together: counts 3, gt_vis 3, est_vis 2, agree 2
    assert re["count"] == 3 and re["oa"] == 2 / 3 and re["d_8"] == 2 / 3 and re["j_8"] == 1 / 4 and re["d_1"] == 0
    assert re["err"] == (20480 + 20480 + CAP) / 4096 / 3
    empty = pipeline.track_score_summary(np.zeros((2, 3, 16), np.uint64))
    assert all(np.isnan(empty["all"][k]) for k in ("oa", "d_avg", "aj", "err")) and empty["all"]["count"] == 0


def test_score_file_round_trip():
    t = R.track_score_ref(*R.random_case(5, 200, 3))
    t[2, 1, R.SUM] = (1 << 64) - 1
    text = pipeline.format_track_score(t)
    lines = text.split("\n")
    assert len(lines) == 5 * 3 + 1 and lines[0].startswith("0 all count=") and lines[4].startswith("1 tracked count=")
    assert lines[-2].startswith("4 reappeared ") and lines[-1] == ""
    assert all(set(ln) <= set("0123456789abcdefghijklmnopqrstuvwxyz_= ") for ln in lines)
    assert np.array_equal(pipeline.parse_track_score_file(text), t)
    for bad in (text[:-1], text + "\n", text.replace("0 all", "1 all", 1), text.replace("gt_vis=", "gtvis=", 1),
                text.replace("count=", "count=-", 1), "\n".join(lines[:5]) + "\n", "\n".join(lines[:3]) + "\n",
                text.replace("max=", "max=18446744073709551616 x=", 1)):
        with pytest.raises(ValueError):
            pipeline.parse_track_score_file(bad)


def test_chain_twin_on_closed_forms():
    W, H = 9, 6
    const = lambda v, L=1: np.broadcast_to(np.array(v, F), (L, H, W, 2)).copy()
    pts = np.array([[0, 0], [2.5, 1.25], [8, 5], [7.5, 0], [np.nan, 1], [8.25, 1]], F)
    pos, occ = R.chain_ref(const([0.5, 0.25], 3), pts)
    assert np.array_equal(pos[3][:2], pts[:2] + F([1.5, 0.75])) and list(occ[:, 0]) == [0, 0, 0, 0]
    assert list(occ[:, 2]) == [0, 255, 255, 255] and np.array_equal(pos[1:, 2], np.broadcast_to(F([8.5, 5.25]), (3, 2)))      # left, stays
    assert list(occ[:, 3]) == [0, 0, 255, 255] and list(occ[:, 4]) == [255] * 4 and list(occ[:, 5]) == [255] * 4
    assert np.array_equal(pos[:, 5], np.broadcast_to(pts[5], (4, 2)))
    ramp = np.zeros((1, H, W, 2), F)                            # u = x / 4: bilinear sampling of a linear field is exact
    ramp[0, ..., 0] = np.arange(W, dtype=F) / 4
    pos, occ = R.chain_ref(ramp, np.array([[2.5, 1.5], [4, 2]], F))
    assert np.array_equal(pos[1], F([[2.5 + 0.625, 1.5], [5, 2]]))
    _, occ = R.chain_ref(const([1, 0]), pts[:2], bwd=const([-1, 0]))
    assert not occ.any()
    _, occ = R.chain_ref(const([1, 0]), pts[:2], bwd=const([1, 1]))
    assert list(occ[1]) == [255, 255] and not occ[0].any()


# ---- both list lines through both grammars -------------------------------------------------------------------------------------
_S = "s=%.9g,%.9g" % tuple(float(v) for v in R.TAPVID_854x480)                              # s=0.299765795,0.533333361
_L63 = " ".join("f%d" % j for j in range(63))
LINE_CORPUS = [
    # accepted
    "tscore GT.trk EST.trk out=T.txt", "tscore GT.trk EST.trk " + _S + " out=T.txt", "tscore GT.trk EST.trk out=T.txt " + _S,
    "tscore G E s=1,1 out=T", "tscore G E s=1e-3,2.5e2 out=T", "tscore G E s=0.1,3 out=T",
    "chain P.trk 1 F1.flo out=O.trk", "chain P.trk 3 F1 F2 F3 bwd=B1,B2,B3 out=O.trk", "chain P.trk 2 F1 F2 out=O.trk bwd=B1,B2",
    "chain P.trk 63 " + _L63 + " out=O",
    # refused
    "tscore", "tscore GT.trk", "tscore GT.trk EST.trk", "tscore GT.trk out=T.txt", "tscore GT.trk EST.trk out=", "tscore GT.trk EST.trk out=A out=B",
    "tscore a=b EST.trk out=T", "tscore GT.trk EST.trk " + _S + " " + _S + " out=T", "tscore G E s=1 out=T", "tscore G E s=1,2,3 out=T",
    "tscore G E s=0,1 out=T", "tscore G E s=1,-2 out=T", "tscore G E s=nan,1 out=T", "tscore G E s=1,inf out=T", "tscore G E s=1,x out=T",
    "tscore G E s=,1 out=T", "tscore G E s= out=T", "tscore G E junk out=T", "tscore G E occ=O out=T", "tscore G E X out=T",
    "chain", "chain P.trk", "chain P.trk 1", "chain P.trk 1 F1", "chain P.trk 0 out=O", "chain P.trk 64 " + _L63 + " f63 out=O",
    "chain P.trk x F1 out=O", "chain P.trk 2 F1 out=O", "chain P.trk 1 F1 F2 out=O", "chain P.trk 2 F1 F2 bwd=B1 out=O",
    "chain P.trk 2 F1 F2 bwd=B1,B2,B3 out=O", "chain P.trk 2 F1 F2 bwd=B1, out=O", "chain P.trk 2 F1 F2 bwd=,B2 out=O",
    "chain P.trk 1 F1 bwd=B1 bwd=B1 out=O", "chain P.trk 1 F1 out=O out=P", "chain P.trk 1 F1 out=", "chain P.trk 1 F1 bwd= out=O",
    "chain p=q 1 F1 out=O", "chain P.trk 1 a=b out=O", "chain P.trk 1 F1 junk out=O", "chain P.trk 1 F1 s=1,1 out=O", "chain P.trk -1 F1 out=O",
]
ACCEPTED = 10


@pytest.fixture(scope="module")
def bins():
    from arap_flow_amd import build
    return {osp.basename(o): o for o in build.build_host()}


def test_both_lines_round_trip_in_python():
    for line in LINE_CORPUS[:ACCEPTED]:
        item = pipeline.parse_line(line)
        assert isinstance(item, (pipeline.TScoreLine, pipeline.ChainLine))
        again = pipeline.parse_line(pipeline.format_line(item))
        assert again == item and pipeline.done_token(item) == item.out
    assert pipeline.format_line(pipeline.parse_line(LINE_CORPUS[2])) == LINE_CORPUS[1]          # s= before out=
    assert pipeline.format_line(pipeline.parse_line(LINE_CORPUS[3])) == "tscore G E out=T"       # (1, 1) is the default
    assert pipeline.format_line(pipeline.parse_line(LINE_CORPUS[8])) == "chain P.trk 2 F1 F2 bwd=B1,B2 out=O.trk"
    it = pipeline.parse_line(LINE_CORPUS[1])
    assert it.scale == tuple(float(v) for v in R.TAPVID_854x480)                                 # %.9g carries a float32 exactly
    it = pipeline.parse_line(LINE_CORPUS[7])
    assert it.flows == ("F1", "F2", "F3") and it.bwd == ("B1", "B2", "B3") and it.points == "P.trk"
    for line in LINE_CORPUS[ACCEPTED:]:
        with pytest.raises(ValueError):
            pipeline.parse_line(line)


def test_list_line_parser_equals_python_twin(bins):
    r = subprocess.run([bins["line_tool"]], input="".join(c + "\n" for c in LINE_CORPUS), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = r.stdout.split("\n")[:-1]
    got = [ln for ln in out if not ln.startswith("Invalid")]
    assert len(got) == len(LINE_CORPUS)
    accepted = 0
    for line, g in zip(LINE_CORPUS, got):
        try:
            item = pipeline.parse_line(line)
        except ValueError:
            assert g == "BAD", (line, g)
            assert "Invalid %s line: %s" % (line.split()[0], line) in out
            continue
        assert g == pipeline.format_line(item) + " done=" + pipeline.done_token(item), line
        accepted += 1
    assert accepted == ACCEPTED


def test_arap_deform_refuses_bad_lines_before_any_gpu_call(bins, tmp_path):
    lst = tmp_path / "l.txt"
    for bad in ("tscore G E s=0,1 out=T", "chain P.trk 2 F1 F2 bwd=B1 out=O"):
        lst.write_text("a b c d e f\n" + bad + "\n")
        r = subprocess.run([bins["arap_deform"], str(lst)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and r.stdout == "Invalid %s line: %s\n" % (bad.split()[0], bad), (r.stdout, r.stderr)
        r = subprocess.run([sys.executable, osp.join(ROOT, "arap_deform.py"), str(lst)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and bad.split()[0] + " line" in r.stdout


# ---- the library's new entry points ----------------------------------------------------------------------------------------------
def test_new_entry_points_exported_and_refusals_without_a_device():
    lib = capi.load()
    names = [s[0] for s in capi.SYMBOLS]
    for name in ("ArapFlow_TrackScore", "ArapFlow_ChainFlows"):
        assert name in names and hasattr(lib, name)
    header = open(osp.join(ROOT, "include", "arap_opt.h")).read()
    for text in ("#define ARAPFLOW_TSCORE_MAX_FRAMES 64", "#define ARAPFLOW_TSCORE_CLASSES 3", "#define ARAPFLOW_TSCORE_FIELDS 16",
                 "int ArapFlow_TrackScore(Opt_State* state, unsigned F, unsigned P, const void* gt_pos, const void* gt_occ,",
                 "int ArapFlow_ChainFlows(Opt_State* state, unsigned W, unsigned H, unsigned L, const void* flows, const void* bwd,"):
        assert text in header
    assert (capi.TSCORE_MAX_FRAMES, capi.TSCORE_CLASSES, capi.TSCORE_FIELDS) == (64, 3, 16) == \
        (pipeline.TSCORE_MAX_FRAMES, len(pipeline.TSCORE_CLASSES), len(pipeline.TSCORE_FIELDS))
    assert opt.TSCORE_CLASSES == pipeline.TSCORE_CLASSES == ("all", "tracked", "reappeared")
    assert opt.TSCORE_FIELDS == pipeline.TSCORE_FIELDS and opt.TSCORE_FIELDS[R.WITHIN] == "within_1" and opt.TSCORE_FIELDS[R.TP] == "tp_1"
    assert opt.TSCORE_FIELDS[R.SUM] == "sum" and opt.TSCORE_FIELDS[R.MAX] == "max"
    # refused before anything is read or launched: a stand-in for the state and the buffers is never dereferenced
    mem = C.create_string_buffer(1 << 16)
    p = C.c_void_p(C.addressof(mem))
    at = lambda off: C.c_void_p(C.addressof(mem) + off)
    ts = lambda state, nf, P, gp, go, ep, eo, sx, sy, table: lib.ArapFlow_TrackScore(state, nf, P, gp, go, ep, eo, sx, sy, table)
    ok = (p, 4, 16, at(0), at(1024), at(2048), at(3072), 1.0, 1.0, at(8192))
    for k in (0, 3, 4, 5, 6, 9):                                # a null state, buffer or table
        a = list(ok)
        a[k] = None
        assert ts(*a) == -1
    for k, v in ((1, 0), (1, 1), (1, 65), (2, 0), (2, (1 << 24) + 1), (7, 0.0), (7, -1.0), (7, float("nan")), (7, float("inf")),
                 (8, 0.0), (8, float("-inf")), (8, float("nan")), (9, at(64)), (9, at(1024 + 8)), (9, at(2048 + 4 * 16 * 8 - 8)), (9, at(3072))):
        a = list(ok)
        a[k] = v
        assert ts(*a) == -1, (k, v)
    cf = lambda state, W, H, L, f, b, P, q, op, oo: lib.ArapFlow_ChainFlows(state, W, H, L, f, b, P, q, op, oo)
    ok = (p, 4, 4, 2, at(0), at(1024), 8, at(2048), at(4096), at(8192))
    for k in (0, 4, 7, 8, 9):
        a = list(ok)
        a[k] = None
        assert cf(*a) == -1
    for k, v in ((1, 0), (2, 0), (3, 0), (3, 64), (6, 0), (6, (1 << 24) + 1), (8, at(128)), (8, at(1024 + 8)), (8, at(2048 + 56)),
                 (9, at(255)), (9, at(1024)), (9, at(2048)), (9, at(4096 + 3 * 8 * 8 - 1)), (8, at(8192 - 8))):
        a = list(ok)
        a[k] = v
        assert cf(*a) == -1, (k, v)
    assert cf(p, 1 << 16, 1 << 15, 2, at(0), None, 8, at(2048), at(4096), at(8192)) == -1               # W * H = 2^31


# ---- track_score_gen.py -------------------------------------------------------------------------------------------------------------
FAKE_WORKER = r'''
import sys
# stand-in for arap_deform --serve (no GPU): a tscore line's table and a chain line's tracks come from the numpy twins
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import tscore_ref
from arap_flow_amd import flo, pipeline, trk
def run(line):
    it = pipeline.parse_line(line)
    if isinstance(it, pipeline.ChainLine):
        pts = trk.read(it.points)
        bwd = np.stack([flo.flow_read(p) for p in it.bwd]) if it.bwd else None
        pos, occ = tscore_ref.chain_ref(np.stack([flo.flow_read(p) for p in it.flows]), pts["pos"][0], bwd)
        trk.write(it.out, pts["W"], pts["H"], pos, occ)
    else:
        gt, est = trk.read(it.gt), trk.read(it.est)
        t = tscore_ref.track_score_ref(gt["pos"], gt["occ"], est["pos"], est["occ"], it.scale)
        open(it.out, "w").write(pipeline.format_track_score(t))
    with open(%r, "a") as log:
        log.write(line)
print("Ready", flush=True)
for line in sys.stdin:
    run(line)
    print("Done " + pipeline.done_token(pipeline.parse_line(line)), flush=True)
'''


def make_tree(tmp_path):
    """OUT/Tracks with a/00000 (4 frames), a/00001 (3 frames) and b/00000 (3 frames); estimates, as track files and as
    link flows (backward ones for a/00000 only), for a/00000 and b/00000.  -> (out, est, {(seq, stem): ground truth})"""
    rng = np.random.default_rng(5)
    out, est = tmp_path / "out", tmp_path / "est"
    W, H, P = 12, 9, 40
    gts = {}
    for seq, stem, nf in (("a", "00000", 4), ("a", "00001", 3), ("b", "00000", 3)):
        os.makedirs(out / "Tracks" / seq, exist_ok=True)
        pos = (rng.uniform(0, 1, (nf, P, 2)) * [W - 1, H - 1]).astype(F)
        occ = np.where(rng.random((nf, P)) < 0.25, 255, 0).astype(np.uint8)
        trk.write(str(out / "Tracks" / seq / (stem + ".trk")), W, H, pos, occ)
        gts[(seq, stem)] = dict(W=W, H=H, pos=pos, occ=occ)
        if stem == "00000":
            os.makedirs(est / seq, exist_ok=True)
            e_pos = (pos + rng.normal(size=pos.shape) * 2).astype(F)
            e_occ = np.where(rng.random((nf, P)) < 0.25, 255, 0).astype(np.uint8)
            trk.write(str(est / seq / (stem + ".trk")), W, H, e_pos, e_occ)
            for j in range(nf - 1):
                fl = (np.round(rng.normal(size=(H, W, 2)) * 32) / 32).astype(F)
                flo.flow_write(str(est / seq / ("%s_l%d.flo" % (stem, j))), fl)
                if seq == "a":
                    flo.flow_write(str(est / seq / ("%s_b%d.flo" % (stem, j))), (-fl + F(0.125)).astype(F))
    return out, est, gts


@pytest.mark.parametrize("from_flows", [False, True], ids=["tracks", "from_flows"])
def test_track_score_gen_with_a_stand_in_worker(tmp_path, from_flows, capsys):
    sys.path.insert(0, ROOT)
    import track_score_gen
    out, est, gts = make_tree(tmp_path)
    fake, log = tmp_path / "fake.py", tmp_path / "lines.log"
    fake.write_text(FAKE_WORKER % (ROOT, osp.join(ROOT, "tests"), str(log)))
    own = "%s %s" % (sys.executable, osp.join(ROOT, "arap_deform.py"))
    flags = track_score_gen.parse(["--data", str(out), "--est", str(est), "--arap_bin", own, "--worker", "serve", "--tapvid"] +
                                  (["--from_flows"] if from_flows else []))
    flags.arap_bin = "%s %s" % (sys.executable, fake)               # (the flags are checked against this repository's driver)
    pooled = track_score_gen.main(flags)
    lines = [pipeline.parse_line(ln) for ln in log.read_text().splitlines()]
    scale = (float(F(256) / F(12)), float(F(256) / F(9)))
    tables = []
    for seq in "ab":
        g = gts[(seq, "00000")]
        if from_flows:
            chain = [it for it in lines if isinstance(it, pipeline.ChainLine) and it.points == str(out / "Tracks" / seq / "00000.trk")]
            assert len(chain) == 1 and len(chain[0].flows) == len(g["pos"]) - 1 and len(chain[0].bwd) == (len(chain[0].flows) if seq == "a" else 0)
            e = trk.read(str(out / "TracksEst" / seq / "00000.trk"))
            bwd = np.stack([flo.flow_read(p) for p in chain[0].bwd]) if chain[0].bwd else None
            pos, occ = R.chain_ref(np.stack([flo.flow_read(p) for p in chain[0].flows]), g["pos"][0], bwd)
            assert np.array_equal(e["pos"], pos) and np.array_equal(e["occ"], occ) and (e["W"], e["H"]) == (12, 9)
        else:
            e = trk.read(str(est / seq / "00000.trk"))
        ref = R.track_score_ref(g["pos"], g["occ"], e["pos"], e["occ"], scale)
        assert (out / "TrackScore" / seq / "00000.txt").read_text() == pipeline.format_track_score(ref)
        tables.append(ref)
    ts = [it for it in lines if isinstance(it, pipeline.TScoreLine)]
    assert len(ts) == 2 and all(it.scale == scale for it in ts) and len(lines) == (4 if from_flows else 2)
    assert pooled.shape == (4, 3, 16) and np.array_equal(pooled, pipeline.add_track_scores(tables))
    assert (out / "track_score.txt").read_text() == pipeline.format_track_score(pooled)
    assert (out / "track_score_missing.list").read_text() == str(out / "Tracks" / "a" / "00001.trk") + "\n"
    printed = capsys.readouterr().out
    assert "2 track files scored, 1 without an estimate" in printed and "reappeared" in printed and "\n3 " in printed


def test_track_score_gen_parse_and_no_estimate(tmp_path, capsys):
    sys.path.insert(0, ROOT)
    import track_score_gen
    out, est, _ = make_tree(tmp_path)
    flags = track_score_gen.parse(["--data", str(out), "--est", str(est)])
    assert (flags.from_flows, flags.tapvid, flags.gpu, flags.worker, flags.narap) == (False, False, [0], "auto", 64)
    flags = track_score_gen.parse(["--data", "D", "--est", "E", "--from_flows", "--tapvid", "--gpu", "2", "3", "--narap", "8", "--worker", "batch"])
    assert (flags.from_flows, flags.tapvid, flags.gpu, flags.worker, flags.narap) == (True, True, [2, 3], "batch", 8)
    with pytest.raises(SystemExit):
        track_score_gen.parse(["--data", str(out), "--est", str(est), "--arap_bin", "/bin/true"])
    with pytest.raises(SystemExit):
        track_score_gen.parse(["--data", str(out)])
    pooled = track_score_gen.main(track_score_gen.parse(["--data", str(out), "--est", str(tmp_path / "nothing")]))      # no worker is started
    assert not pooled.any() and (out / "track_score.txt").read_text() == pipeline.format_track_score(np.zeros((2, 3, 16), np.uint64))
    assert len((out / "track_score_missing.list").read_text().splitlines()) == 3
