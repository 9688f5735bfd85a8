"""CPU: fold diagnostics (DESIGN.md "Fold diagnostics") without a GPU -- the numpy twin of tests/diag_ref.py against
its own sequential statement and against closed forms, the diag file's text, the diag= / fold= tokens through both
line grammars, the --multseg merge, the list-writing step of para_gen.py and its refusals.  Nothing here has a
tolerance: every comparison is of integers, flags or float bits."""
import os
import os.path as osp
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
from PIL import Image

import diag_ref as dr

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
F32 = np.float32
INF = float("inf")


def _bits(v):
    return int(np.float32(v).view(np.uint32))


def _noisy_precondition(stats):
    """a noisy case says something only while some, not all, triangles fold"""
    assert 0 < stats["folded"] < stats["triangles"], stats


# ---- the twin against the sequential statement ---------------------------------------------------------------------------
def _small_cases():
    rng = np.random.default_rng(11)
    for W, H in ((2, 2), (3, 2), (5, 4), (8, 3), (9, 7), (9, 7), (9, 7)):
        mask = np.where(rng.random((H, W)) < 0.15, 255, 0).astype(np.uint8)
        P = dr.grid_field(W, H) + rng.normal(0, 0.6, (H, W, 2)).astype(F32)
        yield "noise %dx%d" % (W, H), mask, P, W * H >= 20
    g = dr.grid_field(9, 7)
    P = g + np.random.default_rng(5).normal(0, 0.5, g.shape).astype(F32)
    for name, (y, x, c), v in (("nan", (3, 4, 0), np.nan), ("inf", (2, 6, 1), np.inf), ("-inf", (5, 1, 0), -np.inf)):
        Q = P.copy()
        Q[y, x, c] = v
        yield name, np.zeros((7, 9), np.uint8), Q, True


@pytest.mark.parametrize("name,mask,P,noisy", list(_small_cases()), ids=lambda v: v if isinstance(v, str) else "")
def test_twin_equals_sequential_statement(name, mask, P, noisy):
    twin = dr.diag(mask, P)
    if noisy:
        _noisy_precondition(twin[0])
    assert dr.same(twin, dr.diag_sequential(mask, P)), (twin[0], dr.diag_sequential(mask, P)[0])
    if name in ("nan", "inf", "-inf"):
        assert twin[0]["nonfinite"] == 6 and twin[0]["vertices"] == 63


def test_collapsed_triangles_give_signed_zeros_in_bit_order():
    """one quad: p01 on p00 collapses triangle 2u; with e2 = (0, 1) its det is +0, with e2 = (1, -1) it is -0, and the
    other triangle is positive.  -0 < +0 in the order of the extrema, both count as folded"""
    mask = np.zeros((2, 2), np.uint8)
    plus = np.array([[[0, 0], [0, 0]], [[0, 1], [1, 1]]], F32)
    minus = np.array([[[0, 0], [0, 0]], [[1, -1], [-1, -1]]], F32)
    for P, zero, top in ((plus, 0x00000000, 1.0), (minus, 0x80000000, 2.0)):
        st, fold = dr.diag(mask, P)
        assert dr.same((st, fold), dr.diag_sequential(mask, P))
        assert (st["triangles"], st["folded"], st["nonfinite"]) == (2, 1, 0)
        assert _bits(st["det_min"]) == zero and st["det_max"] == top
        assert fold.tolist() == [[255, 255], [255, 0]]
    both = np.array([0.0, -0.0, 0.0], F32)
    assert _bits(dr._extreme(both, False, INF)) == 0x80000000 and _bits(dr._extreme(both, True, -INF)) == 0
    assert list(dr.order_key(np.array([-np.inf, -1, -0.0, 0.0, 1, np.inf], F32))) == sorted(
        dr.order_key(np.array([-np.inf, -1, -0.0, 0.0, 1, np.inf], F32)))


# ---- closed forms at 67 x 9, all object ----------------------------------------------------------------------------------
W, H = dr.W0, dr.H0


def test_closed_forms():
    mask, f = dr.masks()["all"], dr.fields()
    st, fold = dr.diag(mask, dr.flow_pos(f["zero"]))
    assert st == dict(vertices=603, outside=0, triangles=1056, folded=0, nonfinite=0, det_min=1, det_max=1, disp2_max=0)
    assert not fold.any()
    st, fold = dr.diag(mask, dr.flow_pos(f["mirror"]))
    assert (st["folded"], st["triangles"], st["det_min"], st["det_max"], st["outside"]) == (1056, 1056, -1, -1, 0)
    assert (fold == 255).all() and st["disp2_max"] == (W - 1) ** 2
    for dx, dy in ((3, -2), (-70, 0), (0, 9), (-1, 1)):
        fl = np.zeros((H, W, 2), F32)
        fl[..., 0], fl[..., 1] = dx, dy
        st, fold = dr.diag(mask, dr.flow_pos(fl))
        assert st["outside"] == dr.translation_outside(W, H, dx, dy) and st["folded"] == 0 and not fold.any()
        assert st["det_min"] == 1 and st["det_max"] == 1 and st["disp2_max"] == dx * dx + dy * dy
    assert dr.translation_outside(W, H, 3, -2) == 603 - 64 * 7


def test_one_nan_vertex_marks_its_six_triangles():
    x, y = 30, 4
    P = dr.grid_field(W, H)
    P[y, x, 1] = np.nan
    st, fold = dr.diag(dr.masks()["all"], P)
    assert (st["nonfinite"], st["folded"], st["outside"], st["det_min"], st["det_max"]) == (6, 0, 1, 1, 1)
    want = np.zeros((H, W), np.uint8)
    for ax, ay in ((x, y), (x + 1, y), (x, y + 1), (x - 1, y), (x - 1, y + 1), (x, y - 1), (x + 1, y - 1)):
        want[ay, ax] = 255
    assert np.array_equal(fold, want)


def test_noisy_fields_fold_some_triangles():
    """the figures the GPU cases rest on, re-derived with the committed twin"""
    m, f = dr.masks(), dr.fields()
    st = dr.diag(m["all"], dr.flow_pos(f["noise_a"]))[0]
    assert (st["folded"], st["triangles"]) == (58, 1056)
    st = dr.diag(m["random"], dr.flow_pos(f["noise_b"]))[0]
    _noisy_precondition(st)
    assert st["triangles"] == 252
    assert dr.diag(m["strip"], dr.flow_pos(f["noise_a"]))[0]["triangles"] == 0
    none = dr.diag(m["none"], dr.flow_pos(f["noise_a"]))
    assert none[0] == dict(vertices=0, outside=0, triangles=0, folded=0, nonfinite=0, det_min=INF, det_max=-INF,
                           disp2_max=0) and not none[1].any()
    for x, y in dr.spikes():
        st, fold = dr.diag(m["all"], dr.flow_pos(f["spike_%d_%d" % (x, y)]))
        assert 0 < st["folded"] <= 3 and st["det_min"] == -1.75 and fold[y, x] == 255 and st["disp2_max"] == 3.8125


# ---- the diag file -------------------------------------------------------------------------------------------------------
def test_format_diag_round_trip():
    from arap_flow_amd import pipeline
    st = dict(vertices=603, outside=3, triangles=1056, folded=58, nonfinite=0, det_min=F32(-1.8179421),
              det_max=F32(4.264151), disp2_max=F32(1.3294791))
    text = pipeline.format_diag(st)
    assert text == ("vertices 603\noutside 3\ntriangles 1056\nfolded 58\nnonfinite 0\ndet_min -1.81794214\n"
                    "det_max 4.2641511\ndisp2_max 1.3294791\n")
    back = pipeline.parse_diag(text)
    assert dr.stats_bytes(back) == dr.stats_bytes(st) and list(back) == list(dr.KEYS)
    none = dict(vertices=7, outside=0, triangles=0, folded=0, nonfinite=0, det_min=F32(INF), det_max=F32(-INF), disp2_max=F32(0))
    text = pipeline.format_diag(none)
    assert text.endswith("det_min inf\ndet_max -inf\ndisp2_max 0\n")
    assert dr.stats_bytes(pipeline.parse_diag(text)) == dr.stats_bytes(none)
    zero = dict(none, det_min=F32(-0.0), det_max=F32(0.0))
    assert "det_min -0\ndet_max 0\n" in pipeline.format_diag(zero)
    assert dr.stats_bytes(pipeline.parse_diag(pipeline.format_diag(zero))) == dr.stats_bytes(zero)
    rng = np.random.default_rng(2)
    for v in rng.normal(0, 30, 50).astype(F32):                     # %.9g carries every float32
        q = dict(st, det_min=v)
        assert dr.stats_bytes(pipeline.parse_diag(pipeline.format_diag(q))) == dr.stats_bytes(q)
    for bad in ("", text + "x 1\n", text.replace("folded", "fold"), "\n".join(text.splitlines()[::-1])):
        with pytest.raises(ValueError):
            pipeline.parse_diag(bad)


# ---- the tokens ----------------------------------------------------------------------------------------------------------
_SIX = "a b c d e f"
DIAG_CORPUS = [
    _SIX + " junk x=y", _SIX + " junk x=y bwd=B.flo occ=O.png occ_bwd=OB.png",
    _SIX + " diag=D.txt", _SIX + " fold=F.png", _SIX + " fold=F.png diag=D.txt",
    _SIX + " junk x=y fold=F.png mid=4,9:pre diag=D.txt bwd=B.flo", _SIX + " diag= fold=F.png", _SIX + " diag=D1 diag=D2",
    _SIX + " diagnostics=D fold", "a b c d e diag=D.txt",
]


def test_tokens_through_both_grammars():
    from arap_flow_amd import build, pipeline
    assert pipeline.EXTRA_KEYS == ("bwd", "occ", "occ_bwd", "mid", "diag", "fold")
    tool = [b for b in build.build_host() if osp.basename(b) == "line_tool"][0]
    r = subprocess.run([tool], input="".join(c + "\n" for c in DIAG_CORPUS), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(DIAG_CORPUS)
    for line, g in zip(DIAG_CORPUS, got):
        item = pipeline.parse_line(line)
        assert g == pipeline.format_line(item) + " done=" + pipeline.done_token(item), line
    ex = [pipeline.parse_line(c).extra for c in DIAG_CORPUS]
    assert ex[0] == {} and ex[1] == dict(bwd="B.flo", occ="O.png", occ_bwd="OB.png")       # the old reading
    assert ex[2] == dict(diag="D.txt") and ex[4] == dict(fold="F.png", diag="D.txt")
    assert pipeline.format_line(pipeline.parse_line(DIAG_CORPUS[5])) == _SIX + " bwd=B.flo mid=4,9:pre diag=D.txt fold=F.png"
    assert ex[6] == dict(fold="F.png") and ex[7] == dict(diag="D2") and ex[8] == {}
    assert pipeline.parse_line(DIAG_CORPUS[9]).extra == {}            # six words: `diag=D.txt` is the warped mask's path


def test_deform_list_turns_diagnostics_on_only_for_batches_that_ask(monkeypatch):
    """a stand-in solver: plain batches never see set_diag; a batch with a diag= or fold= line turns it on in its lane,
    and the next plain batch of that lane turns it off again"""
    from arap_flow_amd import opt, pipeline, run_lines
    six = "r%d.png m%d.png c%d.txt f%d.flo w%d.png wm%d.png"
    extras = [{}, {}, dict(diag="d2.txt"), {}, {}, {}, {}, dict(fold="f7.png"), {}, {}]
    lines = [pipeline.parse_line(" ".join([six.replace("%d", str(k))] + pipeline.extra_tokens(e))) for k, e in enumerate(extras)]
    calls, made = [], []

    class Solver:
        def __init__(self, state, W, H, batch):
            self.id, self.slots = len(made), {}
            made.append(self)

        def set_frame(self, b, mask, cons, rgb=None, border_pins=False):
            self.slots[b] = cons

        def launches_for(self, n):
            return 1

        def set_outputs(self, backward, occlusion):
            pass

        def set_diag(self, on):
            calls.append(("set_diag", self.id, on))

        def solve_async(self, n, *a, **k):
            calls.append(("solve", self.id, [self.slots[b] for b in range(n)]))

        def wait(self):
            pass

        def host_results(self, b):
            return dict(flow=np.zeros(1))

        def close(self):
            pass

    monkeypatch.setattr(opt, "FrameSolver", Solver)
    monkeypatch.setattr(run_lines, "_load_line", lambda ln: (np.zeros((4, 6, 3), np.uint8), np.zeros((4, 6), np.uint8), lines.index(ln)))
    monkeypatch.setattr(run_lines, "_save_result", lambda ln, r: None)
    pipeline.deform_list(SimpleNamespace(use_own_stream=lambda: None), lines, max_batch=2, verbose=False)
    assert calls == [("solve", 0, [0, 1]), ("set_diag", 1, True), ("solve", 1, [2, 3]), ("solve", 0, [4, 5]),
                     ("solve", 1, [6, 7]), ("solve", 0, [8, 9])]
    calls.clear()
    del made[:]
    pipeline.deform_list(SimpleNamespace(use_own_stream=lambda: None), [lines[k] for k in (0, 1, 2, 3, 4, 5, 6, 8, 9)],
                         max_batch=2, verbose=False)
    assert calls == [("solve", 0, [0, 1]), ("set_diag", 1, True), ("solve", 1, [2, 3]), ("solve", 0, [4, 5]),
                     ("set_diag", 1, False), ("solve", 1, [6, 8]), ("solve", 0, [9])]


# ---- --multseg merge -----------------------------------------------------------------------------------------------------
def test_merge_diag(tmp_path):
    from arap_flow_amd import pipeline
    a = dict(vertices=10, outside=1, triangles=8, folded=2, nonfinite=0, det_min=F32(-0.0), det_max=F32(3), disp2_max=F32(2))
    b = dict(vertices=5, outside=0, triangles=0, folded=0, nonfinite=0, det_min=F32(INF), det_max=F32(-INF), disp2_max=F32(0))
    c = dict(vertices=7, outside=2, triangles=6, folded=1, nonfinite=3, det_min=F32(0.0), det_max=F32(0.5), disp2_max=F32(9))
    fa, fb, fc = (np.zeros((3, 4), np.uint8) for _ in range(3))
    fa[0, 0] = fc[2, 3] = fc[0, 0] = 255
    st, fold = pipeline.merge_diag([a, b, c], [fa, fb, fc])
    want = dict(vertices=22, outside=3, triangles=14, folded=3, nonfinite=3, det_min=F32(-0.0), det_max=F32(3), disp2_max=F32(9))
    assert dr.stats_bytes(st) == dr.stats_bytes(want)
    assert fold.dtype == np.uint8 and fold.tolist() == [[255, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 255]]
    assert dr.stats_bytes(pipeline.merge_diag([c, a])[0]) == dr.stats_bytes(dict(want, vertices=17, outside=3))
    assert dr.stats_bytes(pipeline.merge_diag([b])[0]) == dr.stats_bytes(b) and pipeline.merge_diag([b])[1] is None
    # the same as the twin on the union of disjoint masks whose segments share no quad
    g = dr.grid_field(9, 7)
    P = g + np.random.default_rng(5).normal(0, 0.5, g.shape).astype(F32)
    left, right = np.full((7, 9), 255, np.uint8), np.full((7, 9), 255, np.uint8)
    left[:, :4], right[:, 5:] = 0, 0
    parts = [dr.diag(left, P), dr.diag(right, P)]
    _noisy_precondition(parts[0][0])
    merged = pipeline.merge_diag([q[0] for q in parts], [q[1] for q in parts])
    assert dr.same(merged, dr.diag(np.minimum(left, right), P))
    # at file level
    from arap_flow_amd.pipeline import SolveLine
    segs = []
    for k, (s, f) in enumerate(parts):
        e = dict(diag=str(tmp_path / ("d_seg%d.txt" % k)), fold=str(tmp_path / ("f_seg%d.png" % k)))
        open(e["diag"], "w").write(pipeline.format_diag(s))
        pipeline.save_occ(f, e["fold"])
        segs.append(SolveLine(*"abcdef", extra=e))
    frame = SolveLine(*"abcdef", extra=dict(diag=str(tmp_path / "d.txt"), fold=str(tmp_path / "f.png")))
    pipeline.flatten_diag(frame, segs, remove=True)
    assert open(frame.extra["diag"]).read() == pipeline.format_diag(merged[0])
    assert np.array_equal(np.array(Image.open(frame.extra["fold"])), merged[1]) and Image.open(frame.extra["fold"]).mode == "L"
    assert sorted(os.listdir(tmp_path)) == ["d.txt", "f.png"]


# ---- para_gen: the lists ---------------------------------------------------------------------------------------------------
def _pair(tmp_path, name, stats, files=("rgb1_gen", "rgb2_gen", "flow_gen", "fold_gen")):
    from arap_flow_amd import pipeline
    p = {k: str(tmp_path / ("%s_%s" % (name, k))) for k in
         ("rgb1_gen", "msk1_gen", "cstr_tmp", "flow_gen", "rgb2_gen", "msk2_gen", "diag_gen", "fold_gen")}
    for k in files:
        open(p[k], "w").close()
    if stats is not None:
        open(p["diag_gen"], "w").write(pipeline.format_diag(stats))
    return p


def test_write_lists_keeps_and_rejects_from_the_diag_files(tmp_path):
    sys.path.insert(0, ROOT)
    import para_gen
    base = dict(vertices=100, outside=0, triangles=100, folded=0, nonfinite=0, det_min=F32(1), det_max=F32(1), disp2_max=F32(0))
    pairs = [_pair(tmp_path, "clean", base), _pair(tmp_path, "edge", dict(base, folded=10)),
             _pair(tmp_path, "over", dict(base, folded=11)), _pair(tmp_path, "nan", dict(base, nonfinite=1)),
             _pair(tmp_path, "dropped", None, files=()), _pair(tmp_path, "nofold", base, files=("rgb1_gen", "rgb2_gen", "flow_gen"))]
    trio = lambda p: " ".join([p["rgb1_gen"], p["rgb2_gen"], p["flow_gen"]])

    def run(flags):
        for f in ("all_files.list", "all_files_ext.list", "rejected.list"):
            if osp.exists(tmp_path / f):
                os.remove(tmp_path / f)
        ret = para_gen.write_lists(flags, str(tmp_path), pairs)
        read = lambda f: open(tmp_path / f).read().split("\n") if osp.exists(tmp_path / f) else None
        return ret, read("all_files.list"), read("all_files_ext.list"), read("rejected.list")

    (kept, rej), lst, ext, rejected = run(SimpleNamespace(diag=True, max_fold=0.1))
    assert lst == kept == [trio(pairs[k]) for k in (0, 1, 5)]
    assert ext == [" ".join([trio(pairs[k]), pairs[k]["diag_gen"], pairs[k]["fold_gen"]]) for k in (0, 1)]
    assert rejected == rej == [trio(pairs[2]) + " 11 100 0", trio(pairs[3]) + " 0 100 1"]
    assert run(SimpleNamespace(diag=True, max_fold=0.1)) == ((kept, rej), lst, ext, rejected)      # a second time: the same
    (kept0, rej0), lst0, _, rejected0 = run(SimpleNamespace(diag=True, max_fold=0.0))
    assert lst0 == [trio(pairs[k]) for k in (0, 5)] and len(rejected0) == 3
    _, lst1, _, rejected1 = run(SimpleNamespace(diag=True, max_fold=1.0))
    assert lst1 == [trio(pairs[k]) for k in (0, 1, 2, 5)] and rejected1 == [trio(pairs[3]) + " 0 100 1"]
    # --diag alone lists everything and writes no rejected.list; without either flag there is no ext list
    _, lst2, ext2, rejected2 = run(SimpleNamespace(diag=True))
    assert lst2 == [trio(pairs[k]) for k in (0, 1, 2, 3, 5)] and len(ext2) == 4 and rejected2 is None
    plain = [{k: v for k, v in p.items() if k not in ("diag_gen", "fold_gen")} for p in pairs]
    for f in ("all_files.list", "all_files_ext.list"):
        os.remove(tmp_path / f)
    para_gen.write_lists(SimpleNamespace(), str(tmp_path), plain)
    assert open(tmp_path / "all_files.list").read().split("\n") == lst2 and not osp.exists(tmp_path / "all_files_ext.list")


def test_para_gen_flags_and_refusals(tmp_path, capsys):
    sys.path.insert(0, ROOT)
    import para_gen
    base = ["--input", str(tmp_path), "--output", str(tmp_path / "o"), "--matches", str(tmp_path)]
    f = para_gen.parse(base)
    assert f.diag is False and f.max_fold is None
    f = para_gen.parse(base + ["--max_fold", "0.25"])
    assert f.diag is True and f.max_fold == 0.25
    assert para_gen.parse(base + ["--max_fold", "0"]).max_fold == 0 and para_gen.parse(base + ["--max_fold", "1"]).diag
    for bad in (["--max_fold", "-0.1"], ["--max_fold", "1.5"], ["--max_fold", "nan"], ["--max_fold"],
                ["--diag", "--arap_bin", "/bin/true"], ["--max_fold", "0.5", "--arap_bin", "/bin/true"]):
        with pytest.raises(SystemExit):
            para_gen.parse(base + bad)
    capsys.readouterr()
    # the path table: Diag / Fold beside the other outputs, part of what --resume looks for
    inp = tmp_path / "in"
    os.makedirs(inp / "orgRGB" / "s"); os.makedirs(inp / "orgMasks" / "s")
    for n in range(2):
        Image.new("RGB", (8, 8)).save(inp / "orgRGB" / "s" / ("%05d.png" % n))
        Image.new("L", (8, 8)).save(inp / "orgMasks" / "s" / ("%05d.png" % n))
    outp = tmp_path / "out"
    e = para_gen.scan(SimpleNamespace(fd=1, resume=False, diag=True), str(inp), str(outp))
    assert len(e) == 1 and e[0]["diag_gen"] == str(outp / "Diag" / "s" / "00000.txt")
    assert e[0]["fold_gen"] == str(outp / "Fold" / "s" / "00000.png")
    assert "diag_gen" not in para_gen.scan(SimpleNamespace(fd=1, resume=False), str(inp), str(outp))[0]
    from arap_flow_amd import pipeline
    ln = pipeline.make_arap_path(e[0])
    assert ln.extra == dict(diag=e[0]["diag_gen"], fold=e[0]["fold_gen"])
    seg = pipeline.replace_ext(e[0], 3, keep_orgs=["rgb1_gen", "cstr_tmp"])
    assert seg["diag_gen"].endswith("00000_seg3.txt") and seg["fold_gen"].endswith("00000_seg3.png")
    for k in ("flow_gen", "fold_gen"):
        os.makedirs(osp.dirname(e[0][k]), exist_ok=True)
        open(e[0][k], "w").close()
    resume = SimpleNamespace(fd=1, resume=True, diag=True)
    assert len(para_gen.scan(resume, str(inp), str(outp))) == 1          # the diag file is missing: not skipped
    os.makedirs(osp.dirname(e[0]["diag_gen"]), exist_ok=True)
    open(e[0]["diag_gen"], "w").close()
    assert len(para_gen.scan(resume, str(inp), str(outp))) == 0
