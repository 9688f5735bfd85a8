"""CPU-only tests of para_gen.py's scheduler: a pair's plan of follow-up lines as prepare_pair writes it, the schedules of
the flag sets no other host test runs (a full main() over a recording stand-in worker, tests/helpers.py), and every refusal
of parse()'s two tables, word for word."""
import json
import os
import os.path as osp
import re
import sys

import numpy as np
import pytest
from PIL import Image

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, ROOT)
import helpers                              # noqa: E402
import para_gen                             # noqa: E402
from arap_flow_amd import pipeline          # noqa: E402
from test_pipeline_host import _tiny_tree   # noqa: E402

OWN = "%s %s" % (sys.executable, osp.join(ROOT, "arap_deform.py"))


def _tree(tmp_path, nframes):
    inp, mdir = _tiny_tree(tmp_path, nframes=nframes, seqs=("a", "b"))
    os.makedirs(tmp_path / "bgs")
    Image.fromarray(np.random.default_rng(1).integers(0, 256, (50, 80, 3)).astype(np.uint8)).save(tmp_path / "bgs" / "b.png")
    return ["--input", str(inp), "--output", str(tmp_path / "out"), "--matches", str(mdir), "--arap_bin", OWN]


# ---- 1. the plan as a pure function ------------------------------------------------------------------------------------
S, L, T = ("SolveLine", "solves_done"), ("LayersLine", "layers_done"), ("TrkLine", "tracks_done")
B, LI = ("BgLine", "bg_done"), ("LightLine", "light_done")
FIN = "finish_frame"                        # (para_gen.FINISH, spelled out: the table below is written by hand)
BG = ["--bg_dir", "BGS"]
# the order of para_gen.py's docstring, written out by hand: every solve; layers and trk together; one of tex / blur / seg;
# finish_frame; the pair's bg line; the twin's bg line (counted as tex_done) or the light line.  The tiny tree has two labels:
# two solves with --multseg.  Last column: the suffixes of the files each stage deletes.
PLANS = [
    ([], [[S], FIN], [()]),
    (["--multseg"], [[S, S], FIN], [()]),
    (["--multseg", "--occ_layers"], [[S, S], [L], FIN], [(), ()]),
    (["--multseg", "--mid_layers", "2", "--occ_layers"], [[S, S], [L], FIN], [(), ()]),
    (["--mid", "2", "--tracks", "5"], [[S], [T], FIN], [(), ("_pts.trk",)]),
    (["--multseg", "--mid_layers", "2", "--tracks", "5"], [[S, S], [L, T], FIN], [(), ("_pts.trk",)]),
    (BG + ["--bg_motion"], [[S], FIN, [B]], [(), ("_bg.png", "_bg.txt")]),
    (BG + ["--bg_motion", "--mid", "2", "--mid_bg"], [[S], FIN, [B]], [(), ("_bg.png", "_bg.txt")]),
    (BG + ["--bg_motion", "--retex"], [[S], [("TexLine", "tex_done")], FIN, [B], [("BgLine", "tex_done")]],
     [(), (), (), ("_bg.png", "_bg.txt")]),
    (BG + ["--bg_motion", "--relight"], [[S], FIN, [B], [LI]], [(), (), ("_bg.png", "_bg.txt")]),
    (BG + ["--relight", "--multseg"], [[S, S], FIN, [LI]], [(), ("_lightmask.png",)]),
    (BG + ["--blur", "0.5"], [[S], [("BlurLine", "blur_done")], FIN], [(), ("_blurbg.png",)]),
    (["--seg"], [[S], [("SegLine", "seg_done")], FIN], [(), ()]),
    (["--diag", "--multseg"], [[S, S], FIN], [()]),
    # (beyond the list: the bg line's inputs of a --multseg pair include the union mask, and go after the light line)
    (BG + ["--bg_motion", "--relight", "--multseg"], [[S, S], FIN, [B], [LI]], [(), (), ("_bg.png", "_bgmask.png", "_bg.txt")]),
]


@pytest.fixture(scope="module")
def plan_tree(tmp_path_factory):
    d = tmp_path_factory.mktemp("plan")
    return d, _tree(d, nframes=2)


@pytest.mark.parametrize("extra,stages,removed", PLANS, ids=[" ".join(p[0]) or "plain" for p in PLANS])
def test_plan_of_a_pair(plan_tree, extra, stages, removed):
    d, argv = plan_tree
    extra = [str(d / "bgs") if a == "BGS" else a for a in extra]
    flags = para_gen.parse(argv + extra)
    p = para_gen.scan(flags, flags.input, flags.output)[0]
    rec = para_gen.prepare_pair((flags, p, str(d / "bgs" / "b.png") if "--bg_dir" in extra else None))
    got = [st if st == FIN else [(type(s.line).__name__, s.count) for s in st] for st in rec.plan]
    assert got == stages
    stem = osp.splitext(p["cstr_tmp"])[0]
    assert [tuple(q[len(stem):] for q in sum((s.remove for s in st), ())) for st in rec.plan if st != FIN] == list(removed)
    # what main owes the workers: every line of the hand-written table after the solves
    assert len(para_gen.follow_up_steps(rec.plan)) == sum(len(st) for st in stages[1:] if st != FIN)
    assert [s.line for s in rec.plan[0]] == rec.solves and rec.left == 0


def test_a_dropped_pair_has_no_plan(plan_tree):
    d, argv = plan_tree
    flags = para_gen.parse(argv + ["--output", str(d / "out_dropped"), "--matches", str(d / "no_matches")])
    p = para_gen.scan(flags, flags.input, flags.output)[0]
    os.makedirs(d / "no_matches" / p["_seq"], exist_ok=True)
    (d / "no_matches" / p["_seq"] / (p["_stem"] + ".txt")).write_text("")       # no match: no constraint, no solve
    assert para_gen.prepare_pair((flags, p, None)) is None


# ---- 2. the schedules no other host test runs: main() over the recording stand-in --------------------------------------
def _pair_of(item):
    """(sequence, frame) of the pair a line belongs to, from a file only that pair's lines name"""
    q = {pipeline.SolveLine: lambda it: it.flow, pipeline.LayersLine: lambda it: it.rgb, pipeline.BgLine: lambda it: it.rgb1,
         pipeline.TrkLine: lambda it: it.out}[type(item)](item)
    return osp.basename(osp.dirname(q)), re.sub(r"_seg\d+$", "", osp.splitext(osp.basename(q))[0])


TMP_NAMES = ("_bg.png", "_bgmask.png", "_bg.txt", "_pts.trk", "_blurbg", "_lightmask")
RUNS = [      # flags, solves per pair, (layers, trk, bg) lines per pair, files per line of all_files_ext.list
    (["--bg_motion"], 1, (0, 0, 1), 3 + 1),
    (["--bg_motion", "--bwd_flow", "--occ"], 1, (0, 0, 1), 3 + 3 + 4),
    (["--mid", "2", "--tracks", "5"], 1, (0, 1, 0), 3 + 8 + 1),
    (["--multseg", "--mid_layers", "2", "--occ_layers", "--tracks", "5"], 2, (1, 1, 0), 3 + 1 + 8 + 3 + 1),
    (["--multseg", "--bg_motion", "--mid_layers", "2", "--mid_bg", "--occ_layers"], 2, (1, 0, 1), 3 + 1 + 2 + 8 + 3 + 2 + 3 + 3),
    (["--diag", "--multseg", "--max_fold", "0.5"], 2, (0, 0, 0), 3 + 2),
]


@pytest.mark.parametrize("keep", [False, True], ids=["", "keep_segments"])
@pytest.mark.parametrize("extra,nsolves,later,next_len", RUNS, ids=[" ".join(r[0]) for r in RUNS])
def test_para_gen_schedule_with_a_recording_worker(tmp_path, extra, nsolves, later, next_len, keep):
    argv = _tree(tmp_path, nframes=4)                                       # 2 sequences x 3 pairs
    log, outp = tmp_path / "lines.log", tmp_path / "out"
    flags = para_gen.parse(argv + ["--gpu", "0", "1", "--worker", "serve", "--narap", "3", "--jobs", "2"] + extra +
                           (["--bg_dir", str(tmp_path / "bgs")] if "--bg_motion" in extra else []) +
                           (["--keep_segments"] if keep else []))
    flags.arap_bin = helpers.recording_worker(tmp_path / "worker.py", log, ROOT)    # (the flags were checked against OWN)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        out = para_gen.main(flags)          # the stand-in exits 3, and main raises, when a line comes before what it reads
    finally:
        os.chdir(cwd)
    lines = [pipeline.parse_line(ln) for ln in log.read_text().splitlines()]
    n_layers, n_trk, n_bg = later
    kinds = (pipeline.SolveLine,) * nsolves + (pipeline.LayersLine,) * n_layers + (pipeline.TrkLine,) * n_trk + (pipeline.BgLine,) * n_bg
    by_pair = {}
    for at, it in enumerate(lines):
        by_pair.setdefault(_pair_of(it), []).append((at, type(it)))
    assert sorted(by_pair) == [(s, "%05d" % n) for s in "ab" for n in range(3)]
    rank = {pipeline.SolveLine: 0, pipeline.LayersLine: 1, pipeline.TrkLine: 1, pipeline.BgLine: 2}
    for pair, got in by_pair.items():       # every line of the pair exactly once; solves < layers, trk (either order) < bg
        assert sorted(t.__name__ for _, t in got) == sorted(t.__name__ for t in kinds), pair
        ranks = [rank[t] for _, t in sorted(got)]
        assert ranks == sorted(ranks), (pair, got)
    st = json.load(open(outp / "arap_stats.json"))
    want = dict(pairs=6, frames=6, solves=6 * nsolves, frames_done=6, layers_done=6 * n_layers, tracks_done=6 * n_trk,
                bg_done=6 * n_bg, tex_done=0, blur_done=0, light_done=0, seg_done=0)
    assert {k: st[k] for k in want} == want and ("rejected" in st) == ("--max_fold" in extra)
    assert "solves_done" not in st
    listed = (outp / "all_files.list").read_text().split("\n")
    ext = [ln.split(" ") for ln in (outp / "all_files_ext.list").read_text().split("\n")]
    assert out == listed and len(listed) == 6 and [" ".join(e[:3]) for e in ext] == listed
    assert all(len(e) == next_len and all(osp.exists(q) for q in e) for e in ext)
    if "--max_fold" in extra:
        assert (outp / "rejected.list").read_text() == "" and st["rejected"] == 0
    for name in ("all_files_tex.list", "all_files_blur.list", "all_files_light.list"):
        assert not (outp / name).exists()
    # (a segment's INPUT mask, OUT/inpMasks/<seq>/<frame>_segN.png, always stays, as in the reference: only what the solves
    # and the lines wrote per segment is merged and removed)
    names = [f for r, _, fs in os.walk(outp) for f in fs if osp.basename(osp.dirname(r)) != "inpMasks"]
    left = sorted({t for t in TMP_NAMES + ("_seg",) for f in names if t in f})
    want_left = (("_seg",) if nsolves > 1 else ()) + (("_pts.trk",) if n_trk else ()) + \
        ((("_bg.png", "_bg.txt") + (("_bgmask.png",) if nsolves > 1 else ())) if n_bg else ())
    assert left == (sorted(want_left) if keep else []), left


# ---- 3. the refusals of parse()'s two tables, word for word ---------------------------------------------------------------
NEEDS = " this repository's arap_deform (C++ or arap_deform.py): a foreign --arap_bin does "
FOREIGN = [
    (["--seg"], "--seg needs" + NEEDS + "not know the seg line"),
    (["--bg_dir", "b", "--relight"], "--relight needs" + NEEDS + "not know the light line"),
    (["--bg_dir", "b", "--blur", "0.5"], "--blur needs" + NEEDS + "not know the blur line"),
    (["--mid", "2", "--tracks", "5"], "--tracks needs" + NEEDS + "not know the trk line"),
    (["--retex"], "--retex needs" + NEEDS + "not know the tex line"),
    (["--diag"], "--diag / --max_fold need" + NEEDS + "not write the diagnostics"),
    (["--max_fold", "0.5"], "--diag / --max_fold need" + NEEDS + "not write the diagnostics"),
    (["--multseg", "--occ_layers"], "--occ_layers needs" + NEEDS + "not know the layers line"),
    (["--bwd_flow"], "--bwd_flow / --occ need" + NEEDS + "not write the extra outputs"),
    (["--occ"], "--bwd_flow / --occ need" + NEEDS + "not write the extra outputs"),
    (["--bg_dir", "b", "--bg_motion"], "--bg_motion needs" + NEEDS + "not know the bg line"),
    (["--mid", "2"], "--mid needs" + NEEDS + "not know the mid= token"),
    (["--multseg", "--mid_layers", "2"], "--mid_layers needs" + NEEDS + "not know the layers line"),
]
GIVE = dict(mid=["--mid", "2"], mid_layers=["--multseg", "--mid_layers", "2"], mid_bg=["--mid_bg"], retex=["--retex"],
            blur=["--blur", "0.5"], relight=["--relight", "0"], bg_motion=["--bg_motion"], seg=["--seg"],
            tracks=["--mid", "2", "--tracks", "5"])
EXCLUSIVE = [
    ("seg", ("mid", "mid_layers", "mid_bg", "retex", "blur", "relight"),
     "--seg cannot be combined with --mid / --mid_layers / --mid_bg / --retex / --blur / --relight: the variants share the "
     "clean pair's geometry files, and maps of in-between frames are made with opt.seg_maps, not from this command line"),
    ("relight", ("mid", "mid_layers", "mid_bg", "retex", "blur"),
     "--relight cannot be combined with --mid / --mid_layers / --mid_bg / --retex / --blur: relit sequences, twins and "
     "blurred frames are made with opt.relight, not from this command line"),
    ("blur", ("mid", "mid_layers", "mid_bg", "retex"),
     "--blur cannot be combined with --mid / --mid_layers / --mid_bg / --retex: blurred sequences and blurred twins are made "
     "with opt.blur_layers, not from this command line"),
    ("tracks", ("bg_motion",),
     "--tracks cannot be combined with --bg_motion: a track of a background point assumes the static background"),
    ("retex", ("mid", "mid_layers", "mid_bg"),
     "--retex cannot be combined with --mid / --mid_layers / --mid_bg: sequences of retextured in-between frames are not built"),
]
TWO_OFFENCES = [      # the earlier check of parse() wins
    (["--seg", "--relight"], EXCLUSIVE[0][2]),                                 # (not: --relight needs --bg_dir)
    (["--retex", "--mid", "2", "--arap_bin", "/bin/true"], EXCLUSIVE[4][2]),      # (not: --retex needs this repository's ...)
    (["--bg_dir", "b", "--blur", "0.5", "--relight", "--arap_bin", "/bin/true"], EXCLUSIVE[1][2]),
    (["--occ", "--multseg", "--arap_bin", "/bin/true"],
     "--occ cannot be combined with --multseg: forward occlusion across segments needs one query over every segment's solve, "
     "which --occ does not do; use --multseg --occ_layers (--bwd_flow --multseg is supported)"),
]


def _refused(capsys, argv):
    with pytest.raises(SystemExit):
        helpers.para_gen_flags(argv)
    return capsys.readouterr().err


def test_parse_refuses_a_foreign_arap_bin_word_for_word(capsys):
    for argv, message in FOREIGN:
        assert _refused(capsys, argv + ["--arap_bin", "/bin/true"]).endswith(" error: " + message + "\n"), argv
        helpers.para_gen_flags(argv + ["--arap_bin", OWN])                        # this repository's driver: accepted


def test_parse_refuses_exclusive_flags_word_for_word(capsys):
    for flag, others, message in EXCLUSIVE:
        for other in others:
            argv = ["--bg_dir", "b", "--arap_bin", OWN] + GIVE[flag] + GIVE[other]
            assert _refused(capsys, argv).endswith(" error: " + message + "\n"), argv


def test_parse_reports_the_earlier_of_two_offences(capsys):
    for argv, message in TWO_OFFENCES:
        assert _refused(capsys, argv).endswith(" error: " + message + "\n"), argv
