"""CPU-only: motion blur (DESIGN.md "Motion blur") around the kernels.  The numpy twin tests/blur_ref.py against its
sequential statement; the schedule ArapFlow_BlurSchedule (host only) against pipeline.blur_times / blur_maps bit for bit; the
rounding formulas at their extremes; the `blur` list line in Python and in C++ (host/list_line.h through line_tool);
para_gen --blur with a stand-in worker."""
import ctypes as C
import json
import os
import os.path as osp
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import bg_ref
import blur_ref
import occ_layers_ref
from arap_flow_amd import pipeline

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
F = np.float32
MA = bg_ref.similarity(4.0, 1.05, (1.5, 0.25), (3.5, 2.5))
MB = bg_ref.similarity(-3.0, 0.95, (2.0, 1.5), (3.5, 2.5))


# ---- the twin against the sequential statement --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    rgb, masks, flows = occ_layers_ref.layered_case(7, 5, 2, seed=3, overlap=True)
    rng = np.random.default_rng(1)
    return dict(rgb=rgb, masks=masks, flows=flows, flows_a=(rng.normal(size=flows.shape) * 0.5).astype(F),
                bg=rng.integers(0, 256, (9, 11, 3)).astype(np.uint8))


@pytest.mark.parametrize("bg", [False, True], ids=["nobg", "bg"])
@pytest.mark.parametrize("first", [False, True], ids=["a0", "a"])
def test_twin_equals_the_sequential_statement(tiny, bg, first):
    """7x5, n = 2, S = 3, with and without the background"""
    kw = dict(bg=tiny["bg"], Ma=MA, Mb=MB) if bg else {}
    fa = tiny["flows_a"] if first else None
    got = blur_ref.blur_ref(tiny["rgb"], tiny["masks"], tiny["flows"], 0.5 if first else 1.0, 1.0, 3, flows_a=fa, **kw)
    want = blur_ref.blur_brute(tiny["rgb"], tiny["masks"], tiny["flows"], 0.5 if first else 1.0, 1.0, 3, flows_a=fa, **kw)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (got[1] == 255).any() and ((got[1] > 0) & (got[1] < 255)).any()      # fully and partly covered pixels exist
    if not bg:
        assert (got[0][got[1] == 0] == 0).all()                                 # premultiplied: nothing where nothing is


def test_twin_one_sample_is_the_layered_warp(tiny):
    r = occ_layers_ref.layers_ref(tiny["rgb"], tiny["masks"], occ_layers_ref.fields_from_flows(tiny["flows"]))
    for shutter in (0.0, 1.0):
        rgb, alpha = blur_ref.blur_ref(tiny["rgb"], tiny["masks"], tiny["flows"], 1.0, shutter, 1, flows_a=tiny["flows_a"])
        assert np.array_equal(rgb, r["warped_rgb"]) and np.array_equal(alpha, r["warped_mask"])
    assert np.array_equal(blur_ref.mix(tiny["flows_a"], tiny["flows"], 1.0), tiny["flows"])          # t = 1 gives b exactly
    assert np.array_equal(blur_ref.mix(tiny["flows_a"], tiny["flows"], 0.0), tiny["flows_a"])        # t = 0 gives a exactly


# ---- the rounding formulas -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", range(1, 33))
def test_rounding_extremes(S):
    assert blur_ref.mean_alpha(S, S) == 255 and blur_ref.mean_alpha(0, S) == 0
    assert blur_ref.mean_rgb(255 * S, S) == 255 and blur_ref.mean_rgb(0, S) == 0
    tot = np.arange(0, 255 * S + 1)
    exact = np.floor(tot / S + 0.5)                        # (tot / S + 0.5 is exact enough: S <= 32, tot < 2^13)
    assert np.array_equal(blur_ref.mean_rgb(tot, S), exact.astype(np.uint8))
    if S % 2 == 0:                                         # half-way cases round up
        assert blur_ref.mean_rgb(S // 2, S) == 1 and blur_ref.mean_rgb(S // 2 - 1, S) == 0
        assert blur_ref.mean_rgb(3 * S // 2, S) == 2
    cnt = np.arange(0, S + 1)
    assert np.array_equal(blur_ref.mean_alpha(cnt, S), np.floor(255 * cnt / S + 0.5).astype(np.uint8))
    assert (blur_ref.mean_alpha(cnt[:-1], S) < 255).all()                   # 255 only where every sample covers


# ---- the schedule: the library against the Python statement ------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from arap_flow_amd import build, capi
    build.build()
    return capi.load()


def schedule(lib, c, e, S, Ma=None, Mb=None, maps=True):
    m6 = lambda m: None if m is None else (C.c_float * 6)(*[float(v) for v in m])
    times, out = (C.c_float * 32)(), (C.c_float * (6 * 32))()
    rc = lib.ArapFlow_BlurSchedule(c, e, S, m6(Ma), m6(Mb), times, out if maps else None)
    return rc, np.array(times[:max(S, 0)][:32], F), np.array(out[:6 * min(max(S, 0), 32)], F).reshape(-1, 6)


@pytest.mark.parametrize("S", [1, 2, 9, 32])
def test_schedule_equals_python_bit_for_bit(lib, S):
    for c in (0.0, 1.0, 0.5):
        for e in (0.0, 0.5, 1.0, 0.3):
            rc, t, m = schedule(lib, c, e, S, MA, MB)
            assert rc == 0
            want_t = pipeline.blur_times(c, e, S)
            assert t.tobytes() == want_t.tobytes() == blur_ref.times(c, e, S).tobytes()
            want_m = pipeline.blur_maps(want_t, MA, MB)
            assert m.tobytes() == want_m.tobytes() == blur_ref.maps(want_t, MA, MB).tobytes()
            if S == 1:
                assert t[0] == F(c)                                         # one sample sits at the centre, whatever e
            if e == 0.0:
                assert (t == F(c)).all()
            assert np.allclose(t.astype(np.float64).mean(), c, atol=1e-6)   # the window is centred on c
            assert (np.diff(t) >= 0).all() and (e == 0 or S == 1 or t[-1] - t[0] < e)
            rc, t2, m2 = schedule(lib, c, e, S, MA, MA)                     # a still camera: every map is Ma itself
            assert rc == 0 and t2.tobytes() == t.tobytes() and (m2.view(np.uint32) == MA.view(np.uint32)).all()
            assert (pipeline.blur_maps(want_t, MA, MA).view(np.uint32) == MA.view(np.uint32)).all()
            rc, t3, _ = schedule(lib, c, e, S, maps=False)                  # no maps asked: Ma and Mb are not read
            assert rc == 0 and t3.tobytes() == t.tobytes()
    assert not (pipeline.blur_maps(pipeline.blur_times(0.5, 1.0, 2), MA, MB).view(np.uint32) == MA.view(np.uint32)).all()


def test_opt_blur_schedule_is_the_library_call(lib):
    from arap_flow_amd import opt
    t, m = opt.blur_schedule(0.5, 0.3, 9, maps=(MA, MB), lib=lib)
    rc, want_t, want_m = schedule(lib, 0.5, 0.3, 9, MA, MB)
    assert rc == 0 and t.tobytes() == want_t.tobytes() and m.tobytes() == want_m.tobytes() and m.shape == (9, 6)
    t, m = opt.blur_schedule(1.0, 1.0, 32, lib=lib)
    assert m is None and t.tobytes() == pipeline.blur_times(1.0, 1.0, 32).tobytes()
    for args in ((1.0, 0.5, 0), (1.0, 0.5, 33), (1.0, -0.5, 3), (float("nan"), 0.5, 3)):
        with pytest.raises(ValueError):
            opt.blur_schedule(*args, lib=lib)


def test_schedule_rounds_once_from_double(lib):
    """t is the double expression rounded once, not float32 arithmetic: the two differ for some k at S = 9, e = 0.3"""
    c, e, S = F(1.0), F(0.3), 9
    rc, t, _ = schedule(lib, c, e, S, maps=False)
    single = np.array([c + e * (F(F(k + 0.5) / F(S)) - F(0.5)) for k in range(S)], F)
    double = np.array([float(c) + float(e) * ((k + 0.5) / S - 0.5) for k in range(S)]).astype(F)
    assert rc == 0 and t.tobytes() == double.tobytes()
    assert t.tobytes() != single.tobytes()


def test_schedule_refusals(lib):
    nan, inf = float("nan"), float("inf")
    bad = np.array(MA)
    bad[2] = inf
    for kw in (dict(S=0), dict(S=33), dict(c=nan), dict(c=inf), dict(e=nan), dict(e=inf), dict(e=-0.25), dict(Ma=None),
               dict(Mb=None), dict(Ma=bad), dict(Mb=bad)):
        a = dict(dict(c=1.0, e=0.5, S=5, Ma=MA, Mb=MB), **kw)
        assert schedule(lib, a["c"], a["e"], a["S"], a["Ma"], a["Mb"])[0] == -1, kw
    assert lib.ArapFlow_BlurSchedule(1.0, 0.5, 5, None, None, None, None) == -1         # no times
    assert schedule(lib, 1.0, 0.5, 5, None, None, maps=False)[0] == 0
    for args in ((1.0, 0.5, 0), (1.0, 0.5, 33), (nan, 0.5, 3), (1.0, -1.0, 3), (1.0, inf, 3)):
        with pytest.raises(ValueError):
            pipeline.blur_times(*args)
    with pytest.raises(ValueError):
        pipeline.blur_maps(pipeline.blur_times(1.0, 0.5, 3), MA, bad)
    # sizes the device call refuses have no scratch size (host only too)
    assert lib.ArapFlow_BlurLayersScratchBytes(70, 9, 3, 0) == 0 and lib.ArapFlow_BlurLayersScratchBytes(70, 9, 3, 33) == 0
    assert lib.ArapFlow_BlurLayersScratchBytes(70, 9, 0, 5) == 0 and lib.ArapFlow_BlurLayersScratchBytes(70, 9, 256, 5) == 0
    assert lib.ArapFlow_BlurLayersScratchBytes(0, 9, 3, 5) == 0 and lib.ArapFlow_BlurLayersScratchBytes(1 << 16, 1 << 15, 3, 5) == 0
    from arap_flow_amd import capi
    N, G = 70 * 9, capi.BLUR_CHUNK
    up = lambda v: (v + 255) // 256 * 256
    assert lib.ArapFlow_BlurLayersScratchBytes(70, 9, 3, 5) == up(5 * 8 * N)            # keys of what is rasterised, no carry
    assert lib.ArapFlow_BlurLayersScratchBytes(70, 9, 255, G) == up(G * 8 * N)
    assert lib.ArapFlow_BlurLayersScratchBytes(70, 9, 3, G + 1) == lib.ArapFlow_BlurLayersScratchBytes(70, 9, 3, 32) == up(G * 8 * N) + up(8 * N)


# ---- the blur line: host/list_line.h against pipeline.parse_line ------------------------------------------------------
_M = "1,0,0,0,1,0,1.01,0.02,3,-0.02,1.01,-2.5"
_B = "blur R 1 m1 f1 BG"
GOOD = [
    _B + " b=0.5,9 rgb1=A", _B + " rgb2=B b=0.5,9 m=" + _M + " rgb1=A alpha2=C",       # done = B: the first output on the line
    _B + " b=0,1 alpha1=C", "blur R 2 m1 f1 m2 f2 BG b=1e-3,32 m=" + _M + " rgb1=A rgb2=B alpha1=C alpha2=D",
    _B + " b=0.100000001,8 alpha2=D rgb2=B", _B + " m=" + _M.replace("-2.5", "1e-3") + " b=2,5 rgb2=B",
]
BAD = [
    _B + " b=0.5,9", _B + " rgb1=A", _B + " m=" + _M + " rgb1=A",                    # no output; no b=
    _B + " b=0.5,9 rgb1=A foo=B", _B + " b=0.5,9 rgb1=A mask2=O",                    # unknown keys
    _B + " b=0.5,9 rgb1=", _B + " b= rgb1=A", _B + " b=0.5,9 rgb1", _B + " b=0.5,9 m= rgb1=A",     # empty values, a missing `=`
    _B + " b=0.5 rgb1=A", _B + " b=0.5,9,1 rgb1=A", _B + " b=,9 rgb1=A", _B + " b=0.5, rgb1=A",      # not two numbers
    _B + " b=0.5,0 rgb1=A", _B + " b=0.5,33 rgb1=A", _B + " b=0.5,9.0 rgb1=A", _B + " b=0.5,-9 rgb1=A", _B + " b=0.5,x rgb1=A",
    _B + " b=-0.5,9 rgb1=A", _B + " b=nan,9 rgb1=A", _B + " b=inf,9 rgb1=A", _B + " b=1e39,9 rgb1=A", _B + " b=x,9 rgb1=A",
    _B + " b=0.5,9 m=" + _M + ",4 rgb1=A", _B + " b=0.5,9 m=" + _M[:-5] + " rgb1=A",     # 13 and 11 numbers
    _B + " b=0.5,9 m=" + _M.replace("1.01", "nan") + " rgb1=A", _B + " b=0.5,9 m=" + _M.replace("1.01", "1e39") + " rgb1=A",
    _B + " b=0.5,9 m=" + _M.replace("1.01", "x") + " rgb1=A",
    _B + " b=0.5,9 rgb1=A rgb1=B", _B + " b=0.5,9 b=0.5,9 rgb1=A", _B + " b=0.5,9 m=" + _M + " m=" + _M + " rgb1=A",     # repeated keys
    "blur R 0 BG b=0.5,9 rgb1=A", "blur R 256 BG b=0.5,9 rgb1=A", "blur R x m1 f1 BG b=0.5,9 rgb1=A", "blur R 2 m1 f1 m2",
    "blur R 1 m1 f1 b=0.5,9 rgb1=A", "blur R 2 m1 f1 BG b=0.5,9 rgb1=A",             # no background where one is expected
    "blur", "blur R",
]


@pytest.fixture(scope="module")
def bins():
    from arap_flow_amd import build
    return {osp.basename(o): o for o in build.build_host()}


def test_blur_line_round_trip():
    item = pipeline.BlurLine("R", [("m1", "f1"), ("m2", "f2")], "BG", 0.1, 9, tuple(float(v) for v in np.concatenate([MA, MB])),
                             dict(alpha2="D", rgb1="A"))
    text = pipeline.format_line(item)
    back = pipeline.parse_line(text)
    assert back.shutter == float(F(0.1)) and back.samples == 9 and back.m == item.m and back.layers == item.layers
    assert (back.rgb, back.bg) == ("R", "BG") and back.out == dict(rgb1="A", alpha2="D")
    assert pipeline.format_line(back) == text and pipeline.done_token(back) == "A"
    assert pipeline.done_token(pipeline.parse_line(GOOD[1])) == "B"
    plain = pipeline.parse_line(GOOD[0])
    assert plain.m == () and " m=" not in pipeline.format_line(plain)       # no m=: both maps the identity, and none written
    for line in GOOD:
        assert isinstance(pipeline.parse_line(line), pipeline.BlurLine)
        assert pipeline.parse_line(pipeline.format_line(pipeline.parse_line(line))) == pipeline.parse_line(line)


def test_blur_line_parser_equals_python_twin(bins):
    """every line through line_tool in one process: a good one comes back as format_line(parse_line(line)) + its done
    token, a bad one as BAD after the grammar's own message -- and Python refuses exactly those"""
    corpus = GOOD + BAD
    r = subprocess.run([bins["line_tool"]], input="".join(c + "\n" for c in corpus), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")[:-1]
    got = [ln for ln in lines if not ln.startswith("Invalid")]
    assert len(got) == len(corpus)
    assert [ln for ln in lines if ln.startswith("Invalid")] == ["Invalid blur line: " + b for b in BAD]
    for line, g in zip(GOOD, got):
        item = pipeline.parse_line(line)
        assert g == pipeline.format_line(item) + " done=" + pipeline.done_token(item), line
    assert got[1].endswith(" done=B") and got[0].endswith(" done=A") and got[2].endswith(" done=C")
    for line, g in zip(BAD, got[len(GOOD):]):
        assert g == "BAD", line
        with pytest.raises(ValueError):
            pipeline.parse_line(line)


def test_arap_deform_refuses_a_bad_blur_line_before_any_gpu_call(bins, tmp_path):
    lst = tmp_path / "l.txt"
    lst.write_text("a b c d e f\n" + BAD[3] + "\n")
    r = subprocess.run([bins["arap_deform"], str(lst)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "Invalid blur line: " + BAD[3] + "\n"
    r = subprocess.run([sys.executable, osp.join(ROOT, "arap_deform.py"), str(lst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "blur line" in r.stdout


# ---- para_gen --blur with a stand-in worker ----------------------------------------------------------------------------
FAKE_WORKER = r'''
import os, shutil, sys
# stand-in for arap_deform (no GPU): a solve line writes the files para_gen expects; a blur line REFUSES to run (exit 3)
# unless every file it names is there already, then writes its outputs; a bg line writes its second frame and its flow;
# every line is logged
import numpy as np
from PIL import Image
sys.path.insert(0, %r)
from arap_flow_amd import flo as F, pipeline
LOG = %r
def run(line):
    item = pipeline.parse_line(line)
    with open(LOG, "a") as log:
        log.write(line.rstrip("\n") + "\n")
    if isinstance(item, pipeline.BlurLine):
        for q in [item.rgb, item.bg] + [q for pair in item.layers for q in pair]:
            if not os.path.exists(q):
                print("blur line before its inputs: " + q, flush=True)
                sys.exit(3)
        src = np.array(Image.open(item.rgb).convert("RGB"))
        src[::2] = (4, 5, 6)
        for k in item.out:
            Image.fromarray(src).save(item.out[k])
        return
    if isinstance(item, pipeline.BgLine):
        shutil.copy(item.flow, item.out[2])              # (out[1] is the pair's second frame itself, composited in place)
        return
    m = np.array(Image.open(item.mask).convert("RGB"))[..., 0]
    F.flow_write(item.flow, np.zeros(m.shape + (2,), np.float32))
    shutil.copy(item.rgb, item.out_rgb)
    Image.fromarray(m == 0).save(item.out_mask)
if sys.argv[1] == "--serve":
    print("Ready", flush=True)
    for line in sys.stdin:
        run(line)
        print("Done " + pipeline.done_token(pipeline.parse_line(line)), flush=True)
else:
    for l in open(sys.argv[1]).read().splitlines():
        if l.strip(): run(l)
'''


def _blur_run(tmp_path, extra, worker, blur=("0.5",)):
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
                            "--arap_bin", own, "--narap", "3", "--jobs", "2", "--bg_dir", str(tmp_path / "bgs"), "--blur"] +
                           list(blur) + extra)
    flags.arap_bin = "%s %s" % (sys.executable, fake)          # (the flags are checked against this repository's driver)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        out = para_gen.main(flags)
    finally:
        os.chdir(cwd)
    return outp, out, [pipeline.parse_line(ln) for ln in (log.read_text().splitlines() if log.exists() else [])]


@pytest.mark.parametrize("worker,multseg,motion", [("serve", False, False), ("serve", True, True), ("batch", True, False)])
def test_para_gen_blur_with_a_stand_in_worker(tmp_path, worker, multseg, motion):
    extra = (["--multseg"] if multseg else []) + (["--bg_motion"] if motion else [])
    outp, out, lines = _blur_run(tmp_path, extra, worker, blur=("0.25", "5") if motion else ("0.5",))
    assert len(out) == 6                                                    # 2 sequences x 3 pairs
    blur = [it for it in lines if isinstance(it, pipeline.BlurLine)]
    solves = [it for it in lines if isinstance(it, pipeline.SolveLine)]
    bgs = [it for it in lines if isinstance(it, pipeline.BgLine)]
    assert len(blur) == 6 and len(solves) == (12 if multseg else 6) and len(bgs) == (6 if motion else 0)
    # a blur line names the frame's solves (the stand-in refuses one whose flows are not written yet: the run got here)
    assert sorted(f for it in blur for _, f in it.layers) == sorted(s.flow for s in solves)
    assert all(len(it.layers) == (2 if multseg else 1) and set(it.out) == {"rgb1", "rgb2"} for it in blur)
    assert all((it.shutter, it.samples) == ((0.25, 5) if motion else (0.5, 9)) for it in blur)
    if motion:                                                              # the pair's own camera, the pair's own picture
        by_rgb = {it.rgb1: it for it in bgs}
        assert all(it.m == by_rgb[it.rgb].m and it.bg == by_rgb[it.rgb].bg and len(it.m) == 12 for it in blur)
        at = {id(it): k for k, it in enumerate(lines)}
        assert all(at[id(it)] < at[id(by_rgb[it.rgb])] for it in blur)      # before the segments are merged and the bg line runs
    else:
        assert all(it.m == () for it in blur)
    st = json.load(open(outp / "arap_stats.json"))
    assert st["blur_done"] == 6 and st["frames_done"] == 6 and st["tex_done"] == 0
    listed = (outp / "all_files_blur.list").read_text().split("\n")
    assert len(listed) == 6
    for pair, twin in zip(out, listed):
        (rgb1, rgb2, flow), (b1, b2, bflow) = pair.split(" "), twin.split(" ")
        assert bflow == flow and all(osp.exists(q) for q in (b1, b2, bflow))          # the SAME flow file
        assert b1 == rgb1.replace(osp.sep + "inpRGB" + osp.sep, osp.sep + "inpRGB_blur" + osp.sep)
        assert b2 == rgb2.replace(osp.sep + "wRGB" + osp.sep, osp.sep + "wRGB_blur" + osp.sep)
        assert (np.array(Image.open(b2).convert("RGB"))[::2] == (4, 5, 6)).all()
    if multseg:                                                             # per-segment files were merged and removed
        assert not [f for f in os.listdir(outp / "Flow" / "a") if "_seg" in f]
    assert not [f for f in os.listdir(outp / "tmpCnstr" / "a") if "_blurbg" in f]     # the line's own input is gone
    assert not (outp / "all_files_tex.list").exists()


def test_para_gen_blur_resume(tmp_path):
    """--resume skips a pair only when its blurred files exist too"""
    outp, out, lines = _blur_run(tmp_path, [], "serve")
    listed = (outp / "all_files_blur.list").read_text().split("\n")
    assert len(out) == 6 and len(listed) == 6
    gone = listed[2].split(" ")[1]
    os.remove(gone)
    outp, out2, lines = _blur_run(tmp_path, ["--resume"], "serve")
    blur = [it for it in lines if isinstance(it, pipeline.BlurLine)]
    assert len(blur) == 1 and blur[0].out["rgb2"] == gone and osp.exists(gone)
    outp, out3, lines = _blur_run(tmp_path, ["--resume"], "serve")
    assert lines == []                                                      # everything is there: nothing is handed out


def test_para_gen_without_blur_writes_nothing_of_it(tmp_path):
    sys.path.insert(0, ROOT)
    import helpers
    flags = helpers.para_gen_flags([])
    assert flags.blur is None
    assert helpers.para_gen_flags(["--bg_dir", "b", "--blur", "0.5"]).blur == (0.5, 9)
    assert helpers.para_gen_flags(["--bg_dir", "b", "--blur", "0.1", "32", "--multseg", "--bg_motion"]).blur == (float(F(0.1)), 32)
    import para_gen
    paths = para_gen.scan(flags, str(tmp_path / "nothing"), str(tmp_path / "out"))
    assert paths == []


def test_para_gen_refuses_blur(capsys):
    import helpers
    bg = ["--bg_dir", "b"]
    for extra in ([], bg + ["--mid", "2"], bg + ["--multseg", "--mid_layers", "2"], bg + ["--retex"],
                  bg + ["--bg_motion", "--mid", "2", "--mid_bg"], bg + ["--arap_bin", "/bin/true"]):
        with pytest.raises(SystemExit):
            helpers.para_gen_flags(["--blur", "0.5"] + extra)
        assert "--blur" in capsys.readouterr().err
    for blur in (["-1"], ["nan"], ["inf"], ["x"], ["0.5", "0"], ["0.5", "33"], ["0.5", "2.5"], ["0.5", "3", "4"]):
        with pytest.raises(SystemExit):
            helpers.para_gen_flags(bg + ["--blur"] + blur)
        assert "--blur" in capsys.readouterr().err
