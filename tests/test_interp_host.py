"""CPU: frames from flows (DESIGN.md "Frames from flows").  The numpy twin's anchors and its quality on a scene with true
flows; the `interp` list line in Python and in C++ (host/list_line.h through line_tool); the library's new entry points
and the argument sets they refuse without a device; frame_score_gen.py --from_flows with a stand-in worker."""
import ctypes as C
import os
import os.path as osp
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import fscore_ref
import interp_ref as R
from arap_flow_amd import capi, flo, pipeline

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
F = np.float32


# ---- the twin's anchors -------------------------------------------------------------------------------------------------------
def test_zero_flows_between_equal_frames_give_the_frame():
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, (9, 13, 3)).astype(np.uint8)
    z = np.zeros((9, 13, 2), F)
    times = [0.25, 0.5, 1 / 3, 0.999]
    for bwd in (None, z):
        out, src = R.interp_ref(a, a, z, times, bwd)
        assert out.shape == (4, 9, 13, 3) and (out == a[None]).all() and not src.any()


def test_invalid_flows_give_the_blend_baseline():
    rng = np.random.default_rng(2)
    a, b = (rng.integers(0, 256, (7, 40, 3)).astype(np.uint8) for _ in range(2))
    bad = np.full((7, 40, 2), 1e9, F)
    bad[::2, :, 0], bad[1::2, :, 1], bad[3] = np.nan, np.inf, -1e9
    blend = ((a.astype(np.uint16) + b + 1) >> 1).astype(np.uint8)          # frame_score_gen.write_blend
    for bwd in (None, bad):
        out, src = R.interp_ref(a, b, bad, [0.5], bwd)
        assert np.array_equal(out[0], blend) and (src == 255).all()
    out, _ = R.interp_ref(a, b, bad, [0.25])                                # any other time: 8-bit weights
    assert np.array_equal(out[0], ((192 * a.astype(np.int64) + 64 * b.astype(np.int64) + 128) >> 8).astype(np.uint8))


@pytest.mark.parametrize("d", [(3, 0), (-2, 1), (0, -4), (5, 2)])
def test_even_translation_at_half_time_shifts_by_half(d):
    rng = np.random.default_rng(3)
    H, W = 16, 31
    a = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    b = np.roll(a, (2 * d[1], 2 * d[0]), (0, 1))                            # b[y + 2dy][x + 2dx] = a[y][x], where inside
    fwd = np.broadcast_to(np.array([2 * d[0], 2 * d[1]], F), (H, W, 2))
    out, src = R.interp_ref(a, b, fwd, [0.5])
    ys, xs = np.mgrid[0:H, 0:W]
    ok = (xs - d[0] >= 0) & (xs - d[0] < W) & (xs + d[0] >= 0) & (xs + d[0] < W) & \
         (ys - d[1] >= 0) & (ys - d[1] < H) & (ys + d[1] >= 0) & (ys + d[1] < H)
    assert ok.sum() > 100
    assert np.array_equal(out[0][ok], a[ys[ok] - d[1], xs[ok] - d[0]]) and (src[0][ok] == 0).all()


# ---- quality: a textured square moves 19 px over a textured static background, true flows --------------------------------------
SQ, X0, Y0, SHIFT = 24, 9, 11, 19


def moving_square(W=96, H=48):
    """(frame(shift), fwd, bwd): the square's side is above the shift, so that a pixel the square covers at a time t is
    hidden in frame 1 or in frame 2 and no background pixel visible in both competes with it at cost 0"""
    rng = np.random.default_rng(5)
    ground = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    square = rng.integers(0, 256, (SQ, SQ, 3)).astype(np.uint8)

    def frame(shift):
        im = ground.copy()
        im[Y0:Y0 + SQ, X0 + shift:X0 + shift + SQ] = square
        return im
    fwd, bwd = np.zeros((H, W, 2), F), np.zeros((H, W, 2), F)
    fwd[Y0:Y0 + SQ, X0:X0 + SQ, 0] = SHIFT
    bwd[Y0:Y0 + SQ, X0 + SHIFT:X0 + SHIFT + SQ, 0] = -SHIFT
    return frame, fwd, bwd


def test_twin_beats_the_blend_and_is_exact_away_from_the_edge():
    frame, fwd, bwd = moving_square()
    a, b = frame(0), frame(SHIFT)
    H, W = a.shape[:2]
    steps = (4, 9)
    times = pipeline.interp_times(steps, 19)
    out, src = R.interp_ref(a, b, fwd, times, bwd)
    xs = np.arange(W)[None].repeat(H, 0)
    ys = np.arange(H)[:, None].repeat(W, 1)
    for k, step in enumerate(steps):
        truth = frame(step)
        tq = int(times[k] * F(256) + F(0.5))
        blend = (((256 - tq) * a.astype(np.int64) + tq * b.astype(np.int64) + 128) >> 8).astype(np.uint8)
        inside = (xs >= X0 + step) & (xs < X0 + step + SQ) & (ys >= Y0) & (ys < Y0 + SQ)
        in_a = (xs >= X0) & (xs < X0 + SQ) & (ys >= Y0) & (ys < Y0 + SQ)
        in_b = (xs >= X0 + SHIFT) & (xs < X0 + SHIFT + SQ) & (ys >= Y0) & (ys < Y0 + SQ)
        planes = dict(occ=((~inside & (in_a | in_b)) * 255).astype(np.uint8), obj=(~inside * 255).astype(np.uint8))
        mine = pipeline.frame_score_summary(fscore_ref.fscore_ref(truth, out[k], **planes)["table"][0])
        base = pipeline.frame_score_summary(fscore_ref.fscore_ref(truth, blend, **planes)["table"][0])
        populated = [r for r in pipeline.FSCORE_ROWS[:-1] if mine[r]["count"]]
        assert populated == ["all", "noc", "occ", "obj", "bg"]
        for r in populated:
            assert mine[r]["psnr"] > base[r]["psnr"], (step, r, mine[r]["psnr"], base[r]["psnr"])
        # more than 2 px from the square's edge at this time, in either direction
        dx = np.minimum(np.abs(xs - (X0 + step)), np.abs(xs - (X0 + step + SQ - 1)))
        dy = np.minimum(np.abs(ys - Y0), np.abs(ys - (Y0 + SQ - 1)))
        near = (np.minimum(dx, dy) <= 2) & (xs >= X0 + step - 3) & (xs < X0 + step + SQ + 3) & (ys >= Y0 - 3) & (ys < Y0 + SQ + 3)
        sure = (src[k] == 0) & ~near
        assert sure.sum() > 0.7 * W * H and np.array_equal(out[k][sure], truth[sure])
        assert set(np.unique(src[k])) >= {0, 1, 2}                      # the bands only one frame shows are found


# ---- the interp line: host/list_line.h against pipeline.parse_line ------------------------------------------------------------
_S = "interp a.png b.png f.flo"
GOOD = [
    _S + " s=4 n=19 out=P", _S + " s=4,9,14 n=19 out=P", _S + " out=P n=19 s=1,18", _S + " src=1 bwd=g.flo out=P n=2 s=1",
    _S + " s=4 n=19 bwd=a=b out=P", _S + " s=04,4294967294 n=4294967295 out=P", _S + " s=" + ",".join(str(i) for i in range(1, 33)) + " n=33 out=P",
    "interp inpRGB/a/00001.png wRGB/a/00001.png est/Flow/a/00001.flo s=4,9 n=19 bwd=est/FlowBwd/a/00001.flo out=FramesEst/Mid/a/00001",
]
BAD = [
    _S, _S + " s=4 n=19", _S + " s=4 out=P", _S + " n=19 out=P", "interp a.png b.png s=4 n=19 out=P", "interp",     # a missing part
    _S + " s=4 n=19 foo=X out=P", _S + " s=4 n=19 out=P mid=1", _S + " extra s=4 n=19 out=P",        # unknown keys, a stray word
    _S + " s=4 n=19 bwd= out=P", _S + " s=4 n=19 out=", _S + " s= n=19 out=P", _S + " s=4 n=19 src out=P",      # empty values, no `=`
    _S + " s=4 n=19 out=P out=Q", _S + " s=4 s=5 n=19 out=P", _S + " s=4 n=19 n=19 out=P", _S + " s=4 n=19 src=1 src=1 out=P",
    _S + " s=0 n=19 out=P", _S + " s=19 n=19 out=P", _S + " s=4,4 n=19 out=P", _S + " s=9,4 n=19 out=P", _S + " s=4,,9 n=19 out=P",
    _S + " s=4, n=19 out=P", _S + " s=+4 n=19 out=P", _S + " s=4.0 n=19 out=P", _S + " s=4 n=-19 out=P", _S + " s=4 n=1e2 out=P",
    _S + " s=1 n=1 out=P", _S + " s=1 n=0 out=P", _S + " s=4 n=4294967296 out=P", _S + " s=4 n=00000000019 out=P", _S + " s=4 n=19 src=0 out=P", _S + " s=4 n=19 src=yes out=P",
    _S + " s=" + ",".join(str(i) for i in range(1, 34)) + " n=40 out=P",                            # 33 steps
    "interp a=1 b.png f.flo s=4 n=19 out=P", "interp a.png b.png f=1 s=4 n=19 out=P",              # a token where a path is expected
]


@pytest.fixture(scope="module")
def bins():
    from arap_flow_amd import build
    return {osp.basename(o): o for o in build.build_host()}


def test_interp_line_round_trip():
    item = pipeline.InterpLine("a.png", "b.png", "f.flo", (4, 9), 19, "g.flo", True, "P")
    text = pipeline.format_line(item)
    assert text == "interp a.png b.png f.flo s=4,9 n=19 bwd=g.flo src=1 out=P" == pipeline.interp_line(item)
    back = pipeline.parse_line(text)
    assert isinstance(back, pipeline.InterpLine) and back == item
    assert pipeline.done_token(back) == "P" and pipeline.format_line(back) == text
    for line in GOOD:
        it = pipeline.parse_line(line)
        assert isinstance(it, pipeline.InterpLine) and pipeline.parse_line(pipeline.format_line(it)) == it
        assert pipeline.parse_interp(line.split()) == it
    assert pipeline.parse_line(GOOD[0]) == pipeline.InterpLine("a.png", "b.png", "f.flo", (4,), 19, "", False, "P")
    assert pipeline.parse_line(GOOD[4]).bwd == "a=b"                                               # the first `=` splits
    assert pipeline.INTERP_WORD == "interp" and pipeline.INTERP_MAX_TIMES == 32 and len(pipeline.parse_line(GOOD[6]).steps) == 32
    assert pipeline.interp_files("P", 4) == dict(rgb="P_s04.png", src="P_s04_src.png") and pipeline.mid_files("P", 4)["rgb"] == "P_s04.png"
    t = pipeline.interp_times((4, 9), 19)
    assert t.dtype == np.float32 and t[0] == F(4) / F(19) and t[1] == F(9) / F(19)
    for line in BAD:
        with pytest.raises(ValueError):
            pipeline.parse_line(line)


def test_interp_line_parser_equals_python_twin(bins):
    """every line through line_tool in one process: a good one comes back as format_line(parse_line(line)) + its done
    token, a bad one as BAD after the grammar's own message -- and Python refuses exactly those"""
    corpus = GOOD + BAD
    r = subprocess.run([bins["line_tool"]], input="".join(c + "\n" for c in corpus), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")[:-1]
    got = [ln for ln in lines if not ln.startswith("Invalid")]
    assert len(got) == len(corpus)
    assert [ln for ln in lines if ln.startswith("Invalid")] == ["Invalid interp line: " + b for b in BAD]
    for line, g in zip(GOOD, got):
        item = pipeline.parse_line(line)
        assert g == pipeline.format_line(item) + " done=" + pipeline.done_token(item), line
    assert got[0] == _S + " s=4 n=19 out=P done=P"
    assert got[len(GOOD):] == ["BAD"] * len(BAD)


def test_arap_deform_refuses_a_bad_interp_line_before_any_gpu_call(bins, tmp_path):
    lst = tmp_path / "l.txt"
    lst.write_text("a b c d e f\n" + BAD[18] + "\n")
    r = subprocess.run([bins["arap_deform"], str(lst)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "Invalid interp line: " + BAD[18] + "\n"
    r = subprocess.run([sys.executable, osp.join(ROOT, "arap_deform.py"), str(lst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "interp line" in r.stdout


# ---- the library's new entry points -----------------------------------------------------------------------------------------
def test_new_entry_points_exported_and_refusals_without_a_device():
    lib = capi.load()
    names = [s[0] for s in capi.SYMBOLS]
    for name in ("ArapFlow_InterpFrames", "ArapFlow_InterpScratchBytes"):
        assert name in names and hasattr(lib, name)
    header = open(osp.join(ROOT, "include", "arap_opt.h")).read()
    for text in ("#define ARAPFLOW_INTERP_MAX_TIMES 32", "#define ARAPFLOW_INTERP_FILL 16",
                 "uint64_t ArapFlow_InterpScratchBytes(unsigned W, unsigned H, unsigned K);",
                 "int ArapFlow_InterpFrames(Opt_State* state, unsigned W, unsigned H, const void* A, const void* B, const void* fwd,\n"
                 "                          const void* bwd, unsigned K, const float* times, void* out, void* src, void* scratch);"):
        assert text in header
    assert (capi.INTERP_MAX_TIMES, capi.INTERP_FILL) == (32, 16) == (R.MAX_TIMES, R.FILL) and pipeline.INTERP_MAX_TIMES == 32
    sb = lib.ArapFlow_InterpScratchBytes
    assert sb(4, 4, 1) == 256 and sb(4, 4, 3) == 512 and sb(854, 480, 32) == 854 * 480 * 32 * 8 and sb(5, 7, 2) == 768
    assert sb(0, 4, 1) == 0 and sb(4, 0, 1) == 0 and sb(4, 4, 0) == 0 and sb(4, 4, 33) == 0
    assert sb(1 << 16, 1 << 15, 1) == 0 and sb(1 << 15, 1 << 15, 2) == 0 and sb(0xffffffff, 0xffffffff, 32) == 0
    # refused before anything is read or launched: a stand-in for the state and the buffers is never dereferenced
    mem = C.create_string_buffer(1 << 14)
    p = C.c_void_p(C.addressof(mem))
    at = lambda off: C.c_void_p(C.addressof(mem) + off)
    times = lambda *v: (C.c_float * len(v))(*v)
    fn = lib.ArapFlow_InterpFrames
    # W, H = 4, 4, K = 2: A, B 48 bytes, fwd, bwd 128, out 96, src 32, scratch 256
    ok = [p, 4, 4, at(0), at(256), at(512), at(1024), 2, times(0.25, 0.5), at(2048), at(3072), at(4096)]
    for k in (0, 3, 4, 5, 8, 9, 11):                            # a null state, A, B, fwd, times, out or scratch
        a = list(ok)
        a[k] = None
        assert fn(*a) == -1, k
    nan, inf = float("nan"), float("inf")
    for k, v in ((1, 0), (2, 0), (7, 0), (7, 33), (7, 0xffffffff),
                 (8, times(0.25, 0.0)), (8, times(1.0, 0.5)), (8, times(0.5, nan)), (8, times(inf, 0.5)), (8, times(-0.5, 0.5)),
                 (8, times(0.5, -inf)), (8, times(0.5, 1.5)),
                 (9, at(0)), (9, at(47)), (9, at(256 - 95)), (9, at(512 + 127)), (9, at(1024 + 8)),     # out on A, B, fwd, bwd
                 (10, at(40)), (10, at(256 + 47)), (10, at(512 - 31)), (10, at(1024 + 127)),           # src on the inputs
                 (10, at(2048 + 95)), (10, at(2048 - 31)),                                             # src on out
                 (11, at(48 - 255)), (11, at(256)), (11, at(512 + 64)), (11, at(1024 - 255)),          # scratch on the inputs
                 (11, at(2048 - 255)), (11, at(2048 + 95)), (11, at(3072 + 31)), (11, at(3072 - 255))):    # on out, on src
        a = list(ok)
        a[k] = v
        assert fn(*a) == -1, (k, v)
    big = [p, 1 << 16, 1 << 15, at(0), at(256), at(512), None, 1, times(0.5), at(2048), None, at(4096)]
    assert fn(*big) == -1                                       # W * H = 2^31
    big[1], big[7], big[8] = 1 << 15, 2, times(0.5, 0.75)
    assert fn(*big) == -1                                       # K * W * H = 2^31
    big[1], big[2], big[7], big[8] = 0xffffffff, 0xffffffff, 32, times(*([0.5] * 32))
    assert fn(*big) == -1
    assert not any(mem.raw)


# ---- frame_score_gen.py --from_flows ----------------------------------------------------------------------------------------
FAKE_WORKER = r'''
import sys
# stand-in for arap_deform --serve (no GPU): an interp line's frames and an fscore line's table come from the numpy twins
import numpy as np
from PIL import Image
sys.path.insert(0, %r); sys.path.insert(0, %r)
import fscore_ref, interp_ref
from arap_flow_amd import flo, pipeline
def run(line):
    it = pipeline.parse_line(line)
    if isinstance(it, pipeline.InterpLine):
        bwd = flo.flow_read(it.bwd) if it.bwd else None
        out, src = interp_ref.interp_ref(pipeline.load_rgb(it.a), pipeline.load_rgb(it.b), flo.flow_read(it.fwd),
                                         pipeline.interp_times(it.steps, it.n), bwd)
        for k, i in enumerate(it.steps):
            Image.fromarray(out[k]).save(pipeline.interp_files(it.out, i)["rgb"])
    else:
        planes = {k: pipeline.load_mask_red(p) for k, p in it.planes.items()}
        t = fscore_ref.fscore_ref(pipeline.load_rgb(it.ref), pipeline.load_rgb(it.est), **planes)["table"][0]
        open(it.out, "w").write(pipeline.format_frame_score(t))
    with open(%r, "a") as log:
        log.write(line)
print("Ready", flush=True)
for line in sys.stdin:
    run(line)
    print("Done " + pipeline.done_token(pipeline.parse_line(line)), flush=True)
'''


def make_tree(out, full):
    """a dataset tree: sequence `a` with pair 00000 (in-between frames 4 and 9, forward and backward flow) and pair 00001
    (one in-between frame, no flow), sequence `b` with pair 00000 (in-between frame 14, forward flow only)"""
    frame, fwd, bwd = moving_square(64, 40)
    mid = "MidFull" if full else "Mid"
    flow, back = ("FlowFull", "FlowBwdFull") if full else ("Flow", "FlowBwd")
    for seq, stem, steps, has in (("a", "00000", (4, 9), (True, True)), ("a", "00001", (9,), (False, False)), ("b", "00000", (14,), (True, False))):
        for d in ("inpRGB", "wRGB", mid, flow, back):
            os.makedirs(out / d / seq, exist_ok=True)
        Image.fromarray(frame(0)).save(out / "inpRGB" / seq / (stem + ".png"))
        Image.fromarray(frame(SHIFT)).save(out / "wRGB" / seq / (stem + ".png"))
        for i in steps:
            Image.fromarray(frame(i)).save(out / mid / seq / ("%s_s%02d.png" % (stem, i)))
            Image.fromarray(np.zeros((40, 64), np.uint8), "L").save(out / mid / seq / ("%s_s%02d_mask.png" % (stem, i)))    # no frame
        if has[0]:
            flo.flow_write(str(out / flow / seq / (stem + ".flo")), fwd)
        if has[1]:
            flo.flow_write(str(out / back / seq / (stem + ".flo")), bwd)
    return frame, fwd, bwd


@pytest.mark.parametrize("full", [False, True], ids=["objects", "full"])
def test_frame_score_gen_from_flows_with_a_stand_in_worker(tmp_path, full, capsys):
    sys.path.insert(0, ROOT)
    import frame_score_gen
    out = tmp_path / "out"
    frame, fwd, bwd = make_tree(out, full)
    mid = "MidFull" if full else "Mid"
    stale = out / "FramesEst" / mid / "a" / "00001_s09.png"     # an earlier run's file is no estimate of a pair without a flow
    os.makedirs(stale.parent)
    Image.fromarray(frame(9)).save(stale)
    fake, log = tmp_path / "fake.py", tmp_path / "lines.log"
    fake.write_text(FAKE_WORKER % (ROOT, osp.join(ROOT, "tests"), str(log)))
    own = "%s %s" % (sys.executable, osp.join(ROOT, "arap_deform.py"))
    flags = frame_score_gen.parse(["--data", str(out), "--est", str(out), "--from_flows", "--arap_bin", own, "--worker", "serve"] +
                                  (["--full"] if full else []))
    assert flags.from_flows and flags.baseline is None
    flags.arap_bin = "%s %s" % (sys.executable, fake)               # (the flags are checked against this repository's driver)
    pooled = frame_score_gen.main(flags)
    lines = [pipeline.parse_line(ln) for ln in log.read_text().splitlines()]
    interp = [it for it in lines if isinstance(it, pipeline.InterpLine)]
    flow, back = ("FlowFull", "FlowBwdFull") if full else ("Flow", "FlowBwd")
    p = lambda *parts: str(out.joinpath(*parts))
    assert sorted(interp) == [
        pipeline.InterpLine(p("inpRGB", "a", "00000.png"), p("wRGB", "a", "00000.png"), p(flow, "a", "00000.flo"), (4, 9), 19,
                            p(back, "a", "00000.flo"), False, p("FramesEst", mid, "a", "00000")),
        pipeline.InterpLine(p("inpRGB", "b", "00000.png"), p("wRGB", "b", "00000.png"), p(flow, "b", "00000.flo"), (14,), 19,
                            "", False, p("FramesEst", mid, "b", "00000"))]
    scored = [it for it in lines if isinstance(it, pipeline.FScoreLine)]
    assert len(scored) == 3 and len(lines) == 5
    for it in scored:                                               # a frame is scored after the line that writes it
        prefix = it.est[:-len("_s04.png")]
        assert [k for k, ln in enumerate(lines) if isinstance(ln, pipeline.InterpLine) and ln.out == prefix][0] < lines.index(it)
    a, b = frame(0), frame(SHIFT)
    tables = []
    for seq, steps, bw in (("a", (4, 9), bwd), ("b", (14,), None)):
        want, _ = R.interp_ref(a, b, fwd, pipeline.interp_times(steps, 19), bw)
        for k, i in enumerate(steps):
            name = "00000_s%02d" % i
            assert np.array_equal(np.array(Image.open(out / "FramesEst" / mid / seq / (name + ".png"))), want[k])
            t = fscore_ref.fscore_ref(frame(i), want[k])["table"][0]
            assert (out / "FrameScore" / seq / (name + ".txt")).read_text() == pipeline.format_frame_score(t)
            tables.append(t)
    assert np.array_equal(pooled, pipeline.add_frame_scores(tables))
    assert (out / "frame_score.txt").read_text() == pipeline.format_frame_score(pooled)
    missing = [p(mid, "a", "00001_s09.png")] + ([] if full else [p("wRGB", s, n + ".png") for s, n in (("a", "00000"), ("a", "00001"), ("b", "00000"))])
    assert (out / "frame_score_missing.list").read_text() == "".join(m + "\n" for m in missing)
    assert not (out / "FrameScore" / "a" / "00001_s09.txt").exists()
    printed = capsys.readouterr().out
    assert "3 frames scored, %d without an estimate" % len(missing) in printed


def test_frame_score_gen_parse_from_flows():
    sys.path.insert(0, ROOT)
    import frame_score_gen
    flags = frame_score_gen.parse(["--data", "D", "--est", "E"])
    assert flags.from_flows is False
    flags = frame_score_gen.parse(["--data", "D", "--est", "E", "--from_flows", "--full"])
    assert flags.from_flows and flags.full
    for argv in (["--data", "D", "--from_flows"], ["--data", "D", "--from_flows", "--baseline", "blend"],
                 ["--data", "D", "--est", "E", "--from_flows", "--baseline", "blend"]):
        with pytest.raises(SystemExit):
            frame_score_gen.parse(argv)
