"""CPU: the moving background over in-between frames (DESIGN.md "Moving background over in-between frames"): the numpy twin
tests/bg_seq_ref.py against a sequential per-pixel statement and against the pair twin, what the GPU tests' cases cover,
the `bg` line's mid= / mm= / mid_out= tokens in both grammars, pipeline.bg_maps_seq and mid_bg_files, para_gen's --mid_bg
flag and the library's export."""
import ctypes
import os.path as osp
import random
import subprocess

import numpy as np
import pytest

import bg_ref
import bg_seq_ref
import helpers
from arap_flow_amd import pipeline
from test_bg_host import _apply, _hidden, _sample, f32_maps

F = np.float32


def f32_G(Ma, Mb):
    return f32_maps(Ma, Mb)[0]


# ---- the definitions, pixel by pixel, every fmaf rounded exactly (test_bg_host's statements of sample, map and hidden) --
def sequential(bg, maps, Gs, mask_red, covers, rgbs, flows, occs):
    H, W = mask_red.shape
    m = len(maps)
    o = dict(out_rgb=[np.zeros((H, W, 3), np.uint8) for _ in range(m)], flow_full=[np.zeros((H, W, 2), F) for _ in range(m - 1)],
             occ_full=[np.zeros((H, W), np.uint8) for _ in range(m - 1)])
    for f in range(m):
        for y in range(H):
            for x in range(W):
                obj = mask_red[y, x] == 0 if f == 0 else covers[f][y, x] != 0
                o["out_rgb"][f][y, x] = rgbs[f][y, x] if obj else _sample(bg, *_apply(maps[f], x, y))
                if f == m - 1:
                    continue
                if obj:
                    o["flow_full"][f][y, x], o["occ_full"][f][y, x] = flows[f][y, x], occs[f][y, x]
                else:
                    p = _apply(Gs[f], x, y)
                    o["flow_full"][f][y, x] = (F(p[0] - F(x)), F(p[1] - F(y)))
                    o["occ_full"][f][y, x] = 255 if _hidden(p, covers[f + 1] != 0, W, H) else 0
    return o


def assert_same(got, want):
    assert set(got) == set(want) == set(bg_seq_ref.OUTPUTS)
    for k in want:
        assert len(got[k]) == len(want[k]), k
        for f, (a, b) in enumerate(zip(got[k], want[k])):
            assert (a is None) == (b is None), (k, f)
            if b is not None:
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (k, f)


def run_twin(c, maps, G=f32_G, **kw):
    return bg_seq_ref.background_seq(c["bg"], maps, bg_seq_ref.link_maps(maps, G), c["mask_red"], c["covers"], c["rgbs"],
                                     c["flows"], kw.get("occs", c["occs"]))


M1_SMALL = np.array([1, 0, 2, 0, 1, 2], F)


@pytest.mark.parametrize("kind", ["rotation", "leaves_frame", "leaves_bg"])
def test_twin_equals_sequential_statement(kind):
    W, H, m = 9, 6, 4
    c = bg_seq_ref.seq_case(W, H, 13, 10, m, seed=4)
    kw = dict(rotation=dict(deg=9.0, scale=1.05, shift=(0.6, -0.4)), leaves_frame=dict(deg=0.0, scale=1.0, shift=(7.5, 3.75)),
              leaves_bg=dict(deg=40.0, scale=3.0, shift=(-5.0, 2.0)))[kind]
    maps = bg_seq_ref.camera(M1_SMALL, m, W, H, **kw)
    Gs = bg_seq_ref.link_maps(maps, f32_G)
    assert_same(run_twin(c, maps), sequential(c["bg"], maps, Gs, c["mask_red"], c["covers"], c["rgbs"], c["flows"], c["occs"]))
    if kind == "leaves_frame":
        px, py = bg_ref.apply_map(Gs[1], W, H)
        assert ((px < 0) | (px > W - 1) | (py < 0) | (py > H - 1)).any()
    if kind == "leaves_bg":
        sx, sy = bg_ref.apply_map(maps[-1], W, H)
        assert ((sx < 0) | (sx > 12) | (sy < 0) | (sy > 9)).any()


def test_two_frames_are_the_pair_pass():
    """identity I1 in the twins: m = 2 gives bg_ref.background's out_rgb1, flow_full, occ_full, out_rgb2"""
    c = bg_seq_ref.seq_case(31, 11, 40, 20, 2, seed=2)
    maps = bg_seq_ref.camera(np.array([1, 0, 4, 0, 1, 5], F), 2, 31, 11)
    G, Ginv = f32_maps(maps[0], maps[1])
    got = run_twin(c, maps)
    want = bg_ref.background(c["bg"], maps[0], maps[1], G, Ginv, c["rgbs"][0], c["mask_red"], c["rgbs"][1], c["covers"][1],
                             c["flows"][0], c["occs"][0])
    assert_same(got, dict(out_rgb=[want["out_rgb1"], want["out_rgb2"]], flow_full=[want["flow_full"]],
                          occ_full=[want["occ_full"]]))


def test_a_still_camera_is_the_static_background():
    c = bg_seq_ref.seq_case(31, 11, 40, 20, 4, seed=3)
    maps = np.stack([np.array([1, 0, 4, 0, 1, 5], F)] * 4)
    got = run_twin(c, maps)
    win = c["bg"][5:5 + 11, 4:4 + 31]
    for f in range(4):
        obj = c["mask_red"] == 0 if f == 0 else c["covers"][f] != 0
        assert np.array_equal(got["out_rgb"][f], pipeline.add_bg(c["rgbs"][f], np.where(obj, 1, 0), win))
        if f == 3:
            break
        assert got["flow_full"][f].tobytes() == c["flows"][f].tobytes()           # zero off the object, as the input is
        assert (got["flow_full"][f][~obj] == 0).all()
        assert np.array_equal(got["occ_full"][f][~obj] == 255, (c["covers"][f + 1] != 0)[~obj])
        assert np.array_equal(got["occ_full"][f][obj], c["occs"][f][obj])


@pytest.mark.parametrize("size", list(bg_seq_ref.SIZES))
def test_gpu_cases_cover_every_branch_of_every_link(size):
    """what tests/test_gpu_background_seq.py runs: per link object and background pixels, and among the background ones a
    target that leaves the frame, one hidden by the next cover and a visible one -- in the twin's own outputs"""
    c = bg_seq_ref.sized_case(size)
    W, H, bw, bh, _, m = bg_seq_ref.SIZES[size]
    assert c["m"] == m == len(c["maps"]) and (W % 64 and H % 4)
    Gs = bg_seq_ref.link_maps(c["maps"])
    r = bg_seq_ref.background_seq(c["bg"], c["maps"], Gs, c["mask_red"], c["covers"], c["rgbs"], c["flows"], c["occs"])
    for f in range(m - 1):
        cov = bg_seq_ref.link_coverage(c, Gs, f)
        assert min(cov.values()) > 0, (f, cov)
        obj = c["mask_red"] == 0 if f == 0 else c["covers"][f] != 0
        assert obj.sum() == cov["object"] and not np.array_equal(c["covers"][f + 1] != 0, obj)
        occ_bg = r["occ_full"][f][~obj]
        assert (occ_bg == 255).sum() == cov["leaves"] + cov["covered"] and (occ_bg == 0).sum() == cov["visible"]
        assert np.abs(r["flow_full"][f][~obj]).max() > 0 and np.array_equal(r["flow_full"][f][obj], c["flows"][f][obj])
        assert not np.array_equal(c["maps"][f], c["maps"][f + 1])
        if f:
            assert not np.array_equal(c["covers"][f], c["covers"][f + 1]) and not np.array_equal(c["flows"][f], c["flows"][f - 1])


# ---- the line ----------------------------------------------------------------------------------------------------------
def _seq_item():
    M1 = np.array([1, 0, 17, 0, 1, 5], F)
    cams = [bg_ref.compose(M1, bg_ref.similarity(1.7 * t, 1.013 ** t, (2.3 * t, -0.71 * t), (47.5, 31.5))) for t in (4 / 19., 9 / 19., 1.0)]
    return pipeline.BgLine("/t/b.png", "/o/r1.png", "/o/m1.png", "/o/r2.png", "/o/m2.png", "/o/f.flo",
                           m=tuple(float(v) for v in np.concatenate([M1, cams[2]])), inputs=dict(occ="/o/occ.png"),
                           out=("", "/o/r2.png", "/o/ff.flo"), outs=dict(occ_out="/o/of.png"),
                           mid="4,9:/o/Mid/a/00000", mm=tuple(float(v) for v in np.concatenate(cams[:2])),
                           mid_out="/o/MidFull/a/00000"), cams


_BASE = "bg b r1 m1 r2 m2 f m=" + ",".join(["1"] * 12)
_MM12 = ",".join(["0.5"] * 12)
REFUSED = [
    _BASE + " out=a,b,c mid=4,9:P mm=" + ",".join(["1"] * 11) + " mid_out=Q",       # mm= whose count is not 6n
    _BASE + " out=a,b,c mid=4,9:P mm=" + ",".join(["1"] * 13) + " mid_out=Q",
    _BASE + " out=a,b,c mid=4:P mm=" + _MM12 + " mid_out=Q",
    _BASE + " out=a,b,c mid=4,9:P mm=" + ",".join(["x"] * 12) + " mid_out=Q",
    _BASE + " out=a,b,c mid=4,9:P mid_out=Q",                                       # mid= without mm=
    _BASE + " out=a,b,c mid=4,9:P mm=" + _MM12,                                     # mid= without mid_out=
    _BASE + " out=a,b,c mid_out=Q",                                                 # mid_out= without mid=
    _BASE + " out=a,b,c mm=" + _MM12 + " mid_out=Q",
    _BASE + " out=a,b,c mm=" + _MM12,
    _BASE + " out=a,b,c mid=9,4:P mm=" + _MM12 + " mid_out=Q",                      # parse_mid's own rules
    _BASE + " out=a,b,c mid=4,9 mm=" + _MM12 + " mid_out=Q",
    _BASE + " out=a,b,c mid=0:P mm=0,0,0,0,0,0 mid_out=Q",
]
ACCEPTED = [
    _BASE + " mid=4,9:P mm=" + _MM12 + " out=a,b,c mid_out=Q",
    _BASE + " mid_out=Q mm=" + _MM12 + " mid=4,9:P",                                # any order; the sequence alone is an output
    _BASE + " mid=4:P mm=1,0,2.5,0,1,-3.25 occ=O out=,b, occ_out=OO mid_out=Q",
    _BASE + " mid=1,2,3,4,5,6,7,8:P mm=" + ",".join(["0.25"] * 48) + " out=a,b,c mid_out=Q",
]


def test_bg_line_sequence_tokens_round_trip():
    item, cams = _seq_item()
    text = pipeline.format_line(item)
    back = pipeline.parse_line(text)
    assert back == item and isinstance(back, pipeline.BgLine) and pipeline.format_line(back) == text
    assert np.asarray(back.mm, F).tobytes() == np.concatenate(cams[:2]).tobytes()          # %.9g keeps the float32 bits
    assert np.asarray(back.m[6:], F).tobytes() == cams[2].tobytes()
    tok = text.split()
    assert tok[8] == "mid=4,9:/o/Mid/a/00000" and tok[9].startswith("mm=") and tok[-1] == "mid_out=/o/MidFull/a/00000"
    assert all(t == "%.9g" % v for t, v in zip(tok[9][3:].split(","), np.concatenate(cams[:2])))
    # the new files after the old ones; the done token is unchanged
    q = "/o/MidFull/a/00000"
    assert pipeline.bg_outputs(item) == ["/o/r2.png", "/o/ff.flo", "/o/of.png", q + "_s04.png", q + "_s09.png",
                                         q + "_s00_step.flo", q + "_s04_step.flo", q + "_s09_step.flo",
                                         q + "_s00_occ.png", q + "_s04_occ.png", q + "_s09_occ.png"]
    assert pipeline.done_token(item) == "/o/r2.png"
    no_occ = item._replace(inputs={}, outs={})
    assert pipeline.bg_outputs(no_occ) == ["/o/r2.png", "/o/ff.flo", q + "_s04.png", q + "_s09.png", q + "_s00_step.flo",
                                           q + "_s04_step.flo", q + "_s09_step.flo"]
    # a line without the tokens is the line it was
    old = item._replace(mid="", mm=(), mid_out="")
    assert "mid" not in pipeline.format_line(old) and pipeline.parse_line(pipeline.format_line(old)) == old
    assert old == pipeline.BgLine(*item[:6], m=item.m, inputs=item.inputs, out=item.out, outs=item.outs)
    for bad in REFUSED:
        with pytest.raises(ValueError):
            pipeline.parse_line(bad)
    for good in ACCEPTED:
        it = pipeline.parse_line(good)
        assert pipeline.parse_line(pipeline.format_line(it)) == it and len(it.mm) == 6 * len(pipeline.parse_mid(it.mid)[0])


def test_cpp_grammar_reads_the_same_lines():
    from arap_flow_amd import build
    tool = [b for b in build.build_host() if osp.basename(b) == "line_tool"][0]
    corpus = [pipeline.format_line(_seq_item()[0])] + ACCEPTED + REFUSED
    r = subprocess.run([tool], input="".join(c + "\n" for c in corpus), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = [ln for ln in r.stdout.split("\n")[:-1] if not ln.startswith("Invalid")]
    assert len(got) == len(corpus)
    for line, g in zip(corpus, got):
        if line in REFUSED:
            assert g == "BAD", line
        else:
            it = pipeline.parse_line(line)
            assert g == pipeline.format_line(it) + " done=" + pipeline.done_token(it), line


def test_mid_bg_files():
    assert pipeline.mid_bg_files("/o/MidFull/a/00007", 4) == dict(rgb="/o/MidFull/a/00007_s04.png",
                                                                   step="/o/MidFull/a/00007_s04_step.flo",
                                                                   occ="/o/MidFull/a/00007_s04_occ.png")
    assert pipeline.mid_bg_files("p", 0)["step"] == "p_s00_step.flo" and pipeline.mid_bg_files("p", 14)["occ"] == "p_s14_occ.png"
    # the names of the object-side files, under another prefix
    assert pipeline.mid_bg_files("p", 9)["rgb"] == pipeline.mid_files("p", 9)["rgb"]
    assert pipeline.mid_bg_files("p", 9)["step"] == pipeline.mid_files("p", 9)["step"]
    assert pipeline.mid_bg_files("p", 9)["occ"] == pipeline.mid_layer_files("p", 9)["occ"]


# ---- the cameras -------------------------------------------------------------------------------------------------------
def _corners_inside(M, wh, bwh):
    M = np.asarray(M, np.float64)
    return all(0 <= M[0] * x + M[1] * y + M[2] <= bwh[0] - 1 and 0 <= M[3] * x + M[4] * y + M[5] <= bwh[1] - 1
               for x in (0, wh[0] - 1) for y in (0, wh[1] - 1))


def test_bg_maps_seq_without_fractions_is_bg_maps():
    for seed in (0, 1, 7, 99, 12345):
        for args in ((5, 9, (96, 64), (140, 110)), (0, 0, (96, 64), (96, 64)), (2, 1, (96, 64), (100, 67))):
            for fd, strength in ((1, 1.0), (3, 2.5), (1, 0.0)):
                M1, M2 = pipeline.bg_maps(*args, random.Random(seed), fd, strength)
                r1, r2 = random.Random(seed), random.Random(seed)
                a, mids, b = pipeline.bg_maps_seq(*args, r1, (), fd, strength)
                assert mids == [] and a.tobytes() == M1.tobytes() and b.tobytes() == M2.tobytes() and a.dtype == b.dtype == F
                # the same four draws with in-between frames too
                pipeline.bg_maps_seq(*args, r2, (0.25, 0.5), fd, strength)
                assert r1.getstate() == r2.getstate()


def test_bg_maps_seq_interpolates_the_similarity():
    wh, bwh = (96, 64), (200, 160)
    fr = [i / 19.0 for i in (4, 9, 14)]
    for seed in (1, 7, 12345):
        M1, mids, M2 = pipeline.bg_maps_seq(40, 30, wh, bwh, random.Random(seed), fr, fd=2, strength=1.0)
        assert M1.tolist() == [1, 0, 40, 0, 1, 30] and len(mids) == 3 and all(m.dtype == F and m.shape == (6,) for m in mids)
        p1, p2 = pipeline.bg_maps(40, 30, wh, bwh, random.Random(seed), fd=2, strength=1.0)
        assert p1.tobytes() == M1.tobytes() and p2.tobytes() == M2.tobytes()       # nothing halved here: the pair's maps
        assert all(_corners_inside(M, wh, bwh) for M in [M1, M2] + mids)
        # rotation, log-scale and shift of M1^-1 o M grow in proportion to the fraction
        def params(M):
            S = bg_ref.maps_f64(M, M1)[0]
            c = np.array([47.5, 31.5])
            return np.array([np.arctan2(S[3], S[0]), np.log(np.hypot(S[0], S[3])),
                             *(S.reshape(2, 3)[:, :2] @ c + S.reshape(2, 3)[:, 2] - c)])
        full = params(M2)
        assert np.abs(full).max() > 0
        for t, M in zip(fr, mids):
            assert np.allclose(params(M), t * full, rtol=0, atol=2e-5)
            assert not np.array_equal(M, M1) and not np.array_equal(M, M2)
    # fraction 1 is M2, fraction 0 is M1, bit for bit
    M1, mids, M2 = pipeline.bg_maps_seq(40, 30, wh, bwh, random.Random(3), (0.0, 1.0), fd=1, strength=1.0)
    assert mids[0].tobytes() == M1.tobytes() and mids[1].tobytes() == M2.tobytes()


class _Draws:
    """a generator that hands out the given draws"""
    def __init__(self, values):
        self.values = list(values)

    def uniform(self, a, b):
        return self.values.pop(0)


def test_an_in_between_map_alone_forces_a_halving():
    """constructed: a rotation by -2 atan((H-1)/(W-1)) takes the corner (W-1, H-1) to (W-1, 0) -- inside again -- through the
    point furthest to the right, which a picture with a narrow margin in x does not hold"""
    wh, bwh, left, top = (96, 64), (96 + 6, 64 + 60), 3, 30
    rot = -2 * np.degrees(np.arctan2(63, 95))
    draws = (rot, 0.0, 0.0, 0.0)
    M1, M2 = pipeline.bg_maps(left, top, wh, bwh, _Draws(draws))
    assert not np.array_equal(M1, M2) and _corners_inside(M2, wh, bwh)
    S = bg_ref.maps_f64(M2, M1)[0]
    assert abs(np.degrees(np.arctan2(S[3], S[0])) - rot) < 1e-3                     # the pair alone keeps the full rotation
    a, mids, b = pipeline.bg_maps_seq(left, top, wh, bwh, _Draws(draws), (0.5,))
    half = bg_ref.compose(M1, bg_ref.similarity(rot / 2, 1.0, (0.0, 0.0), (47.5, 31.5)))
    assert not _corners_inside(half, wh, bwh)                                       # the frame half way leaves the picture
    assert a.tobytes() == M1.tobytes() and not np.array_equal(b, M2)               # so the sequence is halved, the pair was not
    assert all(_corners_inside(M, wh, bwh) for M in [a, b] + mids)
    S = bg_ref.maps_f64(b, a)[0]
    k = rot / np.degrees(np.arctan2(S[3], S[0]))
    assert abs(k - round(k)) < 1e-3 and round(k) in (2, 4, 8, 16, 32, 64, 128, 256)
    # nine failures: every map is M1
    a, mids, b = pipeline.bg_maps_seq(0, 0, (96, 64), (96, 64), _Draws((1.0, 0.0, 700.0, 0.0)), (0.25, 0.5))
    assert all(M.tobytes() == a.tobytes() for M in mids + [b]) and a.tolist() == [1, 0, 0, 0, 1, 0]


# ---- para_gen ----------------------------------------------------------------------------------------------------------
def test_para_gen_mid_bg_flags(capsys):
    bgm = ["--bg_dir", "bgs", "--bg_motion"]
    assert helpers.para_gen_flags([]).mid_bg is False
    fl = helpers.para_gen_flags(bgm + ["--mid", "2", "--mid_bg"])
    assert fl.mid_bg and fl.mid_steps == pipeline.mid_steps(2, 19) and fl.bg_motion == 1.0
    fl = helpers.para_gen_flags(bgm + ["--multseg", "--mid_layers", "3", "--occ_layers", "--mid_bg"])
    assert fl.mid_bg and fl.mid_layers_steps == pipeline.mid_steps(3, 19)
    # the bare combination is refused as before
    for extra in (["--mid", "2"], ["--multseg", "--mid_layers", "2"]):
        with pytest.raises(SystemExit):
            helpers.para_gen_flags(bgm + extra)
        err = capsys.readouterr().err
        assert ("--bg_motion cannot be combined with --mid / --mid_layers: the background motion of an in-between frame "
                "needs the motion interpolated per snapshot, which is not built") in " ".join(err.split())
    for args, msg in ((["--mid", "2", "--mid_bg", "--matches", "m"], "--mid_bg needs --bg_motion"),
                      (["--bg_dir", "bgs", "--mid", "2", "--mid_bg"], "--mid_bg needs --bg_motion"),
                      (bgm + ["--mid_bg"], "--mid_bg needs --mid K or --multseg --mid_layers K"),
                      (bgm + ["--mid", "2", "--occ", "--mid_bg"], "cannot be combined with --occ"),
                      (bgm + ["--mid_layers", "2", "--mid_bg"], "--mid_layers needs --multseg"),
                      (bgm + ["--multseg", "--mid", "2", "--mid_bg"], "--mid cannot be combined with --multseg")):
        with pytest.raises(SystemExit):
            helpers.para_gen_flags(args)
        assert msg in capsys.readouterr().err, args


def test_para_gen_lists_the_sequence_files(tmp_path):
    """scan: the MidFull files are part of a pair's outputs, in bg_outputs' order, and --resume asks for them"""
    import para_gen
    from PIL import Image
    inp = tmp_path / "in"
    for d in ("orgRGB", "orgMasks"):
        (inp / d / "a").mkdir(parents=True)
        for n in range(2):
            Image.fromarray(np.zeros((4, 4, 3), np.uint8)).save(inp / d / "a" / ("%05d.png" % n))
    flags = helpers.para_gen_flags(["--bg_dir", "bgs", "--bg_motion", "--multseg", "--mid_layers", "2", "--occ_layers", "--mid_bg"])
    (p,) = para_gen.scan(flags, str(inp), str(tmp_path / "out"))
    q = str(tmp_path / "out" / "MidFull" / "a" / "00000")
    assert p["midbg_gen"] == q and p["_midbg"] == (6, 12)
    want = [q + "_s06.png", q + "_s12.png"] + [q + "_s%02d_step.flo" % i for i in (0, 6, 12)] + [q + "_s%02d_occ.png" % i for i in (0, 6, 12)]
    assert para_gen.mid_bg_paths(p) == want
    item = pipeline.BgLine("b", "r1", "m1", "r2", "m2", "f", m=(0.0,) * 12, inputs=dict(occ="o"), out=("", "", ""), outs={},
                           mid="6,12:x", mm=(0.0,) * 12, mid_out=q)
    assert pipeline.bg_outputs(item) == want
    flags = helpers.para_gen_flags(["--bg_dir", "bgs", "--bg_motion", "--mid", "2", "--mid_bg"])
    (p,) = para_gen.scan(flags, str(inp), str(tmp_path / "out"))
    assert para_gen.mid_bg_paths(p) == want[:5]                                     # no link occlusion from a plain --mid run
    assert para_gen.mid_bg_paths({}) == []


def test_library_exports_the_sequence_pass():
    from arap_flow_amd import build, capi
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "ArapFlow_BackgroundSeq")
    assert "ArapFlow_BackgroundSeq" in {s[0] for s in capi.SYMBOLS}
    assert capi.MAX_SNAPSHOTS == pipeline.MAX_SNAPSHOTS == 8
    assert "ArapFlow_BackgroundSeq" in open(osp.join(osp.dirname(build.HERE), "include", "arap_opt.h")).read()
