"""CPU: the moving background's definitions (DESIGN.md "Moving background") in the numpy twin tests/bg_ref.py, the `bg`
list line, pipeline.bg_maps, para_gen's --bg_motion flag and the library's exports."""
import ctypes
import random
from fractions import Fraction

import numpy as np
import pytest

import bg_ref
import helpers
from arap_flow_amd import pipeline

F = np.float32


# ---- a sequential per-pixel statement of the definitions, every fmaf rounded exactly -----------------------------------
def _round_f32(q):
    """the float32 nearest to the Fraction q, ties to even"""
    c = F(float(q))
    best = None
    for cand in (np.nextafter(c, F(-np.inf)), c, np.nextafter(c, F(np.inf))):
        if not np.isfinite(cand):
            continue
        d = abs(Fraction(float(cand)) - q)
        even = int(np.asarray(cand, F).view(np.uint32)) % 2 == 0
        if best is None or d < best[0] or (d == best[0] and even and not best[2]):
            best = (d, cand, even)
    return best[1]


def _fmaf(a, b, c):
    return _round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _apply(m, x, y):
    fx, fy = F(x), F(y)
    return _fmaf(m[0], fx, _fmaf(m[1], fy, m[2])), _fmaf(m[3], fx, _fmaf(m[4], fy, m[5]))


def _sample(bg, bx, by):
    bh, bw = bg.shape[:2]
    bx = min(max(bx, F(0)), F(bw - 1))
    by = min(max(by, F(0)), F(bh - 1))
    x0, y0 = int(np.floor(bx)), int(np.floor(by))
    x1, y1 = min(x0 + 1, bw - 1), min(y0 + 1, bh - 1)
    fx, fy = F(bx - F(x0)), F(by - F(y0))
    out = []
    for c in range(3):
        c00, c01, c10, c11 = (F(bg[y0, x0, c]), F(bg[y0, x1, c]), F(bg[y1, x0, c]), F(bg[y1, x1, c]))
        top, bot = _fmaf(fx, F(c01 - c00), c00), _fmaf(fx, F(c11 - c10), c10)
        v = _fmaf(fy, F(bot - top), top)
        out.append(int(F(v + F(0.5))))
    return out


def _hidden(p, hides, W, H):
    if not (p[0] >= 0 and p[0] <= W - 1 and p[1] >= 0 and p[1] <= H - 1):
        return True
    return bool(hides[int(np.floor(F(p[1] + F(0.5)))), int(np.floor(F(p[0] + F(0.5))))])


def sequential(bg, M1, M2, G, Ginv, rgb1, mask_red, rgb2, cover2, flow, occ, bwd, occ_bwd):
    H, W = mask_red.shape
    o = dict(out_rgb1=np.zeros((H, W, 3), np.uint8), out_rgb2=np.zeros((H, W, 3), np.uint8),
             flow_full=np.zeros((H, W, 2), F), occ_full=np.zeros((H, W), np.uint8),
             bwd_full=np.zeros((H, W, 2), F), occ_bwd_full=np.zeros((H, W), np.uint8))
    for y in range(H):
        for x in range(W):
            if mask_red[y, x] == 0:
                o["out_rgb1"][y, x], o["flow_full"][y, x], o["occ_full"][y, x] = rgb1[y, x], flow[y, x], occ[y, x]
            else:
                o["out_rgb1"][y, x] = _sample(bg, *_apply(M1, x, y))
                p = _apply(G, x, y)
                o["flow_full"][y, x] = (F(p[0] - F(x)), F(p[1] - F(y)))
                o["occ_full"][y, x] = 255 if _hidden(p, cover2 != 0, W, H) else 0
            if cover2[y, x] != 0:
                o["out_rgb2"][y, x], o["bwd_full"][y, x], o["occ_bwd_full"][y, x] = rgb2[y, x], bwd[y, x], occ_bwd[y, x]
            else:
                o["out_rgb2"][y, x] = _sample(bg, *_apply(M2, x, y))
                p = _apply(Ginv, x, y)
                o["bwd_full"][y, x] = (F(p[0] - F(x)), F(p[1] - F(y)))
                o["occ_bwd_full"][y, x] = 255 if _hidden(p, mask_red == 0, W, H) else 0
    return o


def small_case(W=7, H=5, bw=11, bh=9, seed=3):
    rng = np.random.default_rng(seed)
    c = dict(bg=rng.integers(0, 256, (bh, bw, 3)).astype(np.uint8), rgb1=rng.integers(0, 256, (H, W, 3)).astype(np.uint8),
             rgb2=rng.integers(0, 256, (H, W, 3)).astype(np.uint8))
    c["mask_red"] = np.full((H, W), 255, np.uint8)
    c["mask_red"][1:4, 2:5] = 0
    c["cover2"] = np.zeros((H, W), np.uint8)
    c["cover2"][1:4, 3:6] = 255
    c["flow"] = np.where((c["mask_red"] == 0)[..., None], np.array([1, 0], F), F(0))       # (+0 off the object, as the
    c["bwd"] = np.where((c["cover2"] != 0)[..., None], np.array([-1, 0], F), F(0))          # warp writes it)
    c["occ"] = np.where((c["mask_red"] != 0) & (c["cover2"] != 0), 255, 0).astype(np.uint8)
    c["occ_bwd"] = np.where((c["mask_red"] == 0) & (c["cover2"] == 0), 255, 0).astype(np.uint8)
    return c


def f32_maps(M1, M2):
    """the point maps for the CPU tests: the float64 statement rounded once (bit-equal maps: the identity)"""
    if np.array_equal(np.asarray(M1, F), np.asarray(M2, F)):
        return bg_ref.IDENTITY, bg_ref.IDENTITY
    g, gi = bg_ref.maps_f64(M1, M2)
    return g.astype(F), gi.astype(F)


M1_SMALL = np.array([1, 0, 2, 0, 1, 2], F)


@pytest.mark.parametrize("M2", [
    bg_ref.compose(M1_SMALL, bg_ref.similarity(5.0, 1.03, (0.4, -0.3), (3.0, 2.0))),        # a rotation
    bg_ref.compose(M1_SMALL, bg_ref.similarity(0.0, 1.0, (4.5, 2.25), (3.0, 2.0))),         # targets leave the frame
    bg_ref.compose(M1_SMALL, bg_ref.similarity(20.0, 2.5, (-3.0, 1.0), (3.0, 2.0))),        # samples leave bg
], ids=["rotation", "leaves_frame", "leaves_bg"])
def test_twin_equals_sequential_statement(M2):
    c = small_case()
    G, Ginv = f32_maps(M1_SMALL, M2)
    got = bg_ref.background(c["bg"], M1_SMALL, M2, G, Ginv, c["rgb1"], c["mask_red"], c["rgb2"], c["cover2"], c["flow"],
                            c["occ"], c["bwd"], c["occ_bwd"])
    want = sequential(c["bg"], M1_SMALL, M2, G, Ginv, c["rgb1"], c["mask_red"], c["rgb2"], c["cover2"], c["flow"],
                      c["occ"], c["bwd"], c["occ_bwd"])
    assert set(got) == set(bg_ref.OUTPUTS)
    for k in bg_ref.OUTPUTS:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k


def test_cases_leave_frame_and_bg():
    M2f = bg_ref.compose(M1_SMALL, bg_ref.similarity(0.0, 1.0, (4.5, 2.25), (3.0, 2.0)))
    px, py = bg_ref.apply_map(f32_maps(M1_SMALL, M2f)[0], 7, 5)
    assert ((px < 0) | (px > 6) | (py < 0) | (py > 4)).any()
    M2b = bg_ref.compose(M1_SMALL, bg_ref.similarity(20.0, 2.5, (-3.0, 1.0), (3.0, 2.0)))
    sx, sy = bg_ref.apply_map(M2b, 7, 5)
    assert ((sx < 0) | (sx > 10) | (sy < 0) | (sy > 8)).any()


def test_identity_and_translation_consequences():
    c = small_case()
    M = np.array([1, 0, 3, 0, 1, 2], F)
    G, Ginv = f32_maps(M, M)
    r = bg_ref.background(c["bg"], M, M, G, Ginv, c["rgb1"], c["mask_red"], c["rgb2"], c["cover2"], c["flow"], c["occ"],
                          c["bwd"], c["occ_bwd"])
    # every full map is the object-side map (DESIGN "Backward flow and occlusion" items 1-3)
    assert r["flow_full"].tobytes() == c["flow"].tobytes() and r["bwd_full"].tobytes() == c["bwd"].tobytes()
    assert np.array_equal(r["occ_full"], c["occ"]) and np.array_equal(r["occ_bwd_full"], c["occ_bwd"])
    obj1, obj2 = c["mask_red"] == 0, c["cover2"] != 0
    assert (r["flow_full"][~obj1] == 0).all()
    assert np.array_equal(r["occ_full"][~obj1] == 255, obj2[~obj1])
    assert np.array_equal(r["occ_bwd_full"] == 255, ~obj2 & obj1)
    # an integer translation: pipeline.add_bg with the window, byte for byte
    win = c["bg"][2:2 + 5, 3:3 + 7]
    assert np.array_equal(r["out_rgb1"], pipeline.add_bg(c["rgb1"], np.where(obj1, 1, 0), win))
    assert np.array_equal(r["out_rgb2"], pipeline.add_bg(c["rgb2"], c["cover2"], win))
    # the sample at an integer point is the pixel itself, also on the last row and column
    ys, xs = np.mgrid[0:9, 0:11]
    assert np.array_equal(bg_ref.sample(c["bg"], xs.astype(F), ys.astype(F)), c["bg"])


def test_bg_line_round_trip():
    m = np.concatenate([np.array([1, 0, 17, 0, 1, 5], F), bg_ref.similarity(1.7, 1.013, (2.3, -0.71), (47.5, 31.5))])
    item = pipeline.BgLine("/t/b.png", "/o/r1.png", "/o/m1.png", "/o/r2.png", "/o/m2.png", "/o/f.flo",
                           m=tuple(float(v) for v in m), inputs=dict(occ="/o/occ.png", bwd="/o/b.flo", occ_bwd="/o/ob.png"),
                           out=("", "/o/r2.png", "/o/ff.flo"),
                           outs=dict(occ_out="/o/of.png", bwd_out="/o/bf.flo", occ_bwd_out="/o/obf.png"))
    text = pipeline.format_line(item)
    assert text.split()[0] == "bg" and " out=,/o/r2.png,/o/ff.flo " in text
    back = pipeline.parse_line(text)
    assert back == item and isinstance(back, pipeline.BgLine)
    assert np.asarray(back.m, F).tobytes() == m.tobytes()                  # %.9g keeps the float32 bits
    assert all(t == "%.9g" % v for t, v in zip(text.split()[7][2:].split(","), m))
    assert pipeline.done_token(item) == "/o/r2.png"
    assert pipeline.bg_outputs(item) == ["/o/r2.png", "/o/ff.flo", "/o/of.png", "/o/bf.flo", "/o/obf.png"]
    only = item._replace(inputs={}, outs={}, out=("/o/a.png", "", ""))
    assert pipeline.parse_line(pipeline.format_line(only)) == only and pipeline.done_token(only) == "/o/a.png"
    base = "bg b r1 m1 r2 m2 f m=" + ",".join(["1"] * 12)
    for bad in ("bg b r1 m1 r2 m2 f out=a,b,c",                            # no maps
                base,                                                      # no output
                base + " out=a,b", base + " out=a,b,c,d",                  # out= takes three places
                "bg b r1 m1 r2 m2 f m=1,2,3 out=a,b,c",                    # twelve numbers
                "bg b r1 m1 r2 m2 f m=" + ",".join(["x"] * 12) + " out=a,b,c",
                base + " out=a,b,c occ_out=o",                             # an output without its input
                base + " out=a,b,c rgb9=o", base + " out=a,b,c junk",
                "bg b r1 m1 r2 m2"):
        with pytest.raises(ValueError):
            pipeline.parse_line(bad)
    # the other forms still parse as themselves
    assert isinstance(pipeline.parse_line("a b c d e f"), pipeline.SolveLine)
    assert isinstance(pipeline.parse_line("layers r 1 m f occ=o"), pipeline.LayersLine)


def test_bg_maps_window_and_corner_rule():
    rng_bg = np.random.default_rng(0)
    bg = rng_bg.integers(0, 256, (90, 140, 3)).astype(np.uint8)
    im = np.zeros((64, 96, 3), np.uint8)
    for seed in (1, 7, 12345):
        window = pipeline.fit_bg(bg, im, rng=random.Random(seed))
        rng = random.Random(seed)
        big, (left, top) = pipeline.fit_bg_window(bg, im, rng=rng)
        assert np.array_equal(big[top:top + 64, left:left + 96], window)       # the window of a run without the motion
        M1, M2 = pipeline.bg_maps(left, top, (96, 64), (big.shape[1], big.shape[0]), rng, fd=2, strength=1.0)
        assert M1.dtype == M2.dtype == F and M1.tolist() == [1, 0, left, 0, 1, top]
        # the similarity's parameters are within strength x fd x (2 deg, 0.01, 3 px)
        S = bg_ref.maps_f64(M2, M1)[0]                                          # M1^-1 o M2
        assert abs(np.degrees(np.arctan2(S[3], S[0]))) <= 4 + 1e-3
        assert abs(np.log(np.hypot(S[0], S[3]))) <= 0.02 + 1e-5
        c = np.array([47.5, 31.5])
        shift = S.reshape(2, 3)[:, :2] @ c + S.reshape(2, 3)[:, 2] - c
        assert np.abs(shift).max() <= 6 + 1e-3
        for x in (0, 95):
            for y in (0, 63):
                px, py = M2[0] * x + M2[1] * y + M2[2], M2[3] * x + M2[4] * y + M2[5]
                assert 0 <= px <= big.shape[1] - 1 and 0 <= py <= big.shape[0] - 1
    # a window that fills the picture: only M2 = M1 keeps every corner inside -- unless the draw happens to fit
    for seed in range(6):
        M1, M2 = pipeline.bg_maps(0, 0, (96, 64), (96, 64), random.Random(seed), fd=1, strength=1.0)
        for x in (0, 95):
            for y in (0, 63):
                px, py = M2[0] * x + M2[1] * y + M2[2], M2[3] * x + M2[4] * y + M2[5]
                assert 0 <= px <= 95 and 0 <= py <= 63
    # strength 0 draws (the generator's state moves on as for any strength) but does not move
    M1, M2 = pipeline.bg_maps(3, 4, (96, 64), (200, 200), random.Random(5), fd=1, strength=0.0)
    assert np.array_equal(M1, M2)


def test_para_gen_bg_motion_flags(capsys):
    assert helpers.para_gen_flags([]).bg_motion is None
    assert helpers.para_gen_flags(["--bg_dir", "bgs", "--bg_motion"]).bg_motion == 1.0
    assert helpers.para_gen_flags(["--bg_dir", "bgs", "--bg_motion", "0.5"]).bg_motion == 0.5
    with pytest.raises(SystemExit):
        helpers.para_gen_flags(["--bg_motion"])
    assert "--bg_motion needs --bg_dir" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        helpers.para_gen_flags(["--bg_dir", "bgs", "--bg_motion", "--mid", "2"])
    assert "--bg_motion cannot be combined with --mid" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        helpers.para_gen_flags(["--bg_dir", "bgs", "--bg_motion", "--multseg", "--mid_layers", "2"])
    assert "--bg_motion cannot be combined with --mid" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        helpers.para_gen_flags(["--bg_dir", "bgs", "--bg_motion", "--arap_bin", "/bin/true"])
    assert "bg line" in capsys.readouterr().err


def test_new_entry_points_exported_and_maps_on_the_host():
    from arap_flow_amd import build, capi
    lib = ctypes.CDLL(build.build())
    for name in ("ArapFlow_BackgroundMaps", "ArapFlow_Background"):
        assert hasattr(lib, name), name
        assert name in {s[0] for s in capi.SYMBOLS}
    fn = lib.ArapFlow_BackgroundMaps
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.POINTER(ctypes.c_float)] * 4
    arr = lambda m: (ctypes.c_float * 6)(*[float(v) for v in m])
    M1 = np.array([1, 0, 6, 0, 1, 7], F)
    M2 = bg_ref.compose(M1, bg_ref.similarity(3.0, 1.02, (2.5, -1.25), (33.0, 4.0)))
    g, gi = (ctypes.c_float * 6)(), (ctypes.c_float * 6)()
    assert fn(arr(M1), arr(M2), g, gi) == 0
    want_g, want_gi = bg_ref.maps_f64(M1, M2)
    assert np.allclose(np.array(g[:]), want_g, rtol=1e-6, atol=1e-6 * np.abs(want_g).max())
    assert np.allclose(np.array(gi[:]), want_gi, rtol=1e-6, atol=1e-6 * np.abs(want_gi).max())
    assert fn(arr(M2), arr(M2), g, gi) == 0 and g[:] == gi[:] == [1, 0, 0, 0, 1, 0]
    for bad in ([1, 2, 0, 2, 4, 0], [np.nan, 0, 0, 0, 1, 0], [1, 0, np.inf, 0, 1, 0], [0, 0, 0, 0, 0, 0]):
        assert fn(arr(M1), arr(bad), g, gi) == -1 and fn(arr(bad), arr(M1), g, gi) == -1
    assert fn(arr([1, 2, 0, 2, 4, 0]), arr([1, 2, 0, 2, 4, 0]), g, gi) == -1        # singular, even when equal
