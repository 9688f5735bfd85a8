"""CPU-only: relit frames (DESIGN.md "Relit frames") around the kernel.  The numpy twin tests/light_ref.py against its
per-pixel statement; the shadow's window counts at the frame's corners against hand-computed values; ArapFlow_LightTables
(host only) against the Python statement bit for bit, with every refusal; the neutral description; the deviation of the
noise; pipeline.random_light; the `light` list line in Python and in C++ (host/list_line.h through line_tool); para_gen
--relight with a stand-in worker."""
import ctypes as C
import itertools
import json
import os
import os.path as osp
import random
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import light_ref
import tex_ref
from arap_flow_amd import pipeline

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
F = np.float32
NEUTRAL = pipeline.LIGHT_NEUTRAL
# a rotated field of 6-pixel cells with negative coordinates
LIT = NEUTRAL._replace(seed=7, m=(0.15, 0.08, -2.25, -0.08, 0.15, 0.5), amp=0.3, vig=0.5, gain=(1.1, 0.9, 1.0), gamma=0.8,
                       sigma0=1.0, sigma1=0.05)


def picture(W, H, seed=0):
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    rgb[0, 0], rgb[-1, -1] = (255, 255, 255), (0, 0, 0)
    return rgb


def ellipses(W, H, mask=False):
    """two overlapping ellipses that touch the frame's edges, as a cover (255 = object) or a solver mask (0 = object)"""
    ys, xs = np.mgrid[0:H, 0:W]
    obj = ((xs - 0.2 * W) / (0.35 * W)) ** 2 + ((ys - 0.5 * H) / (0.6 * H)) ** 2 <= 1
    obj |= ((xs - 0.7 * W) / (0.4 * W)) ** 2 + ((ys - 0.9 * H) / (0.45 * H)) ** 2 <= 1
    return np.where(obj, 0, 255).astype(np.uint8) if mask else np.where(obj, 255, 0).astype(np.uint8)


# ---- the twin against the per-pixel statement ---------------------------------------------------------------------------
@pytest.mark.parametrize("r", [0, 1, 16])
@pytest.mark.parametrize("shift", [(0, 0), (5, -3), (-64, 64)], ids=lambda s: "%d_%d" % s)
def test_twin_equals_the_per_pixel_statement(r, shift):
    """23x11: every sh_g of {0, 1, 256} under both cover conventions"""
    W, H = 23, 11
    rgb = picture(W, H, seed=r)
    for k, (g, is_mask) in enumerate(itertools.product((0, 1, 256), (False, True))):
        frame = LIT._replace(seed=(0xffffffff, 0, 7)[k % 3], sh_dx=shift[0], sh_dy=shift[1], sh_r=r, sh_g=g)
        cover = ellipses(W, H, mask=is_mask)
        got = light_ref.relight(rgb, cover, frame, cover_is_mask=is_mask)
        want = light_ref.relight_brute(rgb, cover, frame, cover_is_mask=is_mask)
        assert np.array_equal(got, want), (g, is_mask)


def test_window_counts_at_the_corners():
    """a 5x4 frame with objects at its four corners and at (2, 1), by hand"""
    obj = np.zeros((4, 5), bool)
    obj[0, 0] = obj[0, 4] = obj[3, 0] = obj[3, 4] = obj[1, 2] = True
    a = light_ref.window_counts(obj, 0, 0, 1)
    assert [a[0, 0], a[0, 4], a[3, 0], a[3, 4]] == [1, 1, 1, 1]       # a corner's window holds the corner alone
    assert a[0, 1] == 2 and a[1, 1] == 2 and a[2, 2] == 1 and a[3, 2] == 0 and a[0, 2] == 1 and a[2, 4] == 1
    a = light_ref.window_counts(obj, 0, 0, 16)
    assert (a == 5).all()                                             # the window holds the whole frame everywhere
    a = light_ref.window_counts(obj, 1, 0, 0)                         # the shadow falls one pixel to the right
    assert a[0, 1] == 1 and a[0, 0] == 0 and a[1, 3] == 1 and a[3, 1] == 1 and a.sum() == 3    # two fell outside
    a = light_ref.window_counts(obj, -64, 64, 16)
    assert a.sum() == 0                                               # the window lies outside the frame
    a = light_ref.window_counts(obj, 2, -1, 1)                        # pixel (4, 0): window x 1..3, y 0..2 holds (2, 1)
    assert a[0, 4] == 1 and a[2, 0] == 0 and a[3, 4] == 0 and a[2, 2] == 1      # (2, 2): x -1..1, y 2..4 holds (0, 3)


# ---- ArapFlow_LightTables: the library against the Python statement ------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from arap_flow_amd import build, capi
    build.build()
    return capi.load()


@pytest.mark.parametrize("gamma", [1.0, 0.45, 2.2])
def test_tables_equal_python_bit_for_bit(lib, gamma):
    from arap_flow_amd import opt
    for gain in ((1.0, 0.5, 1.5), (1.5, 1.0, 0.5)):
        frame = NEUTRAL._replace(gain=gain, gamma=gamma)
        for W, H in ((1, 1), (2, 1), (854, 480), (70, 9)):
            lut, geom = opt.light_tables(frame, W, H, lib=lib)
            want_lut, want_geom = light_ref.tables(frame, W, H)
            assert lut.tobytes() == want_lut.tobytes() and geom.tobytes() == want_geom.tobytes()
        assert lut[:, 0].tolist() == [0, 0, 0] and lut[gain.index(1.5), 255] == 255 and lut[gain.index(0.5), 255] == 128
        assert (np.diff(lut.astype(int), axis=1) >= 0).all()


def test_identity_table_and_geometry(lib):
    from arap_flow_amd import opt
    lut, geom = opt.light_tables(NEUTRAL, 1, 1, lib=lib)
    assert (lut == np.arange(256, dtype=np.uint8)).all()
    assert geom.tolist() == [0.0, 0.0, 0.0]                                    # one pixel: no radius, inv_r2 = 0
    assert opt.light_tables(NEUTRAL, 2, 1, lib=lib)[1].tolist() == [0.5, 0.0, 4.0]
    geom = opt.light_tables(NEUTRAL, 854, 480, lib=lib)[1]
    assert geom.tolist() == [426.5, 239.5, float(F(1.0 / (426.5 ** 2 + 239.5 ** 2)))]


BAD_FRAMES = [dict(amp=-0.1), dict(amp=float("nan")), dict(amp=float("inf")), dict(vig=-0.1), dict(vig=1.5), dict(vig=float("nan")),
              dict(gain=(1.0, 0.0, 1.0)), dict(gain=(1.0, 1.0, -1.0)), dict(gain=(float("inf"), 1.0, 1.0)),
              dict(gain=(1.0, float("nan"), 1.0)), dict(gamma=0.0), dict(gamma=-1.0), dict(gamma=float("inf")), dict(gamma=float("nan")),
              dict(sh_dx=65), dict(sh_dx=-65), dict(sh_dy=65), dict(sh_dy=-65), dict(sh_r=-1), dict(sh_r=17), dict(sh_g=-1), dict(sh_g=257),
              dict(sigma0=-1.0), dict(sigma0=float("nan")), dict(sigma1=-0.01), dict(sigma1=float("inf")),
              dict(m=(1.0, 0.0, float("nan"), 0.0, 1.0, 0.0)), dict(m=(float("inf"), 0.0, 0.0, 0.0, 1.0, 0.0))]


def test_tables_refusals(lib):
    from arap_flow_amd import opt
    for kw in BAD_FRAMES:
        with pytest.raises(ValueError):
            opt.light_tables(LIT._replace(**kw), 70, 9, lib=lib)
        assert not pipeline.light_frame_ok(LIT._replace(**kw)), kw
    extreme = LIT._replace(sh_dx=-64, sh_dy=64, sh_r=16, sh_g=256, vig=1.0, amp=0.0, sigma0=0.0)
    assert pipeline.light_frame_ok(extreme) and pipeline.light_frame_ok(LIT)
    opt.light_tables(extreme, 70, 9, lib=lib)
    for W, H in ((0, 9), (70, 0), (1 << 16, 1 << 15)):
        with pytest.raises(ValueError):
            opt.light_tables(LIT, W, H, lib=lib)
    q = opt.light_frame(LIT)
    lut, geom = (C.c_uint8 * 768)(), (C.c_float * 3)()
    assert lib.ArapFlow_LightTables(C.byref(q), 70, 9, lut, geom) == 0
    assert lib.ArapFlow_LightTables(None, 70, 9, lut, geom) == -1
    assert lib.ArapFlow_LightTables(C.byref(q), 70, 9, None, geom) == -1
    assert lib.ArapFlow_LightTables(C.byref(q), 70, 9, lut, None) == -1


# ---- what the arithmetic promises ------------------------------------------------------------------------------------
def test_neutral_description_returns_the_input():
    rgb = picture(23, 11)
    assert np.array_equal(light_ref.relight(rgb, None, NEUTRAL), rgb)
    moved = NEUTRAL._replace(seed=0xffffffff, m=LIT.m, sh_dx=5, sh_dy=-3, sh_r=16)      # what a neutral frame may still carry
    assert pipeline.light_is_neutral(moved) and not pipeline.light_is_neutral(LIT)
    assert np.array_equal(light_ref.relight(rgb, ellipses(23, 11), moved), rgb)


def test_object_pixels_ignore_the_rest_of_the_cover():
    rgb, cover = picture(23, 11), ellipses(23, 11)
    frame = LIT._replace(sh_dx=2, sh_dy=1, sh_r=3, sh_g=200)
    alone = np.where(np.arange(23 * 11).reshape(11, 23) % 7 == 0, cover, 0).astype(np.uint8)      # fewer objects
    a, b = light_ref.relight(rgb, cover, frame), light_ref.relight(rgb, alone, frame)
    both = (cover != 0) & (alone != 0)
    assert both.any() and np.array_equal(a[both], b[both]) and not np.array_equal(a, b)


@pytest.mark.parametrize("seed", [0, 0xffffffff, 0x9e3779b9])
def test_noise_has_the_stated_deviation(seed):
    """a flat 128 frame of 256 x 256, sigma0 = 4: per channel the sample deviation lies within 3.9 .. 4.1 (nine standard
    errors sigma / sqrt(2 N) = 0.011; measured 3.99 .. 4.03)"""
    rgb = np.full((256, 256, 3), 128, np.uint8)
    out = light_ref.relight(rgb, None, NEUTRAL._replace(seed=seed, sigma0=4.0)).astype(np.float64)
    for c in range(3):
        std = out[..., c].std()
        print("seed %#x channel %d: std %.4f mean %.4f" % (seed, c, std, out[..., c].mean()))
        assert 3.9 <= std <= 4.1
    assert not np.array_equal(out[..., 0], out[..., 1]) and not np.array_equal(out[..., 1], out[..., 2])


# ---- random_light ------------------------------------------------------------------------------------------------------
def test_random_light():
    for s in range(5):
        f1, f2 = pipeline.random_light(random.Random(s), 0, 854, 480)
        assert pipeline.light_is_neutral(f1) and pipeline.light_is_neutral(f2)
        assert pipeline.light_frame_ok(f1) and pipeline.light_frame_ok(f2)
    rgb = picture(70, 9)
    for f in pipeline.random_light(random.Random(1), 0, 70, 9):
        assert np.array_equal(light_ref.relight(rgb, ellipses(70, 9), f), rgb)
    for s, strength, (W, H) in ((0, 1.0, (854, 480)), (1, 0.25, (70, 9)), (2, 3.0, (1920, 1080)), (3, 1.0, (7, 5))):
        f1, f2 = pipeline.random_light(random.Random(s), strength, W, H)
        assert (f1, f2) == pipeline.random_light(random.Random(s), strength, W, H)      # the same state, the same pair
        assert pipeline.light_frame_ok(f1) and pipeline.light_frame_ok(f2) and not pipeline.light_is_neutral(f1)
        # shared: the shadow's geometry, the vignette (and the field's amplitude, the noise's deviations)
        assert f1[6:] == f2[6:] and f1.vig == f2.vig and f1.amp == f2.amp and f1.sh_g > 0
        assert f1.seed != f2.seed and f1.gain != f2.gain                        # own noise, a flickering tone curve
        assert all(abs(a / b - 1) <= 0.03 * strength + 1e-6 for a, b in zip(f2.gain, f1.gain))
        assert f1.m[:2] == f2.m[:2] and f1.m[3:5] == f2.m[3:5]                  # the field only shifts ...
        du, dv = f2.m[2] + pipeline.LIGHT_TWIN_SHIFT - f1.m[2], f2.m[5] - f1.m[5]
        assert abs(du) <= 0.2501 and abs(dv) <= 0.2501 and (du, dv) != (0, 0)   # ... by a fraction of a cell
    with pytest.raises(ValueError):
        pipeline.random_light(random.Random(0), -1.0, 70, 9)


@pytest.mark.parametrize("seed", [0, 1, 0xffffffff, 0x9e3779b9])
def test_twin_seed_sees_the_same_field_through_other_noise(seed):
    twin = pipeline.light_twin_seed(seed)
    S = pipeline.LIGHT_TWIN_SHIFT
    i, j = np.meshgrid(np.arange(0, S, dtype=np.int32), np.arange(-3, 4, dtype=np.int32))
    assert np.array_equal(tex_ref.hash3(twin, i, j, 0), tex_ref.hash3(seed, i + np.int32(S), j, 0))     # the field's lattice
    x, y = np.meshgrid(np.arange(64, dtype=np.int32), np.arange(8, dtype=np.int32))
    for k in range(1, 13):                                                                                # the noise's streams
        assert (tex_ref.hash3(twin, x, y, k) != tex_ref.hash3(seed, x, y, k)).mean() > 0.99
    # the two frames of a pair: frame 2's field is frame 1's a little further on -- not a jump
    f1, f2 = pipeline.random_light(random.Random(seed), 1.0, 130, 70)
    (u1, v1), (u2, v2) = tex_ref.texture_points((0, 0, f1.m), 130, 70), tex_ref.texture_points((0, 0, f2.m), 130, 70)
    assert u2.min() >= 0 and u2.max() < S - 1 and u1.min() >= S and u1.max() < 2 * S - 1
    drift = np.abs(tex_ref.vnoise(f2.seed, u2, v2, 0) - tex_ref.vnoise(f1.seed, u1, v1, 0)).max()
    jump = np.abs(tex_ref.vnoise(seed + 1, u2, v2, 0) - tex_ref.vnoise(f1.seed, u1, v1, 0)).max()
    print("seed %#x: largest change of the field with the twin %.4f, with another seed %.4f" % (seed, drift, jump))
    assert 0 < drift <= 1.5 * 0.5 + 1e-3            # the smoothstep's slope is at most 1.5 per cell, the drift a quarter cell each way


# ---- the light line: host/list_line.h against pipeline.parse_line ------------------------------------------------------
_F1 = "7,0.15,0.08,-2.25,-0.08,0.15,0.5,0.3,0.5,1.1,0.9,1,0.8,5,-3,16,256,1,0.05"
_F2 = "4294967295,1,0,0,0,1,0,0,0,1,1,1,1,-64,64,0,0,0,0"
_L = "light R1 M1 R2 C2"
_ONE = lambda k, v: ",".join(v if i == k else q for i, q in enumerate(_F1.split(",")))      # _F1 with number k replaced
GOOD = [
    _L + " l=" + _F1 + ";" + _F2 + " rgb1=A rgb2=B", _L + " rgb2=B l=" + _F2 + ";" + _F1 + " rgb1=A",      # done = B: the first output
    _L + " l=" + _F1 + ";" + _F1 + " rgb2=B", _L + " rgb1=A l=" + _ONE(7, "1e-3") + ";" + _ONE(13, "-0"),
    _L + " l=" + _ONE(1, "0.100000001") + ";" + _ONE(8, "1") + " rgb1=A", _L + " l=" + _ONE(15, "0") + ";" + _ONE(17, "2.5e2") + " rgb1=A",
]
BAD = [
    _L + " l=" + _F1 + ";" + _F2, _L + " rgb1=A",                                         # no output; no l=
    _L + " l=" + _F1 + ";" + _F2 + " rgb1=A foo=B", _L + " l=" + _F1 + ";" + _F2 + " rgb1=A alpha1=O",       # unknown keys
    _L + " l=" + _F1 + ";" + _F2 + " rgb1=", _L + " l= rgb1=A", _L + " l=" + _F1 + ";" + _F2 + " rgb1",     # empty values, a missing `=`
    _L + " l=" + _F1 + " rgb1=A", _L + " l=" + _F1 + ";" + _F2 + ";" + _F2 + " rgb1=A", _L + " l=" + _F1 + "; rgb1=A",     # not two frames
    _L + " l=" + _F1 + ",1;" + _F2 + " rgb1=A", _L + " l=" + _F1[:-5] + ";" + _F2 + " rgb1=A",     # 20 and 18 numbers
    _L + " l=" + _F1 + ";" + _F2 + " rgb1=A rgb1=B", _L + " l=" + _F1 + ";" + _F2 + " l=" + _F1 + ";" + _F2 + " rgb1=A",      # repeated keys
    "light R1 M1 R2 l=" + _F1 + ";" + _F2 + " rgb1=A", "light R1 M1 rgb1=A", "light", "light R1",     # a token where a path is expected
] + [_L + " l=" + _ONE(k, v) + ";" + _F2 + " rgb1=A" for k, v in (
    (0, "-1"), (0, "4294967296"), (0, "1.0"), (0, "x"), (1, "nan"), (3, "inf"), (6, "1e39"), (2, "x"), (2, ""),      # seed, map
    (7, "-0.1"), (7, "nan"), (8, "-0.1"), (8, "1.5"), (9, "0"), (10, "-1"), (11, "inf"), (12, "0"), (12, "nan"),      # amp, vig, tone curve
    (13, "65"), (13, "-65"), (14, "65"), (14, "-65"), (13, "1.0"), (14, "x"), (13, "--1"), (13, "99999999999"),      # the shadow's offset
    (15, "17"), (15, "-1"), (15, "1.0"), (16, "257"), (16, "-1"), (16, "x"), (16, "4294967296"),                      # radius, depth
    (17, "-1"), (17, "nan"), (18, "-0.5"), (18, "inf"), (18, "x"))] + [
    _L + " l=" + _F2 + ";" + _ONE(15, "17") + " rgb1=A",                                  # the second frame is checked too
]


@pytest.fixture(scope="module")
def bins():
    from arap_flow_amd import build
    return {osp.basename(o): o for o in build.build_host()}


def test_light_line_round_trip():
    item = pipeline.LightLine("R1", "M1", "R2", "C2", pipeline.random_light(random.Random(5), 1.0, 854, 480), dict(rgb2="B", rgb1="A"))
    text = pipeline.format_line(item)
    back = pipeline.parse_line(text)
    assert back.frames == item.frames and back[:4] == ("R1", "M1", "R2", "C2") and back.out == dict(rgb1="A", rgb2="B")
    assert pipeline.format_line(back) == text and pipeline.done_token(back) == "A"
    assert pipeline.done_token(pipeline.parse_line(GOOD[1])) == "B"
    first = pipeline.parse_line(GOOD[0]).frames[0]
    assert first == LIT._replace(sh_dx=5, sh_dy=-3, sh_r=16, sh_g=256, **{k: tuple(float(F(v)) for v in getattr(LIT, k)) for k in ("m", "gain")},
                                 **{k: float(F(getattr(LIT, k))) for k in ("amp", "gamma", "sigma1")})
    for line in GOOD:
        assert isinstance(pipeline.parse_line(line), pipeline.LightLine)
        assert pipeline.parse_line(pipeline.format_line(pipeline.parse_line(line))) == pipeline.parse_line(line)


def test_light_line_parser_equals_python_twin(bins):
    """every line through line_tool in one process: a good one comes back as format_line(parse_line(line)) + its done
    token, a bad one as BAD after the grammar's own message -- and Python refuses exactly those"""
    corpus = GOOD + BAD
    r = subprocess.run([bins["line_tool"]], input="".join(c + "\n" for c in corpus), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")[:-1]
    got = [ln for ln in lines if not ln.startswith("Invalid")]
    assert len(got) == len(corpus)
    assert [ln for ln in lines if ln.startswith("Invalid")] == ["Invalid light line: " + b for b in BAD]
    for line, g in zip(GOOD, got):
        item = pipeline.parse_line(line)
        assert g == pipeline.format_line(item) + " done=" + pipeline.done_token(item), line
    assert got[1].endswith(" done=B") and got[0].endswith(" done=A")
    for line, g in zip(BAD, got[len(GOOD):]):
        assert g == "BAD", line
        with pytest.raises(ValueError):
            pipeline.parse_line(line)


def test_arap_deform_refuses_a_bad_light_line_before_any_gpu_call(bins, tmp_path):
    lst = tmp_path / "l.txt"
    lst.write_text("a b c d e f\n" + BAD[2] + "\n")
    r = subprocess.run([bins["arap_deform"], str(lst)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "Invalid light line: " + BAD[2] + "\n"
    r = subprocess.run([sys.executable, osp.join(ROOT, "arap_deform.py"), str(lst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "light line" in r.stdout


# ---- para_gen --relight with a stand-in worker --------------------------------------------------------------------------
FAKE_WORKER = r'''
import os, shutil, sys
# stand-in for arap_deform (no GPU): a solve line writes the files para_gen expects; a light line REFUSES to run (exit 3)
# unless every file it names is there already and its second frame carries the background (the marker colour), then writes
# its outputs; a bg line paints the marker into its second frame and writes its flow; every line is logged
import numpy as np
from PIL import Image
sys.path.insert(0, %r)
from arap_flow_amd import flo as F, pipeline
LOG = %r
MOTION = %r
def run(line):
    item = pipeline.parse_line(line)
    with open(LOG, "a") as log:
        log.write(line.rstrip("\n") + "\n")
    if isinstance(item, pipeline.LightLine):
        for q in item[:4]:
            if not os.path.exists(q):
                print("light line before its inputs: " + q, flush=True)
                sys.exit(3)
        if "_seg" in item.rgb2 or "_seg" in item.cover2:
            print("light line on a segment's files", flush=True)
            sys.exit(3)
        src = np.array(Image.open(item.rgb2).convert("RGB"))
        if MOTION and not (src[0, 0] == (9, 8, 7)).all():
            print("light line before the pair's bg line", flush=True)
            sys.exit(3)
        m1 = np.array(Image.open(item.mask1).convert("RGB"))[..., 0]
        if not ((m1 == 0).any() and (m1 != 0).any()):
            print("light line without an object mask", flush=True)
            sys.exit(3)
        src[::2] = (4, 5, 6)
        for k in item.out:
            Image.fromarray(src).save(item.out[k])
        return
    if isinstance(item, pipeline.BgLine):
        shutil.copy(item.flow, item.out[2])
        im = np.array(Image.open(item.out[1]).convert("RGB"))
        im[0, 0] = (9, 8, 7)
        Image.fromarray(im).save(item.out[1])
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


def _light_run(tmp_path, extra, worker, motion=False, relight=()):
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
    fake.write_text(FAKE_WORKER % (ROOT, str(log), motion))
    outp = tmp_path / "out"
    own = "%s %s" % (sys.executable, osp.join(ROOT, "arap_deform.py"))
    flags = para_gen.parse(["--input", str(inp), "--output", str(outp), "--gpu", "0", "1", "--matches", str(mdir), "--worker", worker,
                            "--arap_bin", own, "--narap", "3", "--jobs", "2", "--bg_dir", str(tmp_path / "bgs"), "--relight"] +
                           list(relight) + extra + (["--bg_motion"] if motion else []))
    flags.arap_bin = "%s %s" % (sys.executable, fake)          # (the flags are checked against this repository's driver)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        out = para_gen.main(flags)
    finally:
        os.chdir(cwd)
    return outp, out, [pipeline.parse_line(ln) for ln in (log.read_text().splitlines() if log.exists() else [])]


@pytest.mark.parametrize("worker,multseg,motion", [("serve", False, False), ("serve", True, True), ("batch", True, False),
                                                   ("serve", False, True)])
def test_para_gen_relight_with_a_stand_in_worker(tmp_path, worker, multseg, motion):
    outp, out, lines = _light_run(tmp_path, ["--multseg"] if multseg else [], worker, motion, relight=("0.5",) if motion else ())
    assert len(out) == 6                                                    # 2 sequences x 3 pairs
    light = [it for it in lines if isinstance(it, pipeline.LightLine)]
    solves = [it for it in lines if isinstance(it, pipeline.SolveLine)]
    bgs = [it for it in lines if isinstance(it, pipeline.BgLine)]
    assert len(light) == 6 and len(solves) == (12 if multseg else 6) and len(bgs) == (6 if motion else 0)
    # a light line names the pair's finished frames (the stand-in refuses one whose files are not final: the run got here)
    listed_pairs = [pair.split(" ") for pair in out]
    assert sorted((it.rgb1, it.rgb2) for it in light) == sorted((a, b) for a, b, _ in listed_pairs)
    assert all(set(it.out) == {"rgb1", "rgb2"} and it.cover2.replace("wMasks", "wRGB") == it.rgb2 for it in light)
    at = {id(it): k for k, it in enumerate(lines)}
    if motion:                                                              # after the pair's bg line, over the same object mask
        by_rgb = {it.rgb1: it for it in bgs}
        assert all(at[id(it)] > at[id(by_rgb[it.rgb1])] and it.mask1 == by_rgb[it.rgb1].mask1 for it in light)
    for it in light:                                                        # after every solve of its pair
        stem = osp.splitext(it.rgb2)[0]
        mine = [s for s in solves if s.out_rgb.startswith(stem)]
        assert len(mine) == (2 if multseg else 1) and all(at[id(s)] < at[id(it)] for s in mine)
    # the pair's own light: drawn from the pair's id at the flag's strength, the two frames of random_light
    for it in light:
        f1, f2 = it.frames
        assert f1[6:] == f2[6:] and f1.vig == f2.vig and f2.seed == pipeline.light_twin_seed(f1.seed) and f1.sh_g > 0
    assert len({it.frames for it in light}) == 6
    st = json.load(open(outp / "arap_stats.json"))
    assert st["light_done"] == 6 and st["frames_done"] == 6 and st["bg_done"] == (6 if motion else 0) and st["blur_done"] == 0
    listed = (outp / "all_files_light.list").read_text().split("\n")
    assert len(listed) == 6
    for pair, twin in zip(out, listed):
        (rgb1, rgb2, flow), (l1, l2, lflow) = pair.split(" "), twin.split(" ")
        assert lflow == flow and all(osp.exists(q) for q in (l1, l2, lflow))          # the SAME flow file
        assert l1 == rgb1.replace(osp.sep + "inpRGB" + osp.sep, osp.sep + "inpRGB_light" + osp.sep)
        assert l2 == rgb2.replace(osp.sep + "wRGB" + osp.sep, osp.sep + "wRGB_light" + osp.sep)
        assert (np.array(Image.open(l2).convert("RGB"))[::2] == (4, 5, 6)).all()
    if multseg:                                                             # per-segment files were merged and removed
        assert not [f for f in os.listdir(outp / "Flow" / "a") if "_seg" in f]
    left = [f for f in os.listdir(outp / "tmpCnstr" / "a") if "_lightmask" in f or "_bg" in f]
    assert not left, left                                                   # the lines' own inputs are gone
    assert not (outp / "all_files_tex.list").exists() and not (outp / "all_files_blur.list").exists()


def test_para_gen_relight_resume(tmp_path):
    """--resume skips a pair only when its relit files exist too"""
    outp, out, lines = _light_run(tmp_path, [], "serve")
    listed = (outp / "all_files_light.list").read_text().split("\n")
    assert len(out) == 6 and len(listed) == 6
    gone = listed[2].split(" ")[1]
    os.remove(gone)
    outp, out2, lines = _light_run(tmp_path, ["--resume"], "serve")
    light = [it for it in lines if isinstance(it, pipeline.LightLine)]
    assert len(light) == 1 and light[0].out["rgb2"] == gone and osp.exists(gone)
    outp, out3, lines = _light_run(tmp_path, ["--resume"], "serve")
    assert lines == []                                                      # everything is there: nothing is handed out


def test_para_gen_without_relight_writes_nothing_of_it(tmp_path):
    sys.path.insert(0, ROOT)
    import helpers
    import para_gen
    flags = helpers.para_gen_flags([])
    assert flags.relight is None
    assert helpers.para_gen_flags(["--bg_dir", "b", "--relight"]).relight == 1.0
    assert helpers.para_gen_flags(["--bg_dir", "b", "--relight", "0.25", "--multseg", "--bg_motion"]).relight == 0.25
    assert helpers.para_gen_flags(["--bg_dir", "b", "--relight", "0"]).relight == 0.0
    assert para_gen.scan(flags, str(tmp_path / "nothing"), str(tmp_path / "out")) == []
    from test_pipeline_host import _tiny_tree
    _tiny_tree(tmp_path, nframes=3, seqs=("a",))
    plain = para_gen.scan(helpers.para_gen_flags([]), str(tmp_path / "in"), str(tmp_path / "out"))
    relit = para_gen.scan(helpers.para_gen_flags(["--bg_dir", "b", "--relight"]), str(tmp_path / "in"), str(tmp_path / "out"))
    assert plain and not [k for p in plain for k in p if "light" in k]
    assert all(set(r) - set(p) == {"rgb1light_gen", "rgb2light_gen"} for p, r in zip(plain, relit))
    assert all(p == {k: v for k, v in r.items() if k in p} for p, r in zip(plain, relit))       # nothing else differs


def test_para_gen_refuses_relight(capsys):
    import helpers
    bg = ["--bg_dir", "b"]
    for extra in ([], bg + ["--mid", "2"], bg + ["--multseg", "--mid_layers", "2"], bg + ["--retex"], bg + ["--blur", "0.5"],
                  bg + ["--bg_motion", "--mid", "2", "--mid_bg"], bg + ["--arap_bin", "/bin/true"]):
        with pytest.raises(SystemExit):
            helpers.para_gen_flags(["--relight"] + extra)
        assert "--relight" in capsys.readouterr().err
    for strength in ("-1", "nan", "inf", "x"):
        with pytest.raises(SystemExit):
            helpers.para_gen_flags(bg + ["--relight", strength])
        assert "--relight" in capsys.readouterr().err


def test_new_entry_points_exported():
    from arap_flow_amd import build, capi, opt
    lib = C.CDLL(build.build())
    for name in ("ArapFlow_LightTables", "ArapFlow_Relight"):
        assert hasattr(lib, name), name
        assert name in [s[0] for s in capi.SYMBOLS]
    assert C.sizeof(capi.LightFrame) == 76 and len(pipeline.LightFrame._fields) == 12
    assert (capi.LIGHT_MAX_R, capi.LIGHT_MAX_SHIFT) == (pipeline.LIGHT_MAX_R, pipeline.LIGHT_MAX_SHIFT) == (16, 64)
    header = open(osp.join(ROOT, "include", "arap_opt.h")).read()
    assert "#define ARAPFLOW_LIGHT_MAX_R 16\n" in header and "#define ARAPFLOW_LIGHT_MAX_SHIFT 64\n" in header
    for name in ("relight", "relight_pair", "light_tables", "light_frame"):
        assert callable(getattr(opt, name))
    for name in ("LightFrame", "LightLine", "parse_light", "light_line", "run_light", "random_light"):
        assert hasattr(pipeline, name)
