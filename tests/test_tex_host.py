"""CPU-only: random textures (DESIGN.md "Random textures") around the kernel.  The numpy twin tests/tex_ref.py against
closed forms that need no twin; the layer draws of para_gen --retex (pipeline.tex_layers); the `tex` list line in Python
and in C++ (host/list_line.h through line_tool); para_gen --retex with a stand-in worker."""
import json
import os
import os.path as osp
import random
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import tex_ref
from arap_flow_amd import pipeline

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
F = np.float32
C0, C1, C2 = (250, 10, 30), (20, 200, 90), (5, 5, 120)
W, H = 64, 36
CELLS = (pipeline.TEX_CELL_MIN, max(pipeline.TEX_CELL_MIN, min(W, H) / 3.0))       # the ends of tex_layers' range here


def scaled(kind, size, seed=7, p0=0.0, p1=0.0, shift=(0.0, 0.0), aspect=1.0):
    """the identity map scaled by 1 / size (and 1 / aspect more along x), shifted by whole cells"""
    m = tuple(float(F(v)) for v in (1.0 / (size * aspect), 0.0, shift[0], 0.0, 1.0 / size, shift[1]))
    return pipeline.TexLayer(kind, seed, m, float(F(p0)), float(F(p1)), C0, C1, C2)


@pytest.mark.parametrize("s", [4, 5, 8])
def test_checker_closed_form(s):
    ys, xs = np.mgrid[0:H, 0:W]
    want = np.array([C0, C1], np.uint8)[(xs // s + ys // s) & 1]
    assert np.array_equal(tex_ref.colour(scaled(tex_ref.CHECKER, s), W, H), want)


def test_checker_shifts_by_whole_cells():
    s, k = 4, 3
    base = tex_ref.colour(scaled(tex_ref.CHECKER, s), W, H)
    moved = tex_ref.colour(scaled(tex_ref.CHECKER, s, shift=(k, -2)), W, H)      # u + 3, v - 2
    assert np.array_equal(moved[2 * s:, :W - k * s], base[:H - 2 * s, k * s:])


def test_brick_mortar_is_where_the_formula_puts_it():
    """u = x / 8, v = y / 4, mortar 1/4 of a cell, odd rows shifted by half a cell: every number is a power of two"""
    img = tex_ref.colour(scaled(tex_ref.BRICK, 4, p0=0.25, p1=0.5, aspect=2.0), W, H)
    ys, xs = np.mgrid[0:H, 0:W]
    row = ys // 4
    mortar = (ys % 4 == 0) | np.where(row % 2 == 0, xs % 8 < 2, (xs + 4) % 8 < 2)
    is_c2 = (img == np.array(C2, np.uint8)).all(-1)
    assert np.array_equal(is_c2, mortar)
    bricks = img[~mortar]
    assert ((bricks == np.array(C0, np.uint8)).all(-1) | (bricks == np.array(C1, np.uint8)).all(-1)).all()
    col = np.where(row % 2 == 0, xs // 8, (xs + 4) // 8)
    for r, c in {(int(a), int(b)) for a, b in zip(row[~mortar], col[~mortar])}:   # one colour per brick
        assert len(np.unique(img[(row == r) & (col == c) & ~mortar], axis=0)) == 1
    assert len(np.unique(bricks, axis=0)) == 2


@pytest.mark.parametrize("kind", range(5), ids=tex_ref.KINDS)
def test_every_channel_stays_inside_the_palette(kind):
    lo, hi = np.min([C0, C1, C2], 0), np.max([C0, C1, C2], 0)
    for size in CELLS:
        for p1 in (0.0, 1.0):
            rot = pipeline.TexLayer(kind, 99, (0.31 / size, 0.2 / size, -7.5, -0.2 / size, 0.31 / size, 3.25), 0.4, p1, C0, C1, C2)
            for layer in (scaled(kind, size, p0=0.1, p1=p1), rot):
                img = tex_ref.colour(layer, W, H)
                assert (img >= lo).all() and (img <= hi).all()


@pytest.mark.parametrize("kind", range(5), ids=tex_ref.KINDS)
def test_no_kind_comes_out_flat_at_either_end_of_the_cell_range(kind):
    """fixed seeds, checked here with the twin alone: an all-object 64x36 frame shows at least two colours"""
    for size in CELLS:
        for seed in (7, 0xdeadbeef):
            img = tex_ref.colour(scaled(kind, size, seed=seed, p0=0.1, p1=0.5, aspect=2.5 if kind == tex_ref.BRICK else 1.0), W, H)
            assert len(np.unique(img.reshape(-1, 3), axis=0)) >= 2, (size, seed)


def test_owner_is_the_highest_layer():
    masks = np.full((3, 2, 3), 255, np.uint8)
    masks[0, 0, :] = 0
    masks[1, 0, 1:] = 0
    masks[2, 0, 2] = 0
    assert tex_ref.owner(masks).tolist() == [[0, 1, 2], [-1, -1, -1]]
    rgb = np.arange(18, dtype=np.uint8).reshape(2, 3, 3)
    layers = [scaled(tex_ref.CHECKER, 64)._replace(c0=(l, l, l)) for l in (10, 20, 30)]
    out = tex_ref.texture(rgb, masks, layers)
    assert out[0].tolist() == [[10] * 3, [20] * 3, [30] * 3] and np.array_equal(out[1], rgb[1])


def test_tex_layers_is_a_function_of_the_rng_state():
    a = pipeline.tex_layers(random.Random(123), 4, (854, 480))
    b = pipeline.tex_layers(random.Random(123), 4, (854, 480))
    c = pipeline.tex_layers(random.Random(124), 4, (854, 480))
    assert a == b and a != c and len(a) == 4
    kinds = set()
    for wh in ((854, 480), (64, 36), (16, 10)):
        hi = max(pipeline.TEX_CELL_MIN, min(wh) / 3.0)
        for q in pipeline.tex_layers(random.Random(5), 60, wh):
            kinds.add(q.kind)
            assert 0 <= q.kind < len(pipeline.TEX_KINDS) and 0 <= q.seed <= 0xffffffff and q.c0 != q.c1
            assert all(float(F(v)) == v and np.isfinite(v) for v in q.m + (q.p0, q.p1))
            size = 1.0 / np.hypot(q.m[3], q.m[4])                  # the cell's height in pixels
            assert pipeline.TEX_CELL_MIN * (1 - 1e-5) <= size <= hi * (1 + 1e-5)
            wide = 1.0 / np.hypot(q.m[0], q.m[1]) / size           # the cell's aspect ratio
            assert (2 - 1e-4 <= wide <= 3 + 1e-4) if pipeline.TEX_KINDS[q.kind] == "brick" else abs(wide - 1) < 1e-4
            assert abs(q.m[0] * q.m[3] + q.m[1] * q.m[4]) < 1e-6   # a rotation: the axes stay orthogonal
    assert kinds == set(range(len(pipeline.TEX_KINDS)))


def test_tex_layers_redraws_an_equal_second_colour():
    class Stuck(random.Random):
        """uniform() gives its lower bound for the first 16 calls: a layer's seven shape draws and three equal colours"""
        calls = 0

        def uniform(self, a, b):
            self.calls += 1
            return a if self.calls <= 16 else super().uniform(a, b)
    rng = Stuck(1)
    q, = pipeline.tex_layers(rng, 1, (64, 36))
    assert rng.calls > 16 and q.c0 == q.c2 == (128, 128, 128) and q.c1 != q.c0


def _random_line(rng, n, out):
    bits = rng.integers(0, 1 << 32, (n, 8), dtype=np.uint64).astype(np.uint32)
    bits = np.where((bits & 0x7f800000) == 0x7f800000, bits & np.uint32(0x3fffffff), bits)      # finite ones only
    vals = bits.view(F)
    tex = tuple(pipeline.TexLayer(int(rng.integers(0, 5)), int(rng.integers(0, 1 << 32)), tuple(float(v) for v in vals[l, :6]),
                                  float(vals[l, 6]), float(vals[l, 7]), *[tuple(int(c) for c in rng.integers(0, 256, 3)) for _ in range(3)])
                for l in range(n))
    return pipeline.TexLine("R.png", [("m%d.png" % l, "f%d.flo" % l) for l in range(n)], tex, out)


def test_tex_line_round_trips_every_float_bit():
    rng = np.random.default_rng(11)
    for n, out in ((1, dict(rgb1="a")), (3, dict(rgb1="a", rgb2="b", mask2="c")), (255, dict(mask2="c"))):
        item = _random_line(rng, n, out)
        text = pipeline.format_line(item)
        back = pipeline.parse_line(text)
        assert isinstance(back, pipeline.TexLine) and back == item
        for q, r in zip(item.tex, back.tex):
            assert np.array(q.m + (q.p0, q.p1), F).tobytes() == np.array(r.m + (r.p0, r.p1), F).tobytes()
        assert pipeline.format_line(back) == text and pipeline.done_token(back) == next(iter(out.values()))
    seeds = pipeline.parse_line("tex R 2 m f m f t=%s;%s rgb2=x" % (_L.replace("7,0.25", "0,0.25"), _L.replace("7,0.25", "4294967295,0.25")))
    assert [q.seed for q in seeds.tex] == [0, 0xffffffff] and pipeline.done_token(seeds) == "x"


# ---- the tex line: host/list_line.h against pipeline.parse_line ---------------------------------------------------------
_L = "1,7,0.25,0,-3.5,0,0.125,1e-3,0.1,0.5,1,2,3,40,50,60,255,0,9"
_T = "tex R 1 m1 f1"
GOOD = [
    _T + " t=" + _L + " rgb1=A", _T + " rgb2=B t=" + _L + " rgb1=A mask2=C",          # done = B: the first output on the line
    _T + " t=" + _L + " mask2=C", "tex R 2 m1 f1 m2 f2 t=" + _L + ";" + _L.replace("1,7,", "4,4294967295,") + " rgb1=A rgb2=B",
    _T + " t=" + _L.replace("1e-3", "0.100000001") + " rgb1=A",
]
BAD = [
    _T + " t=" + _L, _T + " rgb1=A",                                                  # no output; no t=
    _T + " t=" + _L + " rgb1=A foo=B", _T + " t=" + _L + " rgb1=A occ=O",             # unknown keys
    _T + " t=" + _L + " rgb1=", _T + " t= rgb1=A", _T + " t=" + _L + " rgb1",         # empty values, a missing `=`
    _T + " t=" + _L + ",4 rgb1=A", _T + " t=" + _L[:-2] + " rgb1=A",                  # 20 and 18 numbers
    _T + " t=" + _L + ";" + _L + " rgb1=A", "tex R 2 m1 f1 m2 f2 t=" + _L + " rgb1=A",     # layers: one too many, one too few
    _T + " t=" + _L + "; rgb1=A",
    _T + " t=" + _L.replace("1,7,", "5,7,") + " rgb1=A", _T + " t=" + _L.replace("1,7,", "1,4294967296,") + " rgb1=A",
    _T + " t=" + _L.replace("255,0,9", "256,0,9") + " rgb1=A", _T + " t=" + _L.replace("1,7,", "1,-7,") + " rgb1=A",
    _T + " t=" + _L.replace("1,7,", "1.0,7,") + " rgb1=A", _T + " t=" + _L.replace("0.125", "x") + " rgb1=A",
    _T + " t=" + _L.replace("0.125", "nan") + " rgb1=A", _T + " t=" + _L.replace("0.125", "inf") + " rgb1=A",
    _T + " t=" + _L.replace("0.125", "1e39") + " rgb1=A", _T + " t=" + _L.replace("0.125", "") + " rgb1=A",
    _T + " t=" + _L + " rgb1=A rgb1=B", _T + " t=" + _L + " t=" + _L + " rgb1=A",     # repeated keys
    "tex R 0 t=" + _L + " rgb1=A", "tex R 256 t=" + _L + " rgb1=A", "tex R x m1 f1 t=" + _L + " rgb1=A", "tex R 2 m1 f1 m2",
    "tex", "tex R",
]


@pytest.fixture(scope="module")
def bins():
    from arap_flow_amd import build
    return {osp.basename(o): o for o in build.build_host()}


def test_tex_line_parser_equals_python_twin(bins):
    """every line through line_tool in one process: a good one comes back as format_line(parse_line(line)) + its done
    token, a bad one as BAD after the grammar's own message -- and Python refuses exactly those"""
    corpus = GOOD + BAD
    r = subprocess.run([bins["line_tool"]], input="".join(c + "\n" for c in corpus), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")[:-1]
    got = [ln for ln in lines if not ln.startswith("Invalid")]
    assert len(got) == len(corpus)
    assert [ln for ln in lines if ln.startswith("Invalid")] == ["Invalid tex line: " + b for b in BAD]
    for line, g in zip(GOOD, got):
        item = pipeline.parse_line(line)
        assert g == pipeline.format_line(item) + " done=" + pipeline.done_token(item), line
    assert got[1].endswith(" done=B") and got[0].endswith(" done=A") and got[2].endswith(" done=C")
    for line, g in zip(BAD, got[len(GOOD):]):
        assert g == "BAD", line
        with pytest.raises(ValueError):
            pipeline.parse_line(line)


def test_arap_deform_refuses_a_bad_tex_line_before_any_gpu_call(bins, tmp_path):
    lst = tmp_path / "l.txt"
    lst.write_text("a b c d e f\n" + BAD[2] + "\n")
    r = subprocess.run([bins["arap_deform"], str(lst)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "Invalid tex line: " + BAD[2] + "\n"
    r = subprocess.run([sys.executable, osp.join(ROOT, "arap_deform.py"), str(lst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "tex line" in r.stdout


# ---- para_gen --retex with a stand-in worker ----------------------------------------------------------------------------
FAKE_WORKER = r'''
import os, shutil, sys
# stand-in for arap_deform (no GPU): a solve line writes the files para_gen expects; a tex line REFUSES to run (exit 3)
# unless every flow it names is there already, then writes its outputs; every line is logged with the files it found
import numpy as np
from PIL import Image
sys.path.insert(0, %r)
from arap_flow_amd import flo as F, pipeline
LOG = %r
def run(line):
    item = pipeline.parse_line(line)
    with open(LOG, "a") as log:
        log.write(line.rstrip("\n") + "\n")
    if isinstance(item, pipeline.TexLine):
        for m, f in item.layers:
            if not (os.path.exists(m) and os.path.exists(f)):
                print("tex line before its solve: " + f, flush=True)
                sys.exit(3)
        src = np.array(Image.open(item.rgb).convert("RGB"))
        obj = np.any([np.array(Image.open(m).convert("RGB"))[..., 0] == 0 for m, _ in item.layers], axis=0)
        src[obj] = (1, 2, 3)
        for k in ("rgb1", "rgb2"):
            Image.fromarray(src).save(item.out[k])
        return
    m = np.array(Image.open(item.mask).convert("RGB"))[..., 0]
    F.flow_write(item.flow, np.zeros(m.shape + (2,), np.float32))
    shutil.copy(item.rgb, item.out_rgb)
    Image.fromarray(m == 0).save(item.out_mask)
    return item
if sys.argv[1] == "--serve":
    print("Ready", flush=True)
    for line in sys.stdin:
        run(line)
        print("Done " + pipeline.done_token(pipeline.parse_line(line)), flush=True)
else:
    for l in open(sys.argv[1]).read().splitlines():
        if l.strip(): run(l)
'''


def _retex_run(tmp_path, extra, worker):
    sys.path.insert(0, ROOT)
    import para_gen
    from test_pipeline_host import _tiny_tree
    inp, mdir = _tiny_tree(tmp_path, nframes=4, seqs=("a", "b"))
    fake, log = tmp_path / "fake_arap.py", tmp_path / "lines.log"
    fake.write_text(FAKE_WORKER % (ROOT, str(log)))
    outp = tmp_path / "out"
    own = "%s %s" % (sys.executable, osp.join(ROOT, "arap_deform.py"))
    flags = para_gen.parse(["--input", str(inp), "--output", str(outp), "--gpu", "0", "1", "--matches", str(mdir), "--worker", worker,
                            "--arap_bin", own, "--narap", "3", "--jobs", "2", "--retex"] + extra)
    flags.arap_bin = "%s %s" % (sys.executable, fake)          # (the flags are checked against this repository's driver)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        out = para_gen.main(flags)
    finally:
        os.chdir(cwd)
    return outp, out, [pipeline.parse_line(ln) for ln in log.read_text().splitlines()]


@pytest.mark.parametrize("worker,multseg,bg", [("serve", False, False), ("serve", True, True), ("batch", True, False)])
def test_para_gen_retex_with_a_stand_in_worker(tmp_path, worker, multseg, bg):
    extra = ["--multseg"] if multseg else []
    if bg:
        os.makedirs(tmp_path / "bgs")
        Image.fromarray(np.random.default_rng(1).integers(0, 256, (50, 80, 3)).astype(np.uint8)).save(tmp_path / "bgs" / "b.png")
        extra += ["--bg_dir", str(tmp_path / "bgs")]
    outp, out, lines = _retex_run(tmp_path, extra, worker)
    assert len(out) == 6                                                    # 2 sequences x 3 pairs
    tex = [it for it in lines if isinstance(it, pipeline.TexLine)]
    solves = [it for it in lines if isinstance(it, pipeline.SolveLine)]
    assert len(tex) == 6 and len(solves) == (12 if multseg else 6)
    # a tex line names the frame's solves (the stand-in refuses one whose flows are not written yet: the run got here)
    assert sorted(f for it in tex for _, f in it.layers) == sorted(s.flow for s in solves)
    assert all(len(it.layers) == len(it.tex) == (2 if multseg else 1) for it in tex)
    st = json.load(open(outp / "arap_stats.json"))
    assert st["tex_done"] == 6 and st["frames_done"] == 6
    twins = (outp / "all_files_tex.list").read_text().split("\n")
    assert len(twins) == 6
    for pair, twin in zip(out, twins):
        (rgb1, rgb2, flow), (t1, t2, tflow) = pair.split(" "), twin.split(" ")
        assert tflow == flow and all(osp.exists(q) for q in (t1, t2, tflow))          # the SAME flow file
        assert t1 == rgb1.replace(osp.sep + "inpRGB" + osp.sep, osp.sep + "inpRGB_tex" + osp.sep)
        assert t2 == rgb2.replace(osp.sep + "wRGB" + osp.sep, osp.sep + "wRGB_tex" + osp.sep)
        a, b = np.array(Image.open(rgb2).convert("RGB")), np.array(Image.open(t2).convert("RGB"))
        cover = np.array(Image.open(rgb2.replace(osp.sep + "wRGB" + osp.sep, osp.sep + "wMasks" + osp.sep))) != 0
        assert np.array_equal(a[~cover], b[~cover]) and (~cover).any()      # with --bg_dir: the pair's background
        assert (b[cover] == (1, 2, 3)).all() and not (a[cover] == (1, 2, 3)).all()
    if multseg:                                                             # per-segment files were merged and removed
        assert not [f for f in os.listdir(outp / "Flow" / "a") if "_seg" in f]
    # the same rng state gives the same layers: a line's textures are those of its pair's id
    import para_gen
    for it in tex:
        seq, stem = it.out["rgb1"].split(osp.sep)[-2], osp.splitext(osp.basename(it.out["rgb1"]))[0]
        assert list(it.tex) == pipeline.tex_layers(random.Random(para_gen._pair_id(seq, stem)), len(it.layers), (64, 40))


def test_para_gen_refuses_retex_with_in_between_frames(capsys):
    import helpers
    for extra in (["--mid", "2"], ["--multseg", "--mid_layers", "2"], ["--arap_bin", "/bin/true"]):
        with pytest.raises(SystemExit):
            helpers.para_gen_flags(["--retex"] + extra)
        assert "--retex" in capsys.readouterr().err
    assert helpers.para_gen_flags(["--retex"]).retex and not helpers.para_gen_flags([]).retex
