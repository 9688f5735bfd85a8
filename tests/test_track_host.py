"""Point tracks (DESIGN.md "Point tracks") at the host layer, no GPU: the numpy restatement of tests/track_ref.py against
the sequential statement of the definitions, its identity with the layered step at the integer pixels, a closed form,
the input conditions of every multi-layer GPU case, the track file format, the `trk` line in Python (pipeline.parse_trk)
and in C++ (host/list_line.h through line_tool), the point sampler and para_gen.py's --tracks flag."""
import os.path as osp
import random
import struct
import subprocess
import sys

import numpy as np
import pytest

import layers_step_ref as sref
import mid_ref
import occ_layers_ref as lref
import track_ref as tref
from arap_flow_amd import pipeline, trk
from helpers import para_gen_flags as _parse

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
F = np.float32
TINY = [c for c in sref.MULTI if c[0] * c[1] <= 96] + [(9, 8, 2, 3, False)] + sref.SINGLE


def _case(W, H, n, seed, overlap):
    _, masks, fa, fb = sref.two_state_layers(W, H, n, seed, overlap=overlap)
    return masks, np.stack([lref.fields_from_flows(fa), lref.fields_from_flows(fb)])


def _tiny_points(W, H, seed):
    """integer pixels, the quarter lattice thinned, random points, the borders, outside and NaN"""
    rng = np.random.default_rng(seed + 77)
    ys, xs = np.mgrid[0:4 * (H - 1) + 1, 0:4 * (W - 1) + 1]
    lat = np.stack([xs.ravel() / 4.0, ys.ravel() / 4.0], -1)
    lat = lat[rng.permutation(len(lat))[:60]]
    sub = np.stack([rng.uniform(0, W - 1, 40), rng.uniform(0, H - 1, 40)], -1)
    edge = np.array([[W - 1, (H - 1) / 2.0], [(W - 1) / 2.0, H - 1], [W - 1, H - 1]])
    bad = np.array([[-0.25, 0.0], [W - 0.75, 0.0], [0.0, H], [np.nan, 0.0], [0.0, np.inf]])
    return np.concatenate([tref.pixel_points(W, H), lat, sub, edge, bad]).astype(F)


@pytest.mark.parametrize("W,H,n,seed,overlap", TINY)
def test_restatement_equals_sequential_definitions(W, H, n, seed, overlap):
    assert W <= 12 and H <= 8 and n <= 4
    masks, fields = _case(W, H, n, seed, overlap)
    if W > 2 and H > 2:
        fields[1, n - 1, 2, 2] = (F(np.nan), F(1.0))             # a NaN position: its triangles hide nothing
    pts = _tiny_points(W, H, seed)
    a, b = tref.track_ref(masks, fields, pts), tref.track_brute(masks, fields, pts)
    assert a["pos"].tobytes() == b["pos"].tobytes()
    assert np.array_equal(a["occ"], b["occ"])
    bad = ~trk.in_frame(pts, W, H)
    assert bad.sum() == 5 and (a["occ"][:, bad] == 255).all()
    assert a["pos"][:, bad].tobytes() == np.stack([pts[bad]] * 2).tobytes()


@pytest.mark.parametrize("W,H,n,seed,overlap", sref.MULTI + sref.SINGLE)
def test_integer_pixels_equal_the_layered_step_from_the_grid(W, H, n, seed, overlap):
    masks, fields = _case(W, H, n, seed, overlap)
    grid = np.stack([mid_ref.grid_field(W, H)] * n)
    q = tref.pixel_points(W, H)
    r = tref.track_ref(masks, fields, q)
    for s in range(2):
        step = sref.layers_step_ref(masks, grid, fields[s])
        covered = step["warped_mask"].ravel() != 0
        assert np.array_equal(r["occ"][s], step["occlusion_step"].ravel())
        with np.errstate(invalid="ignore", over="ignore"):
            mine = r["pos"][s] - q
        assert mine[covered].tobytes() == step["step"].reshape(-1, 2)[covered].tobytes()
        assert r["pos"][s][~covered].tobytes() == q[~covered].tobytes()


@pytest.mark.parametrize("W,H,n,seed,overlap", sref.MULTI)
def test_multi_layer_cases_exercise_every_class(W, H, n, seed, overlap):
    """the input conditions of every multi-layer case of the GPU tests, from the restatement alone, at the integer
    points and for both states: visible owned, !in_frame, same-layer hit, higher-layer hit, background hit, background
    free -- counted as tref.class_counts states"""
    masks, fields = _case(W, H, n, seed, overlap)
    r = tref.track_ref(masks, fields, tref.pixel_points(W, H), parts=True)
    for s in range(2):
        counts = tref.class_counts(r, s)
        assert all(counts), (s, dict(zip(tref.CLASSES, counts)))
    if (W, H, n, seed) == (10, 8, 3, 3):                         # the smallest case
        assert tref.class_counts(r, 0) == [21, 34, 2, 16, 3, 8]


def _rectangles():
    masks, fa, fb, _ = sref.rectangles_case()
    pts = tref.rectangle_points()
    upper = (pts[:, 0] > 10) & (pts[:, 0] < 14) & (pts[:, 1] > 3) & (pts[:, 1] < 8)         # strictly inside
    upper_closed = (pts[:, 0] >= 10) & (pts[:, 0] <= 14) & (pts[:, 1] >= 3) & (pts[:, 1] <= 8)
    want = []
    for shift in ((-2.0, 0.0), (-6.0, -2.0)):
        x0, x1, y0, y1 = 10 + shift[0], 14 + shift[0], 3 + shift[1], 8 + shift[1]
        hidden = (pts[:, 0] >= x0) & (pts[:, 0] <= x1) & (pts[:, 1] >= y0) & (pts[:, 1] <= y1)
        want.append((np.array(shift, F), hidden))
    return masks, np.stack([fa, fb]), pts, upper, ~upper_closed, want


def check_rectangles(r, pts, upper, rest, want):
    """the closed form, shared with the GPU test"""
    for s, (shift, hidden) in enumerate(want):
        assert r["pos"][s][upper].tobytes() == (pts[upper] + shift).tobytes() and (r["occ"][s][upper] == 0).all()
        assert r["pos"][s][rest].tobytes() == pts[rest].tobytes()
        assert np.array_equal(r["occ"][s][rest] == 255, hidden[rest])
    assert set(np.unique(r["occ"])) <= {0, 255}


def test_upper_rectangle_moves_over_resting_lower_one():
    """closed form; the sequential statement confirms it on a thinned point set, the restatement on all of them"""
    masks, flows, pts, upper, rest, want = _rectangles()
    fields = np.stack([lref.fields_from_flows(f) for f in flows])
    assert upper.any() and rest.any() and all((h & rest).any() and (~h & rest).any() for _, h in want)
    check_rectangles(tref.track_ref(masks, fields, pts), pts, upper, rest, want)
    thin = np.arange(0, len(pts), 7)
    check_rectangles(tref.track_brute(masks, fields, pts[thin]), pts[thin], upper[thin], rest[thin],
                     [(sh, h[thin]) for sh, h in want])


def test_trk_round_trip_and_malformed_files(tmp_path):
    rng = np.random.default_rng(4)
    pos = rng.uniform(-2, 12, (3, 7, 2)).astype(F)
    pos[1, 2] = (np.nan, 1.0)
    occ = rng.choice([0, 255], (3, 7)).astype(np.uint8)
    p = str(tmp_path / "a.trk")
    trk.write(p, 10, 8, pos, occ)
    raw = open(p, "rb").read()
    assert raw[:4] == b"ATRK" and struct.unpack("<5i", raw[4:24]) == (1, 10, 8, 3, 7) and len(raw) == 24 + 9 * 21
    assert raw[24:24 + 8 * 21] == pos.astype("<f4").tobytes() and raw[24 + 8 * 21:] == occ.tobytes()
    r = trk.read(p)
    assert (r["W"], r["H"]) == (10, 8) and r["pos"].tobytes() == pos.tobytes() and np.array_equal(r["occ"], occ)
    # a points file: one frame, occ by in_frame
    q = str(tmp_path / "p.trk")
    trk.write(q, 10, 8, pos[1])
    r = trk.read(q)
    assert r["pos"].shape == (1, 7, 2) and r["pos"][0].tobytes() == pos[1].tobytes()
    assert np.array_equal(r["occ"][0] == 0, trk.in_frame(pos[1], 10, 8)) and r["occ"][0, 2] == 255
    for name, data, word in (("short", raw[:10], "truncated"), ("cut", raw[:-1], "truncated"),
                             ("long", raw + b"\0", "mis-sized"), ("magic", b"ATRX" + raw[4:], "not a track file"),
                             ("ver", raw[:4] + struct.pack("<i", 2) + raw[8:], "version"),
                             ("zero", raw[:20] + struct.pack("<i", 0) + raw[24:], "sizes"), ("empty", b"", "truncated")):
        bad = str(tmp_path / (name + ".trk"))
        open(bad, "wb").write(data)
        with pytest.raises(ValueError, match=word):
            trk.read(bad)
    with pytest.raises(ValueError):
        trk.write(p, 10, 8, pos, occ[:2])
    with pytest.raises(ValueError):
        trk.write(p, 10, 8, pos[..., :1])


# ---- the trk line: pipeline.parse_trk and host/list_line.h -------------------------------------------------------------
GOOD = ["trk P.trk 1 1 m f out=O.trk", "trk P.trk 2 3 m0 a1 a2 a3 m1 b1 b2 b3 out=dir/O.trk",
        "trk P.trk 1 9 m " + " ".join("f%d" % s for s in range(9)) + " out=O.trk",
        "trk P 255 1 " + " ".join("m%d f%d" % (l, l) for l in range(255)) + " out=O"]
BAD = ["trk", "trk P.trk", "trk P.trk 1", "trk P.trk 1 1 m f",                         # no output
       "trk P.trk 1 1 m f out=", "trk P.trk 1 1 m f out", "trk P.trk 1 1 m f occ=O.trk",      # empty, no `=`, another key
       "trk P.trk 1 1 m f out=O.trk extra", "trk P.trk 1 1 m f out=O.trk out=Q.trk",          # anything after out=
       "trk P.trk 1 1 m out=O.trk", "trk P.trk 2 3 m0 a1 a2 a3 m1 b1 b2 out=O.trk",           # a state file short
       "trk P.trk 1 2 m f out=O.trk g",                                                       # a token where a path is
       "trk P.trk 0 1 out=O.trk", "trk P.trk 256 1 m f out=O.trk", "trk P.trk 1 0 m out=O.trk",
       "trk P.trk 1 10 m " + " ".join("f%d" % s for s in range(10)) + " out=O.trk",           # T above the cap
       "trk P.trk x 1 m f out=O.trk", "trk P.trk 1 -1 m f out=O.trk", "trk P.trk 1.0 1 m f out=O.trk"]


def test_trk_line_round_trips():
    for text in GOOD:
        item = pipeline.parse_line(text)
        assert isinstance(item, pipeline.TrkLine) and pipeline.parse_trk(text.split()) == item
        assert pipeline.format_line(item) == text == pipeline.trk_line(item)
        assert pipeline.done_token(item) == text.split("out=")[1]
    item = pipeline.parse_line(GOOD[1])
    assert item == pipeline.TrkLine("P.trk", [("m0", ("a1", "a2", "a3")), ("m1", ("b1", "b2", "b3"))], "dir/O.trk")
    for text in BAD:
        with pytest.raises(ValueError):
            pipeline.parse_line(text)
    assert pipeline.LAYER_KEYS == ("occ", "bwd", "occ_bwd", "rgb2", "mask2", "mid")           # the other forms stay
    assert pipeline.EXTRA_KEYS == ("bwd", "occ", "occ_bwd", "mid", "diag", "fold")
    assert isinstance(pipeline.parse_line("trk.png m c f r w"), pipeline.SolveLine)           # the first WORD decides


@pytest.fixture(scope="module")
def bins():
    from arap_flow_amd import build
    return {osp.basename(o): o for o in build.build_host()}


def test_trk_line_parser_equals_python_twin(bins):
    """every line through line_tool in one process: a good one comes back as format_line(parse_line(line)) + its done
    token, a bad one as BAD after the grammar's own message -- and Python refuses exactly those"""
    corpus = GOOD + BAD
    r = subprocess.run([bins["line_tool"]], input="".join(c + "\n" for c in corpus), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")[:-1]
    got = [ln for ln in lines if not ln.startswith("Invalid")]
    assert len(got) == len(corpus)
    assert [ln for ln in lines if ln.startswith("Invalid")] == ["Invalid trk line: " + b for b in BAD]
    for line, g in zip(GOOD, got):
        item = pipeline.parse_line(line)
        assert g == pipeline.format_line(item) + " done=" + pipeline.done_token(item), line
    assert got[len(GOOD):] == ["BAD"] * len(BAD)


def test_arap_deform_refuses_a_bad_trk_line_before_any_gpu_call(bins, tmp_path):
    lst = tmp_path / "l.txt"
    lst.write_text("a b c d e f\n" + BAD[7] + "\n")
    r = subprocess.run([bins["arap_deform"], str(lst)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "Invalid trk line: " + BAD[7] + "\n"
    r = subprocess.run([sys.executable, osp.join(ROOT, "arap_deform.py"), str(lst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "trk line" in r.stdout


# ---- para_gen --tracks ------------------------------------------------------------------------------------------------
def test_sample_track_points_determinism_counts_and_range():
    W, H = 23, 17
    masks = np.full((2, H, W), 255, np.uint8)
    masks[0, 3:6, 4:9] = 0
    masks[1, 10:17, 20:23] = 0                                   # object up to the right and bottom border
    obj = (masks == 0).any(0)
    for P in (1, 2, 7, 64, 501):
        a = pipeline.sample_track_points(random.Random(5), P, W, H, masks)
        b = pipeline.sample_track_points(random.Random(5), P, W, H, masks)
        assert a.dtype == np.float32 and a.shape == (P, 2) and a.tobytes() == b.tobytes()
        assert trk.in_frame(a, W, H).all()
        near = a[(P + 1) // 2:]                                  # the rest: within half a pixel of an object pixel
        ix, iy = np.floor(near[:, 0] + 0.5).astype(int), np.floor(near[:, 1] + 0.5).astype(int)
        assert obj[np.clip(iy, 0, H - 1), np.clip(ix, 0, W - 1)].all()
    c = pipeline.sample_track_points(random.Random(6), 64, W, H, masks)
    assert c.tobytes() != a[:64].tobytes()
    first = pipeline.sample_track_points(random.Random(5), 501, W, H, masks)[:251]
    ix, iy = np.floor(first[:, 0] + 0.5).astype(int), np.floor(first[:, 1] + 0.5).astype(int)
    assert not obj[iy, ix].all()                                 # the first half is spread over the frame
    assert first[:, 0].min() < 2 and first[:, 0].max() > W - 3 and first[:, 1].min() < 2 and first[:, 1].max() > H - 3
    none = pipeline.sample_track_points(random.Random(5), 40, W, H, np.full((1, H, W), 255, np.uint8))
    assert trk.in_frame(none, W, H).all() and none[:, 0].max() > W / 2 and none[:, 1].max() > H / 2


def test_para_gen_tracks_flag(capsys):
    py = "%s %s" % (sys.executable, osp.join(ROOT, "arap_deform.py"))
    f = _parse(["--mid", "2", "--tracks", "64", "--arap_bin", py])
    assert f.tracks == 64 and f.mid_steps
    f = _parse(["--multseg", "--mid_layers", "2", "--tracks", "5", "--arap_bin", py])
    assert f.tracks == 5 and f.mid_layers_steps
    assert _parse(["--mid", "2", "--arap_bin", py]).tracks == 0
    for bad, word in ((["--tracks", "64"], "--mid K"), (["--multseg", "--tracks", "64"], "--mid K"),
                      (["--mid", "2", "--tracks", "0x"], "invalid int"), (["--mid", "2", "--tracks", "-1"], "2^24"),
                      (["--mid", "2", "--tracks", "16777217"], "2^24"),
                      (["--mid", "2", "--tracks", "8", "--bg_dir", "b", "--bg_motion", "--mid_bg"], "static"),
                      (["--mid", "2", "--tracks", "8", "--arap_bin", "/usr/bin/true"], "foreign")):
        with pytest.raises(SystemExit):
            _parse(bad + ([] if "--arap_bin" in bad else ["--arap_bin", py]))
        assert word in capsys.readouterr().err, bad
