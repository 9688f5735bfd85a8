"""The generator's side of the host pipeline: the arithmetic and the file-level merges of para_gen.py.

What the reference's Python 2 scripts do AROUND the hot path, written from their behaviour (the contract
each function states in its docstring), with the size / selection arithmetic as pure functions that tests/golden/host/
pins with hand-computed cases:
  cover_scale, fit_bg, add_bg            para_gen.py:36-61      (background compositing)
  fit_bg_window, bg_maps, bg_maps_seq    the camera of a `bg` line: moving background, per in-between frame (addition)
  tex_layers, sample_track_points, random_light    what para_gen draws for a `tex`, `trk`, `light` line (addition)
  parse_diag, merge_diag, pair_rejected, flatten_diag    the diag= / fold= files: fold diagnostics (addition)
  match_ok, valid_cnstr, filter_matches  para_gen.py:216-223,468-482
  resize_crop_geometry, scale_rotate     para_gen.py:253-291
  make_arap_path, replace_ext            para_gen.py:318-339
  merge_segments, flatten                para_gen.py:136-175    (--multseg: merge per-segment outputs by the warped masks)
  merge_backward, flatten_backward       --multseg merge of the backward flow / backward occlusion (addition)
The list line -- its forms, their text, the table of them -- is lines.py; what runs a line on the GPU is run_lines.py; a
score table's text is scores.py.  Their public names are re-exported here, so `pipeline.X` reaches all four files.
"""
import colorsys
import math
import os
import os.path as osp
import random as rn

import numpy as np
from PIL import Image

from . import flo
from .lines import (MAX_SNAPSHOTS, MAX_BLUR_SAMPLES, SEG_MAX_RADIUS, INTERP_MAX_TIMES, LIGHT_MAX_R, LIGHT_MAX_SHIFT, TEX_KINDS,      # noqa: F401
                    LAYERS_WORD, BG_WORD, TEX_WORD, TRK_WORD, BLUR_WORD, LIGHT_WORD, SEG_WORD, SCORE_WORD, TSCORE_WORD,
                    CHAIN_WORD, FSCORE_WORD, INTERP_WORD, LSCORE_WORD, MSCORE_WORD, EXTRA_KEYS, LAYER_KEYS, BG_IN_KEYS,
                    BG_OUT_KEYS, TEX_KEYS, BLUR_KEYS, LIGHT_KEYS, SEG_KEYS, SCORE_KEYS, FSCORE_KEYS,
                    Form, FORMS, FORM_OF, parse_line, format_line, done_token, read_list_items,
                    parse_mid, mid_token, mid_files, mid_layer_files, mid_bg_files, mid_steps,
                    SolveLine, parse_extra, extra_tokens, parse_solve, solve_line, LayersLine, parse_layers, layers_line,
                    BgLine, parse_bg, bg_line, bg_outputs, TexLayer, TexLine, parse_tex, tex_line,
                    TrkLine, parse_trk, trk_line, BlurLine, parse_blur, blur_line, blur_times, blur_maps,
                    LightFrame, LIGHT_NEUTRAL, light_frame_ok, light_is_neutral, LightLine, parse_light, light_line,
                    SegLine, parse_seg, seg_line, ScoreLine, parse_score, score_line, TScoreLine, parse_tscore, tscore_line,
                    ChainLine, parse_chain, chain_line, FScoreLine, parse_fscore, fscore_line,
                    LScoreLine, parse_lscore, lscore_line, MScoreLine, parse_mscore, mscore_line,
                    InterpLine, parse_interp, interp_line, interp_files, interp_times)
from .run_lines import (RUN, run_list, deform_list, batch_snapshots, warp_files, FILL_MIN, FILL_MAX,      # noqa: F401
                        run_layers, run_layers_mid, run_background, run_background_seq, run_texture, run_tracks, run_blur,
                        run_light, run_seg, run_score, run_tscore, run_chain, run_fscore, run_lscore, run_mscore, run_interp,
                        load_rgb, load_mask_red, save_mask, save_occ, seg_dist_png, dist_from_png, owner_flow,
                        DIAG_COUNTS, DIAG_FLOATS, format_diag)
# a score table's names, its file's text, pooling and metrics: scores.py.  (LSCORE_FIELDS here is a label row as its file
# writes it, 7 names; opt.LSCORE_FIELDS is the table's 8.)
from .scores import (SCORE_ROWS, SCORE_FIELDS, FSCORE_ROWS, FSCORE_FIELDS, TSCORE_MAX_FRAMES, TSCORE_CLASSES, TSCORE_X,      # noqa: F401
                     TSCORE_FIELDS, LSCORE_FRAME_FIELDS, LSCORE_FILE_FIELDS as LSCORE_FIELDS, MSCORE_MAX_THR, MSCORE_MATCH_FIELDS,
                     format_score, parse_score_file, add_scores, score_summary,
                     format_track_score, parse_track_score_file, add_track_scores, track_score_summary,
                     format_frame_score, parse_frame_score_file, add_frame_scores, frame_score_summary,
                     format_label_score, parse_label_score_file, add_label_scores, label_score_summary,
                     format_map_score, parse_map_score_file, add_map_scores, map_score_summary)

ARAP_BG = 255        # para_gen.py:30

_ANTIALIAS = getattr(Image, "LANCZOS", None) or Image.ANTIALIAS   # Image.ANTIALIAS of the reference's PIL


# ------------------------------------------------------------------------------------------------------
# what para_gen draws for a tex, trk or light line
# ------------------------------------------------------------------------------------------------------
TEX_CELL_MIN = 4.0           # pixels: a cell this small still survives the warp's resampling


def tex_layers(rng, n, frame_wh):
    """para_gen --retex: one TexLayer per segment, drawn from `rng` (a random.Random; the same state gives the same
    layers).  Per layer, in this order: the kind, the seed, the cell size in pixels -- log-uniform between TEX_CELL_MIN
    and a third of the frame's short side (at least TEX_CELL_MIN), so the pattern survives the warp and an object never
    comes out flat --, the rotation, the aspect ratio (bricks: 2 .. 3 cells wide; drawn for every kind), the offset in
    cells, the two parameters, and three colours (hue, saturation, value), in the spirit of the reference's random_color;
    c1 is redrawn while it equals c0.  The map is computed in double and rounded once to float32."""
    W, H = frame_wh
    hi = max(TEX_CELL_MIN, min(W, H) / 3.0)

    def colour():
        r, g, b = colorsys.hsv_to_rgb(rng.uniform(0, 1), rng.uniform(0, 1), rng.uniform(0.5, 1))
        return (int(r * 255 + 0.5), int(g * 255 + 0.5), int(b * 255 + 0.5))
    out = []
    for _ in range(n):
        kind = rng.randrange(len(TEX_KINDS))
        seed = rng.getrandbits(32)
        size = math.exp(rng.uniform(math.log(TEX_CELL_MIN), math.log(hi)))
        rot = rng.uniform(0, 2 * math.pi)
        aspect = rng.uniform(2, 3)
        ou, ov = rng.uniform(-8, 8), rng.uniform(-8, 8)
        q0, q1 = rng.uniform(0, 1), rng.uniform(0, 1)
        c0, c1, c2 = colour(), colour(), colour()
        while c1 == c0:
            c1 = colour()
        su = size * aspect if TEX_KINDS[kind] == "brick" else size
        co, si = math.cos(rot), math.sin(rot)
        m = (co / su, si / su, ou, -si / size, co / size, ov)
        p0 = p1 = 0.0
        if TEX_KINDS[kind] == "brick":
            p0, p1 = 0.04 + 0.08 * q0, 0.3 + 0.4 * q1       # mortar width, shift of odd rows
        elif TEX_KINDS[kind] == "wave":
            p0, p1 = 0.2 + 0.8 * q0, float(q1 >= 0.5)       # amplitude of the bend, triangle or saw
        f32 = lambda v: float(np.float32(v))
        out.append(TexLayer(kind, seed, tuple(f32(v) for v in m), f32(p0), f32(p1), c0, c1, c2))
    return out


def sample_track_points(rng, P, W, H, masks):
    """para_gen --tracks P: P query points of a W x H frame 1, float32 [P,2], drawn from `rng` (a random.Random; the same
    state gives the same points).  The first ceil(P / 2) are uniform over [0, W-1] x [0, H-1]; the rest are a uniformly
    chosen object pixel (the union of the layers: masks u8[n,H,W], 0 = object) plus a uniform offset in [-0.5, 0.5)^2,
    clipped to the frame; all are uniform over the frame when there is no object pixel."""
    obj = np.flatnonzero((np.asarray(masks) == 0).any(0).ravel())
    out = np.zeros((P, 2), np.float32)
    for k in range(P):
        if k < (P + 1) // 2 or not len(obj):
            x, y = rng.uniform(0, W - 1), rng.uniform(0, H - 1)
        else:
            i = int(obj[rng.randrange(len(obj))])
            x, y = i % W + (rng.random() - 0.5), i // W + (rng.random() - 0.5)
        out[k] = (min(max(x, 0.0), W - 1.0), min(max(y, 0.0), H - 1.0))      # (rounding to float32 stays in the frame)
    return out


LIGHT_TWIN_SHIFT = 1024      # cells: how far apart the fields of a seed and its twin lie (a power of two)


def _tex_mix(x, inverse=False):
    """the 32-bit mixer of the textures' hash (tex_mix of arap_tex.h), or its inverse: it is a bijection"""
    M = 0xffffffff
    if not inverse:
        x ^= x >> 16; x = x * 0x7feb352d & M; x ^= x >> 15; x = x * 0x846ca68b & M      # noqa: E702
        return x ^ x >> 16
    x ^= x >> 16; x = x * pow(0x846ca68b, -1, 1 << 32) & M; x ^= x >> 15 ^ x >> 30      # noqa: E702
    x = x * pow(0x7feb352d, -1, 1 << 32) & M
    return x ^ x >> 16


def light_twin_seed(seed):
    """the seed whose illumination field is `seed`'s moved by LIGHT_TWIN_SHIFT cells: the hash of lattice point (i, j),
    stream 0, is mix(mix(mix(seed) ^ i) ^ j), so with mix(twin) = mix(seed) ^ LIGHT_TWIN_SHIFT the twin's value at (i, j)
    is the seed's at (i + LIGHT_TWIN_SHIFT, j) for 0 <= i < LIGHT_TWIN_SHIFT.  The noise streams (seed + 1 .. seed + 12)
    of the two seeds have nothing in common.  A frame description has ONE seed, for its field and its noise: this is how
    the two frames of a pair see the same drifting light through different noise."""
    return _tex_mix(_tex_mix(seed & 0xffffffff) ^ LIGHT_TWIN_SHIFT, inverse=True)


def random_light(rng, strength, W, H):
    """para_gen --relight: the two LightFrames of a pair, drawn from `rng` (a random.Random; the same state gives the same
    pair), every amplitude scaled by `strength` >= 0; strength = 0 gives two neutral descriptions.  In this order: the
    seed; the field's cell size in pixels (log-uniform between half the frame's short side and twice its long side), its
    rotation and its drift between the frames in cells (each component within a quarter cell times min(strength, 1)); the
    field's amplitude; the vignette; per channel the gain of frame 1, then its flicker; the gamma of frame 1 and its flicker;
    the shadow's direction, distance, penumbra and depth; the two noise deviations.
    Shared by the two frames: the shadow's geometry and depth, the vignette, the field's amplitude, the noise deviations.
    Frame 2's seed is frame 1's twin (light_twin_seed) and its map is frame 1's moved by the drift minus LIGHT_TWIN_SHIFT
    cells: the same field a little further on -- the light drifts, it does not jump -- under different noise.  Frame 1's
    map puts the frame's centre at (1.5, 0.5) * LIGHT_TWIN_SHIFT, so both frames stay inside the range where the twin
    relation holds.  Maps are computed in double and rounded once to float32."""
    s = float(strength)
    if not (math.isfinite(s) and s >= 0):
        raise ValueError("random_light: a finite strength >= 0 expected")
    f32 = lambda v: float(np.float32(v))
    seed = rng.getrandbits(32)
    cell = math.exp(rng.uniform(math.log(max(1.0, min(W, H) / 2.0)), math.log(2.0 * max(W, H))))
    rot = rng.uniform(0, 2 * math.pi)
    du, dv = (rng.uniform(-0.25, 0.25) * min(s, 1.0) for _ in range(2))
    amp = min(0.3 * s * rng.uniform(0.3, 1), 0.9)
    vig = min(s * rng.uniform(0, 0.5), 1.0)
    gain1, gain2 = [], []
    for _ in range(3):
        g = min(max(1 + 0.1 * s * rng.uniform(-1, 1), 0.25), 4.0)
        gain1.append(f32(g))
        gain2.append(f32(min(max(g * (1 + 0.03 * s * rng.uniform(-1, 1)), 0.25), 4.0)))
    gamma1 = math.exp(0.2 * min(s, 4.0) * rng.uniform(-1, 1))
    gamma2 = gamma1 * min(max(1 + 0.03 * s * rng.uniform(-1, 1), 0.5), 2.0)
    ang, dist = rng.uniform(0, 2 * math.pi), rng.uniform(4, 24) * max(1.0, min(W, H) / 480.0)
    lim = lambda v: max(-LIGHT_MAX_SHIFT, min(int(round(v)), LIGHT_MAX_SHIFT))
    sh_dx, sh_dy = lim(dist * math.cos(ang)), lim(dist * math.sin(ang))
    sh_r = rng.randint(2, LIGHT_MAX_R)
    sh_g = min(int(round(s * rng.uniform(64, 160))), 256)
    sigma0, sigma1 = f32(s * rng.uniform(0.5, 3)), f32(s * rng.uniform(0, 0.02))
    co, si = math.cos(rot) / cell, math.sin(rot) / cell
    xc, yc = (W - 1) / 2.0, (H - 1) / 2.0
    cu, cv = 1.5 * LIGHT_TWIN_SHIFT - (co * xc + si * yc), 0.5 * LIGHT_TWIN_SHIFT - (-si * xc + co * yc)
    m1 = tuple(f32(v) for v in (co, si, cu, -si, co, cv))
    m2 = tuple(f32(v) for v in (co, si, cu + du - LIGHT_TWIN_SHIFT, -si, co, cv + dv))
    shared = (sh_dx, sh_dy, sh_r, sh_g, sigma0, sigma1)
    return (LightFrame(seed, m1, f32(amp), f32(vig), tuple(gain1), f32(gamma1), *shared),
            LightFrame(light_twin_seed(seed), m2, f32(amp), f32(vig), tuple(gain2), f32(gamma2), *shared))


# ------------------------------------------------------------------------------------------------------
# the diag file (run_lines.format_diag writes it)
# ------------------------------------------------------------------------------------------------------
def parse_diag(text):
    """the inverse of format_diag: {name: int or numpy float32}; anything but its eight lines is an error"""
    rows = [ln.split() for ln in text.splitlines()]
    if [r[0] if len(r) == 2 else None for r in rows] != list(DIAG_COUNTS + DIAG_FLOATS):
        raise ValueError("not a diag file: %r" % text)
    out = {k: int(v) for k, v in rows[:len(DIAG_COUNTS)]}
    out.update({k: np.float32(float(v)) for k, v in rows[len(DIAG_COUNTS):]})
    return out


def _bit_order(v):
    """a float32's place in the total order of the IEEE bit patterns (-0 < +0): the order of the statistics' extrema"""
    u = int(np.float32(v).view(np.uint32))
    return (u ^ 0xffffffff) if u >> 31 else (u | 0x80000000)


def merge_diag(stats, folds=None):
    """--multseg: the diagnostics of a frame's segments become the frame's: the counts are summed, the extrema combined
    in the order of the bit patterns (a segment without a value holds the identity: +inf, -inf, 0), and the fold maps
    OR-ed -- the segments' masks are disjoint.  Returns (stats, fold or None)."""
    stats = list(stats)
    out = {k: sum(int(q[k]) for q in stats) for k in DIAG_COUNTS}
    out["det_min"] = min([np.float32(q["det_min"]) for q in stats] + [np.float32(np.inf)], key=_bit_order)
    out["det_max"] = max([np.float32(q["det_max"]) for q in stats] + [np.float32(-np.inf)], key=_bit_order)
    out["disp2_max"] = max([np.float32(q["disp2_max"]) for q in stats] + [np.float32(0)], key=_bit_order)
    fold = None
    if folds is not None:
        fold = np.where(np.any([np.asarray(f) != 0 for f in folds], axis=0), 255, 0).astype(np.uint8)
    return out, fold


def pair_rejected(stats, max_fold):
    """para_gen --max_fold FRAC: a pair is rejected iff a triangle went non-finite or more than FRAC of them folded"""
    return stats["nonfinite"] > 0 or stats["folded"] > max_fold * stats["triangles"]


def flatten_diag(frame_line, seg_lines, remove=True):
    """merge_diag at file level: reads every segment's diag and fold files, writes the frame's, deletes the segments'"""
    ex = [ln.extra for ln in seg_lines]
    stats = [parse_diag(open(e["diag"]).read()) for e in ex]
    folds = [np.array(Image.open(e["fold"]).convert("L")) for e in ex] if "fold" in frame_line.extra else None
    merged, fold = merge_diag(stats, folds)
    with open(frame_line.extra["diag"], "w") as f:
        f.write(format_diag(merged))
    if fold is not None:
        save_occ(fold, frame_line.extra["fold"])
    if remove:
        for e in ex:
            for k in ("diag", "fold"):
                if k in e and osp.exists(e[k]):
                    os.remove(e[k])


# ------------------------------------------------------------------------------------------------------
# para_gen helpers
# ------------------------------------------------------------------------------------------------------
def cover_scale(bg_hw, im_hw, u):
    """Background compositing, size arithmetic (behaviour of /root/reference/para_gen.py:36-48): the background is
    enlarged by u (a draw from U(1, 2)) times the smallest factor that makes it cover the image in both directions
    (never shrunk below its own size); sizes truncate.  Returns the enlarged (height, width)."""
    (bh, bw), (ih, iw) = bg_hw, im_hw
    cover = max(max(bh, ih) / float(bh), max(bw, iw) / float(bw))
    return int(bh * (u * cover)), int(bw * (u * cover))


def fit_bg_window(bg, im, rng=rn):
    """The enlarged copy of `bg` and the (left, top) of a random window of it as large as `im`.  Three draws from `rng`,
    in this order (so that a seeded run picks the windows the reference would): the enlargement u = uniform(1, 2), then
    the window's top row and its left column, each randint over every position that keeps the window inside (both ends
    included)."""
    ih, iw = im.shape[:2]
    u = rng.uniform(1, 2)
    nh, nw = cover_scale(bg.shape[:2], (ih, iw), u)
    big = np.asarray(Image.fromarray(bg).resize((nw, nh), _ANTIALIAS))
    top = rng.randint(0, big.shape[0] - ih)
    left = rng.randint(0, big.shape[1] - iw)
    return big, (left, top)


def fit_bg(bg, im, rng=rn):
    """A random window of an enlarged copy of `bg`, as large as `im` (fit_bg_window's draws)."""
    ih, iw = im.shape[:2]
    big, (left, top) = fit_bg_window(bg, im, rng)
    return big[top:top + ih, left:left + iw, :]


BG_MOTION_PER_FD = (2.0, 0.01, 3.0)      # degrees, log-scale, pixels per frame of distance: SURVEY 8d's object motion


def _affine_compose(A, B):
    """A o B of two six-number affine maps (first B, then A), in float64"""
    a, b, c, d, e, f = A
    g, h, i, j, k, l = B
    return (a * g + b * j, a * h + b * k, a * i + b * l + c, d * g + e * j, d * h + e * k, d * i + e * l + f)


def bg_maps_seq(win_left, win_top, frame_wh, bg_wh, rng, fractions, fd=1, strength=1.0):
    """The sampling maps of a pair and of its in-between frames over the enlarged background (DESIGN.md "Moving
    background", "Moving background over in-between frames"): (M1, [M at each fraction], M2), float32 [6] each.  M1 is
    the window translation.  With S(tau) the similarity about the frame centre with rotation tau x rot, log-scale tau x
    lsc and shift tau x (sx, sy), the frame at fraction tau gets M1 o S(tau) and M2 = M1 o S(1); rot, lsc, sx, sy are
    drawn from `rng` in this order, uniformly within strength x BG_MOTION_PER_FD x fd.  While a frame corner maps outside
    [0, bgW - 1] x [0, bgH - 1] under any map of the sequence the parameters are halved, up to 8 times; then every map
    is M1."""
    W, H = frame_wh
    bw, bh = bg_wh
    M1 = (1.0, 0.0, float(win_left), 0.0, 1.0, float(win_top))
    lim = [strength * fd * v for v in BG_MOTION_PER_FD]
    rot, lsc = rng.uniform(-lim[0], lim[0]), rng.uniform(-lim[1], lim[1])
    sx, sy = rng.uniform(-lim[2], lim[2]), rng.uniform(-lim[2], lim[2])
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    taus = [float(t) for t in fractions] + [1.0]

    def inside(cand):
        m = cand.astype(np.float64)
        corners = [(m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]) for x in (0, W - 1) for y in (0, H - 1)]
        return all(0 <= px <= bw - 1 and 0 <= py <= bh - 1 for px, py in corners)
    found = None
    for _ in range(9):
        cands = []
        for tau in taus:
            t, sc = np.deg2rad(tau * rot), np.exp(tau * lsc)
            a, b = sc * np.cos(t), sc * np.sin(t)
            S = (a, -b, cx - a * cx + b * cy + tau * sx, b, a, cy - b * cx - a * cy + tau * sy)
            cands.append(np.asarray(_affine_compose(M1, S), np.float32))
        if all(inside(c) for c in cands):
            found = cands
            break
        rot, lsc, sx, sy = rot / 2, lsc / 2, sx / 2, sy / 2
    M1 = np.asarray(M1, np.float32)
    if found is None:
        found = [M1.copy() for _ in taus]
    return M1, found[:-1], found[-1]


def bg_maps(win_left, win_top, frame_wh, bg_wh, rng, fd=1, strength=1.0):
    """The sampling maps (M1, M2) of a pair over the enlarged background (DESIGN.md "Moving background"), float32 [6]
    each: bg_maps_seq without an in-between frame.  M1 is the window translation.  M2 = M1 o S with S a similarity about
    the frame centre: rotation, log-scale and a shift in x and y, drawn from `rng` in this order, uniformly within
    strength x BG_MOTION_PER_FD x fd.  While a frame corner maps outside [0, bgW - 1] x [0, bgH - 1] the parameters are
    halved, up to 8 times; then M2 = M1."""
    M1, _, M2 = bg_maps_seq(win_left, win_top, frame_wh, bg_wh, rng, (), fd, strength)
    return M1, M2


def add_bg(im, mk, bgim, bgval=0):
    """Composite: pixels whose mask value equals `bgval` come from `bgim`, all others from `im`
    (/root/reference/para_gen.py:50-61).  `im` and `bgim` are (H, W, C) of one shape, `mk` is (H, W)."""
    if im.ndim != 3 or mk.shape != im.shape[:2]:
        raise AssertionError("Sizes mismatch mask and image %s vs. %s" % (mk.shape, im.shape[:-1]))
    if bgim.shape != im.shape:
        raise AssertionError("Sizes mismatch background and image %s vs. %s" % (bgim.shape, im.shape))
    return np.where((mk == bgval)[..., None], bgim, im).astype(im.dtype, copy=False)


MAX_MATCH_DIST = 60          # a match moves less than this many pixels ...


def match_ok(xy1, xy2, msk1, msk2):
    """Which matches become constraints (/root/reference/para_gen.py:216-223)?  xy1, xy2: integer arrays (n, 2) of
    (x, y) in the first / second frame.  A match is kept when both ends lie inside their label masks, it moves by more
    than nothing and by less than MAX_MATCH_DIST pixels (Euclidean; compared as squared integers, which is the same
    predicate), its source lies on a segment (label > 0) and both ends carry the same label.  Returns a bool array.
    (Negative coordinates are rejected here; the reference would index from the far edge, which no matcher output
    can mean.)"""
    xy1 = np.asarray(xy1, np.int64).reshape(-1, 2)
    xy2 = np.asarray(xy2, np.int64).reshape(-1, 2)
    (h1, w1), (h2, w2) = msk1.shape[:2], msk2.shape[:2]
    inside = ((xy1 >= 0).all(1) & (xy2 >= 0).all(1) &
              (xy1[:, 0] < w1) & (xy1[:, 1] < h1) & (xy2[:, 0] < w2) & (xy2[:, 1] < h2))
    d2 = ((xy2 - xy1) ** 2).sum(1)
    keep = inside & (d2 > 0) & (d2 < MAX_MATCH_DIST ** 2)
    lab1 = np.zeros(len(xy1), msk1.dtype)
    lab2 = np.zeros(len(xy1), msk2.dtype)
    lab1[inside] = msk1[xy1[inside, 1], xy1[inside, 0]]
    lab2[inside] = msk2[xy2[inside, 1], xy2[inside, 0]]
    return keep & (lab1 > 0) & (lab1 == lab2)


def valid_cnstr(x1, y1, x2, y2, msk1, msk2):
    """one match (the reference's call shape, para_gen.py:216-223)"""
    return bool(match_ok([(x1, y1)], [(x2, y2)], msk1, msk2)[0])


def filter_matches(match_lines, mk1, mk2):
    """para_gen.py:468-482: the matcher's lines `x1 y1 x2 y2 score index` -> (constraint rows, label of each kept row),
    in the matcher's order"""
    rows = []
    for line in match_lines:
        tok = line.split()
        if len(tok) >= 4:
            rows.append([int(float(t)) for t in tok[:4]])
    if not rows:
        return [], []
    a = np.asarray(rows, np.int64)
    keep = match_ok(a[:, 0:2], a[:, 2:4], mk1, mk2)
    kept = a[keep]
    return [tuple(int(v) for v in r) for r in kept], [int(mk1[r[1], r[0]]) for r in kept]


def write_constraints(path, cstrs):
    """para_gen.py:476-479: count, then tab-separated x1 y1 x2 y2 rows"""
    with open(path, "w") as f:
        f.write("\n".join([str(len(cstrs))] + ["\t".join("%d" % v for v in c) for c in cstrs]))


def resize_crop_geometry(in_size, out_size, margin=10):
    """Frame preparation, size arithmetic (behaviour of /root/reference/para_gen.py:275-287).  in_size, out_size:
    (width, height).  The frame is scaled by the one factor that makes it at least `margin` pixels larger than the
    target in both directions (sizes truncate) and the target window is cut around the centre: left = floor(w / 2) -
    floor(target_w / 2), likewise the top.  Returns ((w, h), (left, upper, right, lower))."""
    (iw, ih), (ow, oh) = in_size, out_size
    r = max((ow + margin) / float(iw), (oh + margin) / float(ih))
    w, h = int(iw * r), int(ih * r)
    left, upper = w // 2 - ow // 2, h // 2 - oh // 2
    return (w, h), (left, upper, left + ow, upper + oh)


def _is_jpeg(path):
    ext = osp.splitext(path)[1].upper()
    return "JPG" in ext or "JPEG" in ext


def scale_rotate(im_path, mk_path, size=None):
    """Open a frame and its label mask and bring them to the working format (/root/reference/para_gen.py:253-291):
    portrait frames are transposed to landscape; with a target `size` (w, h) every frame of another size is scaled
    (image: antialiased, mask: nearest neighbour) and centre-cropped by resize_crop_geometry.  Returns (changed, image,
    mask) as PIL images; `changed` is also true for JPEG inputs, which the caller then re-encodes as PNG."""
    im, mk = Image.open(im_path), Image.open(mk_path)
    if im.size != mk.size:
        raise AssertionError("Image and mask must be of the same size but given %s vs. %s" % (im.size, mk.size))
    changed = _is_jpeg(im_path) or _is_jpeg(mk_path)
    if im.height > im.width:
        im, mk = (x.transpose(Image.TRANSPOSE) for x in (im, mk))
        changed = True
    if size is not None and tuple(im.size) != tuple(size):
        new_size, box = resize_crop_geometry(im.size, tuple(size))
        im = im.resize(new_size, _ANTIALIAS).crop(box)
        mk = mk.resize(new_size, Image.NEAREST).crop(box)
        changed = True
    return changed, im, mk


EXTRA_OF = dict(bwd_gen="bwd", occbwd_gen="occ_bwd", occ_gen="occ",   # para_gen's path key -> list-line token
                diag_gen="diag", fold_gen="fold")


def make_arap_path(p):
    """para_gen.py:331-339: the list-file line of one solve, from para_gen's path table of the pair (or segment)"""
    six = [osp.abspath(p[k]) for k in ("rgb1_gen", "msk1_gen", "cstr_tmp", "flow_gen", "rgb2_gen", "msk2_gen")]
    extra = {t: p[k] for k, t in EXTRA_OF.items() if k in p}
    if "mid_gen" in p:                          # --mid: the prefix of the pair's in-between files, steps in "_mid"
        extra["mid"] = mid_token(p["_mid"], p["mid_gen"])
    return SolveLine(*six, extra=extra)


def replace_ext(dict_path, seg_num, keep_orgs=()):
    """para_gen.py:318-329"""
    out = {}
    for k, v in dict_path.items():
        fn, ext = osp.splitext(v)
        out[k] = v if k in keep_orgs else "%s_seg%d%s" % (fn, seg_num, ext)
    return out


def split_segments(mk1, valid_labels):
    """--multseg (para_gen.py:518-540): one inverted mask per label that has at least one constraint"""
    out = []
    for s in np.unique(valid_labels):
        if s == 0:
            continue
        mask = np.zeros_like(mk1, dtype=np.uint8) + ARAP_BG
        mask[mk1 == s] = 0
        out.append((int(s), mask))
    return out


def merge_segments(flows, rgbs, masks):
    """--multseg: the per-segment results of one frame, stacked (segment, H, W, ...), become one result: at every pixel
    the LAST segment after the first whose warped mask is set wins, and the first segment fills the rest
    (/root/reference/para_gen.py:136-175, which folds the segments in with `old * (mask == 0) + new * (mask != 0)`: the
    same selection, up to the sign of a zero flow and non-finite values under a cleared mask)."""
    masks = np.asarray(masks)
    n = masks.shape[0]
    on = masks != 0
    on[0] = True                                               # the first segment is the base layer
    winner = (n - 1) - np.argmax(on[::-1], axis=0)             # last segment with its mask set
    pick = winner[None, ...]
    flow = np.take_along_axis(np.asarray(flows), pick[..., None], axis=0)[0]
    rgb = np.take_along_axis(np.asarray(rgbs), pick[..., None], axis=0)[0]
    mask = np.take_along_axis(masks, pick, axis=0)[0]
    return flow, rgb, mask


def flatten(arap_seg_paths, remove=True):
    """para_gen.py:136-175 at file level: for every (frame SolveLine, [segment SolveLines]) read the segments' flow /
    warped RGB / warped mask files, merge them (merge_segments), write the frame's three files, delete the segments'
    files.  Returns the frames' lines."""
    for frame_line, seg_lines in arap_seg_paths:
        if len(seg_lines) == 0:
            raise AssertionError("Something wrong with seg_paths")
        files = [(ln.flow, ln.out_rgb, ln.out_mask) for ln in seg_lines]
        flows = [flo.flow_read(f) for f, _, _ in files]
        rgbs = [np.asarray(Image.open(r)) for _, r, _ in files]
        rgbs = [a[..., None] if a.ndim == 2 else a for a in rgbs]
        masks = [np.asarray(Image.open(m)) for _, _, m in files]
        flow, rgb, mask = merge_segments(flows, rgbs, masks)
        if remove:
            for trio in files:
                for q in trio:
                    os.remove(q)
        flo.flow_write(frame_line.flow, flow)
        Image.fromarray(rgb.astype(np.uint8).squeeze()).save(frame_line.out_rgb)
        # (a 1-bit mask file comes out 0 / 1 valued, as in the reference)
        Image.fromarray(mask.astype(np.uint8)).save(frame_line.out_mask)
    return [e[0] for e in arap_seg_paths]


def merge_backward(bwds, covers, objects):
    """--multseg: the per-segment backward flows (segment, H, W, 2) of one frame become one, exactly: at every pixel the
    LAST segment whose warped mask covers it wins (the top layer, as merge_segments picks the warped RGB); where no
    segment covers it the flow is 0 and the backward occlusion is 255 if the pixel was object in frame 1 in any
    segment.  covers, objects: (segment, H, W) bool.  Returns (backward flow, backward occlusion u8 0/255)."""
    covers = np.asarray(covers, bool)
    n = covers.shape[0]
    any_cover = covers.any(0)
    winner = (n - 1) - np.argmax(covers[::-1], axis=0)
    bwd = np.take_along_axis(np.asarray(bwds, np.float32), winner[None, ..., None], axis=0)[0]
    bwd[~any_cover] = 0
    occ_bwd = np.where(~any_cover & np.asarray(objects, bool).any(0), 255, 0).astype(np.uint8)
    return bwd, occ_bwd


def flatten_backward(frame_line, seg_lines, remove=True):
    """merge_backward at file level, before flatten removes the segments' warped masks: reads every segment's backward
    flow, warped mask and frame-1 mask (red channel 0 = object), writes the files named in the frame line's `extra` and
    deletes the segments' backward files."""
    covers = [np.asarray(Image.open(ln.out_mask)) != 0 for ln in seg_lines]
    objects = [load_mask_red(ln.mask) == 0 for ln in seg_lines]
    bwds = [flo.flow_read(ln.extra["bwd"]) for ln in seg_lines]
    bwd, occ_bwd = merge_backward(bwds, covers, objects)
    if "bwd" in frame_line.extra:
        flo.flow_write(frame_line.extra["bwd"], bwd)
    if "occ_bwd" in frame_line.extra:
        save_occ(occ_bwd, frame_line.extra["occ_bwd"])
    if remove:
        for ln in seg_lines:
            for q in ln.extra.values():
                if osp.exists(q):
                    os.remove(q)
