"""Python 3 host side of the dataset generator, over libarapopt.so.

What the reference's Python 2 scripts and C++ drivers do AROUND the hot path, written from their
behaviour (the contract each function states in its docstring), with the size / selection arithmetic as pure
functions that tests/golden/host/ pins with hand-computed cases:
  SolveLine, parse_line, format_line, done_token, read_list_items    the list line: a solve (6 paths, optional output
                            tokens bwd= occ= occ_bwd= mid= diag= fold=) or the `layers` line, the layered warp of one frame (addition)
  format_diag, parse_diag, merge_diag, pair_rejected    the diag= / fold= tokens: fold diagnostics (addition)
  parse_mid, mid_token, mid_files, mid_steps    the mid= token: in-between frames from the constraint ramp (addition)
  mid_layer_files, owner_flow, run_layers_mid   a layers line's mid= token: layered in-between frames (addition)
  deform_list, run_layers   ARAP/deformation/src/main.cpp:162-241  (arap_deform over a list)
  warp_files                ARAP/warping/src/main.cpp:302-336      (warp_image)
  cover_scale, fit_bg, add_bg            para_gen.py:36-61      (background compositing)
  BgLine, parse_bg, bg_line, run_background, fit_bg_window, bg_maps    the `bg` line: moving background (addition)
  mid_bg_files, bg_maps_seq, run_background_seq    its mid= / mm= / mid_out= tokens: the camera per in-between frame (addition)
  TexLayer, TexLine, parse_tex, tex_line, tex_layers, run_texture    the `tex` line: the random-texture twin (addition)
  blur_times, blur_maps                  the schedule of a motion-blurred frame (addition)
  BlurLine, parse_blur, blur_line, run_blur    the `blur` line: the motion-blurred frames of a pair (addition)
  LightFrame, LightLine, parse_light, light_line, random_light, run_light    the `light` line: the relit pair (addition)
  SegLine, parse_seg, seg_line, run_seg  the `seg` line: object index maps, motion boundaries, boundary distance (addition)
  ScoreLine, parse_score, score_line, run_score    the `score` line: the error table of an estimated flow (addition)
  format_score, parse_score_file, score_summary, add_scores, dist_from_png    a score table as text, as metrics, pooled
  TrkLine, parse_trk, trk_line, sample_track_points, run_tracks    the `trk` line: point tracks of a sequence (addition)
  TScoreLine, parse_tscore, tscore_line, run_tscore    the `tscore` line: the TAP-Vid table of an estimated track file (addition)
  ChainLine, parse_chain, chain_line, run_chain    the `chain` line: an estimated track file from per-link flows (addition)
  format_track_score, parse_track_score_file, track_score_summary, add_track_scores    a track score table as text, as metrics, pooled
  FScoreLine, parse_fscore, fscore_line, run_fscore    the `fscore` line: the PSNR / SSIM table of an estimated frame (addition)
  format_frame_score, parse_frame_score_file, frame_score_summary, add_frame_scores    a frame score table as text, as metrics, pooled
  LScoreLine, parse_lscore, lscore_line, run_lscore    the `lscore` line: the DAVIS J / F table of an estimated label map (addition)
  MScoreLine, parse_mscore, mscore_line, run_mscore    the `mscore` line: the precision / recall table of an estimated map (addition)
  format_label_score, parse_label_score_file, label_score_summary, add_label_scores    a label score table as text, as metrics, pooled
  format_map_score, parse_map_score_file, map_score_summary, add_map_scores    a map score as text, as metrics, pooled
  InterpLine, parse_interp, interp_line, run_interp    the `interp` line: in-between frames from a flow estimate (addition)
  merge_segments, flatten                para_gen.py:136-175    (--multseg: merge per-segment outputs by the warped masks)
  merge_backward, flatten_backward       --multseg merge of the backward flow / backward occlusion (addition)
  match_ok, valid_cnstr, filter_matches  para_gen.py:216-223,468-482
  resize_crop_geometry, scale_rotate     para_gen.py:253-291
  make_arap_path, replace_ext            para_gen.py:318-339
No oracle import; the solve and the rasteriser run on the GPU through arap_flow_amd.opt.
"""
import colorsys
import math
import os
import os.path as osp
import random as rn
import re
from typing import NamedTuple, Optional

import numpy as np
from PIL import Image

from . import flo
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
# arap_deform
# ------------------------------------------------------------------------------------------------------
# A list line is the unit of work between para_gen.py, arap_deform.py and `arap_deform --serve` (C++ twin: parse_item in
# host/arap_deform.cpp).  It is a solve line, SolveLine, a `layers` line, the dict of parse_layers, a `bg` line, BgLine, or a
# `tex` line, TexLine, or a `trk` line, TrkLine;
# parse_line reads any of them from text, format_line writes it back, done_token is the path a worker reports it done by.
EXTRA_KEYS = ("bwd", "occ", "occ_bwd", "mid", "diag", "fold")
MAX_SNAPSHOTS = 8            # ARAPFLOW_MAX_SNAPSHOTS of include/arap_opt.h
LAYERS_WORD = "layers"
LAYER_KEYS = ("occ", "bwd", "occ_bwd", "rgb2", "mask2", "mid")
BG_WORD = "bg"
BG_IN_KEYS = ("occ", "bwd", "occ_bwd")                               # optional object-side inputs of a bg line
BG_OUT_KEYS = ("occ_out", "bwd_out", "occ_bwd_out")                  # the full maps made from them
TEX_WORD = "tex"
TEX_KEYS = ("rgb1", "rgb2", "mask2")
TEX_KINDS = ("checker", "brick", "voronoi", "noise", "wave")         # ARAPFLOW_TEX_*: a kind's number is its index
TRK_WORD = "trk"
BLUR_WORD = "blur"
BLUR_KEYS = ("rgb1", "rgb2", "alpha1", "alpha2")
LIGHT_WORD = "light"
SEG_WORD = "seg"
SEG_KEYS = ("idx1", "idx2", "mb1", "mb2", "dist1", "dist2")
SEG_MAX_RADIUS = 254         # ARAPFLOW_SEG_MAX_RADIUS of include/arap_opt.h
SCORE_WORD = "score"
SCORE_KEYS = ("occ", "dist", "skip", "mask")
FSCORE_WORD = "fscore"
FSCORE_KEYS = ("occ", "dist", "skip", "obj")
INTERP_WORD = "interp"
LSCORE_WORD = "lscore"
MSCORE_WORD = "mscore"
INTERP_MAX_TIMES = 32        # ARAPFLOW_INTERP_MAX_TIMES of include/arap_opt.h
TSCORE_WORD = "tscore"
CHAIN_WORD = "chain"
LIGHT_KEYS = ("rgb1", "rgb2")


class SolveLine(NamedTuple):
    """main.cpp:183-191: one solve per line, six whitespace-separated paths
        rgb mask constraints out_flow out_rgb out_mask [bwd=PATH.flo] [occ=PATH.png] [occ_bwd=PATH.png] [mid=I1,I2,..:PREFIX]
                                                       [diag=PATH.txt] [fold=PATH.png]
    `extra`: the optional outputs the line asks for, {key: path} (parse_extra); the value of `mid` is the token's text
    after the `=` (parse_mid)"""
    rgb: str
    mask: str
    constraints: str
    flow: str
    out_rgb: str
    out_mask: str
    extra: dict


def parse_mid(value):
    """the value of a mid= token, I1,I2,..:PREFIX (DESIGN.md "In-between frames") -> (steps, prefix): 1 to MAX_SNAPSHOTS
    strictly increasing ramp-step indices >= 1 and the path prefix of the files of mid_files"""
    idx, colon, prefix = value.partition(":")
    try:
        steps = tuple(int(t) for t in idx.split(","))
    except ValueError:
        steps = ()
    if not (colon and prefix and 1 <= len(steps) <= MAX_SNAPSHOTS and steps[0] >= 1 and
            all(a < b for a, b in zip(steps, steps[1:]))):
        raise ValueError("bad mid= token %r: mid=I1,I2,..:PREFIX with 1 <= I1 < I2 < .., at most %d" % (value, MAX_SNAPSHOTS))
    return steps, prefix


def mid_token(steps, prefix):
    """the inverse of parse_mid"""
    return "%s:%s" % (",".join("%d" % i for i in steps), prefix)


def mid_files(prefix, step):
    """the four files of the snapshot after ramp step `step`: its flow from frame 1, the in-between frame and its mask
    (formats of a line's own flow, warped RGB and warped mask) and the flow from it to the next state"""
    stem = "%s_s%02d" % (prefix, step)
    return dict(flow=stem + ".flo", rgb=stem + ".png", mask=stem + "_mask.png", step=stem + "_step.flo")


def mid_layer_files(prefix, step):
    """the files a `layers` line's mid= token writes BESIDE mid_files' four: `occ`, the occlusion of the link that
    starts at the snapshot after ramp step `step` (DESIGN.md "Layered in-between frames"); step 0 is frame 1 itself,
    the link frame 1 -> first snapshot"""
    return dict(occ="%s_s%02d_occ.png" % (prefix, step))


def mid_bg_files(prefix, step):
    """the files a `bg` line's mid_out= token writes (DESIGN.md "Moving background over in-between frames"): `rgb`, the
    in-between frame after ramp step `step` with the moving background behind it (steps >= 1); `step`, the full-frame
    flow of the link that starts at that frame, and `occ`, that link's full-frame occlusion (step 0 is frame 1 itself)"""
    stem = "%s_s%02d" % (prefix, step)
    return dict(rgb=stem + ".png", step=stem + "_step.flo", occ=stem + "_occ.png")


def mid_steps(K, num_iter):
    """para_gen --mid K: K ramp steps spread evenly over the ramp, (i * num_iter) // (K + 1) for i = 1 .. K; they must be
    distinct and >= 1 (19 and K = 3: 4, 9, 14)"""
    K, num_iter = int(K), int(num_iter)
    steps = [(i * num_iter) // (K + 1) for i in range(1, K + 1)]
    if not 1 <= K <= MAX_SNAPSHOTS or min(steps) < 1 or len(set(steps)) != K:
        raise ValueError("--mid %d: 1 .. %d distinct steps of a ramp of %d are needed" % (K, MAX_SNAPSHOTS, num_iter))
    return steps


def parse_extra(tokens):
    """optional tokens after a line's paths: bwd=PATH.flo, occ=PATH.png, occ_bwd=PATH.png, mid=I1,I2,..:PREFIX,
    diag=PATH.txt, fold=PATH.png (DESIGN.md "Fold diagnostics") -> {key: value}.  Any other token is ignored (a line's tokens after the sixth always were); a malformed mid= token is
    an error (parse_mid)."""
    out = {}
    for t in tokens:
        k, eq, v = t.partition("=")
        if eq and k in EXTRA_KEYS and v:
            if k == "mid":
                parse_mid(v)
            out[k] = v
    return out


def extra_tokens(extra):
    """the inverse of parse_extra, in a fixed order"""
    return ["%s=%s" % (k, extra[k]) for k in EXTRA_KEYS if extra.get(k)]


def parse_layers(tokens):
    """a `layers` line (DESIGN.md "Layered warp"), recognised by its first word:
        layers RGB n MASK_1 FLO_1 ... MASK_n FLO_n [occ=P] [bwd=P] [occ_bwd=P] [rgb2=P] [mask2=P] [mid=I1,I2,..:PREFIX]
    -> dict(rgb, layers=[(mask, flo)] in layer order (the later on top), out={key: path} in line order).  At least one
    output; anything else after the layers is an error (a new line form has no old meaning to keep)."""
    if len(tokens) < 3 or tokens[0] != LAYERS_WORD:
        raise ValueError("not a layers line: %r" % " ".join(tokens))
    try:
        n = int(tokens[2])
    except ValueError:
        raise ValueError("layers line: layer count expected, got %r" % tokens[2])
    if not 1 <= n <= 255 or len(tokens) < 3 + 2 * n:
        raise ValueError("layers line: 1..255 layers, a mask and a flow each: %r" % " ".join(tokens))
    out = {}
    for t in tokens[3 + 2 * n:]:
        k, eq, v = t.partition("=")
        if not (eq and k in LAYER_KEYS and v):
            raise ValueError("layers line: bad output token %r" % t)
        if k == "mid":
            parse_mid(v)
        out[k] = v
    if not out:
        raise ValueError("layers line without an output: %r" % " ".join(tokens))
    return dict(rgb=tokens[1], layers=[(tokens[3 + 2 * l], tokens[4 + 2 * l]) for l in range(n)], out=out)


def layers_line(rgb, layers, out):
    """the inverse of parse_layers; outputs in the order of LAYER_KEYS"""
    tok = [LAYERS_WORD, rgb, str(len(layers))] + [p for pair in layers for p in pair]
    return " ".join(tok + ["%s=%s" % (k, out[k]) for k in LAYER_KEYS if out.get(k)])


class BgLine(NamedTuple):
    """a `bg` line (DESIGN.md "Moving background"), recognised by its first word: the full-frame pass of one pair
        bg BG.png RGB1.png MASK1.png RGB2.png MASK2.png FLOW.flo m=<12 numbers> [mid=I1,..,In:PREFIX mm=<6n numbers>]
           [occ=IN] [bwd=IN] [occ_bwd=IN] out=RGB1_OUT.png,RGB2_OUT.png,FLOW_OUT.flo [occ_out=..] [bwd_out=..]
           [occ_bwd_out=..] [mid_out=PREFIX_OUT]
    MASK1: the solver's mask (red 0 = object); MASK2: a warped mask (non-zero = object).  `m`: M1 then M2, twelve
    float32 written with %.9g, comma separated.  `out`: three paths, any of them empty (not wanted).  `inputs` / `outs`:
    {key: path} over BG_IN_KEYS / BG_OUT_KEYS; an output needs its input.  At least one output.
    `mid`, `mm`, `mid_out` (DESIGN.md "Moving background over in-between frames"), all three or none: the text of a mid=
    token (parse_mid) naming the pair's in-between files (mid_files, and with occ= the link occlusions of
    mid_layer_files), the sampling maps of the n in-between frames (6n float32, as `m`), and the prefix of the files of
    mid_bg_files that the sequence pass writes."""
    bg: str
    rgb1: str
    mask1: str
    rgb2: str
    mask2: str
    flow: str
    m: tuple
    inputs: dict
    out: tuple
    outs: dict
    mid: str = ""
    mm: tuple = ()
    mid_out: str = ""


def _bg_numbers(text):
    try:
        return tuple(float(np.float32(float(q))) for q in text.split(","))
    except ValueError:
        return ()


def parse_bg(tokens):
    if len(tokens) < 7 or tokens[0] != BG_WORD:
        raise ValueError("not a bg line: %r" % " ".join(tokens))
    m, out, inputs, outs = None, ("", "", ""), {}, {}
    mid, mm, mid_out = "", None, ""
    for t in tokens[7:]:
        k, eq, v = t.partition("=")
        if not (eq and v):
            raise ValueError("bg line: bad token %r" % t)
        if k == "m":
            m = _bg_numbers(v)
            if len(m) != 12:
                raise ValueError("bg line: m= takes 12 numbers, M1 then M2: %r" % t)
        elif k == "mid":
            parse_mid(v)
            mid = v
        elif k == "mm":
            mm = _bg_numbers(v)
        elif k == "mid_out":
            mid_out = v
        elif k == "out":
            out = tuple(v.split(","))
            if len(out) != 3:
                raise ValueError("bg line: out= takes RGB1_OUT,RGB2_OUT,FLOW_OUT (a place may be empty): %r" % t)
        elif k in BG_IN_KEYS:
            inputs[k] = v
        elif k in BG_OUT_KEYS:
            outs[k] = v
        else:
            raise ValueError("bg line: bad token %r" % t)
    if m is None:
        raise ValueError("bg line without m=: %r" % " ".join(tokens))
    for k in outs:
        if k[:-len("_out")] not in inputs:
            raise ValueError("bg line: %s= needs %s=" % (k, k[:-len("_out")]))
    if mid or mm is not None or mid_out:
        if not (mid and mm is not None and mid_out):
            raise ValueError("bg line: mid=, mm= and mid_out= come together: %r" % " ".join(tokens))
        if len(mm) != 6 * len(parse_mid(mid)[0]):
            raise ValueError("bg line: mm= takes six numbers per index of mid=: %r" % " ".join(tokens))
    if not any(out) and not outs and not mid_out:
        raise ValueError("bg line without an output: %r" % " ".join(tokens))
    return BgLine(*tokens[1:7], m=m, inputs=inputs, out=out, outs=outs, mid=mid, mm=mm or (), mid_out=mid_out)


def bg_line(item):
    """the inverse of parse_bg; optional tokens in the order mid=, mm=, BG_IN_KEYS, out=, BG_OUT_KEYS, mid_out="""
    tok = [BG_WORD] + list(item[:6]) + ["m=" + ",".join("%.9g" % v for v in item.m)]
    if item.mid:
        tok += ["mid=" + item.mid, "mm=" + ",".join("%.9g" % v for v in item.mm)]
    tok += ["%s=%s" % (k, item.inputs[k]) for k in BG_IN_KEYS if item.inputs.get(k)]
    if any(item.out):
        tok.append("out=" + ",".join(item.out))
    tok += ["%s=%s" % (k, item.outs[k]) for k in BG_OUT_KEYS if item.outs.get(k)]
    return " ".join(tok + (["mid_out=" + item.mid_out] if item.mid_out else []))


def bg_outputs(item):
    """every file a bg line writes, in the fixed order out= (three places), then BG_OUT_KEYS, then those of mid_out=:
    the in-between frames, the link flows (frame 1's first), and with occ= the link occlusions"""
    files = [q for q in item.out if q] + [item.outs[k] for k in BG_OUT_KEYS if item.outs.get(k)]
    if item.mid_out:
        steps = parse_mid(item.mid)[0]
        files += [mid_bg_files(item.mid_out, i)["rgb"] for i in steps]
        files += [mid_bg_files(item.mid_out, i)["step"] for i in (0,) + steps]
        if "occ" in item.inputs:
            files += [mid_bg_files(item.mid_out, i)["occ"] for i in (0,) + steps]
    return files


class TexLayer(NamedTuple):
    """one layer's procedural texture (ArapFlow_TexLayer, DESIGN.md "Random textures"): kind, a number (index of
    TEX_KINDS); seed, 32 bits; m, six float32 (pixel -> texture point); p0, p1 float32; c0, c1, c2, RGB bytes"""
    kind: int
    seed: int
    m: tuple
    p0: float
    p1: float
    c0: tuple
    c1: tuple
    c2: tuple


class TexLine(NamedTuple):
    """a `tex` line (DESIGN.md "Random textures"), recognised by its first word: the random-texture twin of one frame
        tex RGB1 n MASK_1 FLO_1 ... MASK_n FLO_n t=<layer 1>;...;<layer n> [rgb1=P] [rgb2=P] [mask2=P]
    The layers are those of the frame's `layers` line (the later on top).  A layer of t= is 19 numbers, comma separated:
    kind, seed, the six of m, p0, p1 (floats written with %.9g), then the nine palette bytes c0, c1, c2.  rgb1: the
    retextured frame 1; rgb2 / mask2: its layered warp with the layers' flows.  `out`: {key: path} in line order.  At
    least one output; anything else -- an unknown or repeated key, a missing `=`, an empty value, a wrong count of numbers
    -- is an error."""
    rgb: str
    layers: list
    tex: tuple
    out: dict


_UINT = re.compile(r"[0-9]{1,10}$")


def _tex_layer(text):
    q = text.split(",")
    if len(q) != 19 or not all(_UINT.match(v) for v in q[:2] + q[10:]):
        return None
    ints = [int(v) for v in q[:2] + q[10:]]
    with np.errstate(over="ignore"):            # (a number beyond float32 becomes inf, refused below)
        fl = _bg_numbers(",".join(q[2:10]))
    if len(fl) != 8 or not all(math.isfinite(v) for v in fl):
        return None
    if ints[0] >= len(TEX_KINDS) or ints[1] > 0xffffffff or max(ints[2:]) > 255:
        return None
    return TexLayer(ints[0], ints[1], fl[:6], fl[6], fl[7], tuple(ints[2:5]), tuple(ints[5:8]), tuple(ints[8:11]))


def parse_tex(tokens):
    if len(tokens) < 3 or tokens[0] != TEX_WORD:
        raise ValueError("not a tex line: %r" % " ".join(tokens))
    try:
        n = int(tokens[2]) if _UINT.match(tokens[2]) else 0
    except ValueError:
        n = 0
    if not 1 <= n <= 255 or len(tokens) < 3 + 2 * n:
        raise ValueError("tex line: 1..255 layers, a mask and a flow each: %r" % " ".join(tokens))
    out, tex = {}, None
    for t in tokens[3 + 2 * n:]:
        k, eq, v = t.partition("=")
        if not (eq and v and (k == "t" or k in TEX_KEYS)) or k in out or (k == "t" and tex is not None):
            raise ValueError("tex line: bad or repeated token %r" % t)
        if k == "t":
            tex = tuple(_tex_layer(q) for q in v.split(";"))
            if len(tex) != n or None in tex:
                raise ValueError("tex line: t= takes %d layers of 19 numbers: %r" % (n, t))
        else:
            out[k] = v
    if tex is None:
        raise ValueError("tex line without t=: %r" % " ".join(tokens))
    if not out:
        raise ValueError("tex line without an output: %r" % " ".join(tokens))
    return TexLine(tokens[1], [(tokens[3 + 2 * l], tokens[4 + 2 * l]) for l in range(n)], tex, out)


def tex_line(item):
    """the inverse of parse_tex: t=, then the outputs in the order of TEX_KEYS"""
    tok = [TEX_WORD, item.rgb, str(len(item.layers))] + [p for pair in item.layers for p in pair]
    nums = lambda q: ["%d" % q.kind, "%d" % q.seed] + ["%.9g" % float(np.float32(v)) for v in tuple(q.m) + (q.p0, q.p1)] + \
        ["%d" % c for c in tuple(q.c0) + tuple(q.c1) + tuple(q.c2)]
    tok.append("t=" + ";".join(",".join(nums(q)) for q in item.tex))
    return " ".join(tok + ["%s=%s" % (k, item.out[k]) for k in TEX_KEYS if item.out.get(k)])


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


def run_texture(state, spec):
    """one `tex` line: read the frame's RGB and every layer's mask (and, for rgb2 / mask2, flow) once, one opt.texture
    and, if rgb2 or mask2 is wanted, one opt.warp_layers on its result; write what the line asks for (rgb1, rgb2: RGB
    PNG; mask2: 1-bit PNG as a solve's warped mask)"""
    from . import opt
    rgb = load_rgb(spec.rgb)
    masks = np.stack([load_mask_red(m) for m, _ in spec.layers])
    if masks.shape[1:] != rgb.shape[:2]:
        raise ValueError("tex line: image and mask sizes differ")
    out = spec.out
    rgb1 = opt.texture(state, rgb, masks, spec.tex)
    if "rgb1" in out:
        Image.fromarray(rgb1).save(out["rgb1"])
    if "rgb2" in out or "mask2" in out:
        flows = np.stack([flo.flow_read(f) for _, f in spec.layers])
        if flows.shape[1:3] != rgb.shape[:2]:
            raise ValueError("tex line: image and flow sizes differ")
        r = opt.warp_layers(state, rgb1, masks, flows, occ=False)
        if "rgb2" in out:
            Image.fromarray(r["warped_rgb"]).save(out["rgb2"])
        if "mask2" in out:
            save_mask(r["warped_mask"], out["mask2"])


class TrkLine(NamedTuple):
    """a `trk` line (DESIGN.md "Point tracks"), recognised by its first word: the tracks of the points of one file
    through the T states of the n layers of a frame
        trk PTS.trk n T  MASK_1 FLO_1,1 .. FLO_1,T  ..  MASK_n FLO_n,1 .. FLO_n,T  out=OUT.trk
    PTS.trk: a points file (trk.py, one frame); every state file of every layer is named, in the order of the sequence
    (the later layer on top); OUT.trk has T + 1 frames, the points first.  `layers`: [(mask, (flo_1, .., flo_T))].  Any
    other token is an error."""
    points: str
    layers: list
    out: str


def parse_trk(tokens):
    if len(tokens) < 4 or tokens[0] != TRK_WORD:
        raise ValueError("not a trk line: %r" % " ".join(tokens))
    n, T = (int(t) if _UINT.match(t) else 0 for t in tokens[2:4])
    if not (1 <= n <= 255 and 1 <= T <= MAX_SNAPSHOTS + 1):
        raise ValueError("trk line: 1..255 layers and 1..%d states: %r" % (MAX_SNAPSHOTS + 1, " ".join(tokens)))
    end = 4 + n * (T + 1)
    if len(tokens) != end + 1:
        raise ValueError("trk line: %d layers of a mask and %d flows, then out=: %r" % (n, T, " ".join(tokens)))
    k, eq, v = tokens[end].partition("=")
    if not (k == "out" and eq and v):
        raise ValueError("trk line: bad output token %r" % tokens[end])
    if any("=" in t for t in tokens[1:end]):
        raise ValueError("trk line: a path expected where a token is: %r" % " ".join(tokens))
    at = lambda l: 4 + l * (T + 1)
    return TrkLine(tokens[1], [(tokens[at(l)], tuple(tokens[at(l) + 1:at(l) + 1 + T])) for l in range(n)], v)


def trk_line(item):
    """the inverse of parse_trk"""
    tok = [TRK_WORD, item.points, str(len(item.layers)), str(len(item.layers[0][1]))]
    for mask, flows in item.layers:
        tok += [mask] + list(flows)
    return " ".join(tok + ["out=" + item.out])


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


def run_tracks(state, spec):
    """one `trk` line: read the points, every layer's mask and its T state flows, one opt.track_points, write the track
    file: frame 0 the points themselves (occ by in_frame), frames 1 .. T the states"""
    from . import opt, trk
    pts = trk.read(spec.points)
    if pts["pos"].shape[0] != 1:
        raise ValueError("trk line: %s is no points file (%d frames)" % (spec.points, pts["pos"].shape[0]))
    masks = np.stack([load_mask_red(m) for m, _ in spec.layers])
    H, W = masks.shape[1:]
    if (pts["W"], pts["H"]) != (W, H):
        raise ValueError("trk line: points and mask sizes differ")
    T = len(spec.layers[0][1])
    flows = np.stack([np.stack([flo.flow_read(fl[s]) for _, fl in spec.layers]) for s in range(T)])
    if flows.shape[2:4] != (H, W):
        raise ValueError("trk line: mask and flow sizes differ")
    r = opt.track_points(state, masks, flows, pts["pos"][0])
    first = np.where(trk.in_frame(pts["pos"][0], W, H), 0, 255).astype(np.uint8)
    trk.write(spec.out, W, H, np.concatenate([pts["pos"], r["pos"]]), np.concatenate([first[None], r["occ"]]))


MAX_BLUR_SAMPLES = 32        # ARAPFLOW_MAX_BLUR_SAMPLES of include/arap_opt.h


def blur_times(centre, shutter, samples):
    """the sample times of an exposure window (ArapFlow_BlurSchedule, DESIGN.md "Motion blur"), float32 [samples]:
    t_k = centre + shutter * ((k + 0.5) / samples - 0.5), in double from the float32 values of centre and shutter, rounded
    once to float32"""
    c, e = float(np.float32(centre)), float(np.float32(shutter))
    if not 1 <= samples <= MAX_BLUR_SAMPLES or not (math.isfinite(c) and math.isfinite(e) and e >= 0):
        raise ValueError("blur: 1 .. %d samples, a finite centre, a finite shutter >= 0 expected" % MAX_BLUR_SAMPLES)
    return np.array([c + e * ((k + 0.5) / samples - 0.5) for k in range(samples)], np.float64).astype(np.float32)


def blur_maps(times, Ma, Mb):
    """the sampling map of every sample (ArapFlow_BlurSchedule), float32 [samples, 6]: u * Ma + t * Mb per coefficient
    with u = 1 - t, every operation in float32; Ma itself for every sample when Ma and Mb are bit-equal (a still camera)"""
    Ma, Mb = (np.ascontiguousarray(m, np.float32).reshape(-1) for m in (Ma, Mb))
    if Ma.shape != (6,) or Mb.shape != (6,) or not (np.isfinite(Ma).all() and np.isfinite(Mb).all()):
        raise ValueError("blur: two maps of six finite numbers expected")
    t = np.asarray(times, np.float32)[:, None]
    if Ma.tobytes() == Mb.tobytes():
        return np.repeat(Ma[None], len(t), 0)
    with np.errstate(over="ignore", invalid="ignore"):
        return ((np.float32(1.0) - t) * Ma[None] + t * Mb[None]).astype(np.float32)


class BlurLine(NamedTuple):
    """a `blur` line (DESIGN.md "Motion blur"), recognised by its first word: the two motion-blurred frames of one pair
        blur RGB1 n MASK_1 FLO_1 ... MASK_n FLO_n BG.png b=<shutter>,<samples> [m=<12 numbers: M1 then M2>]
             [rgb1=P] [rgb2=P] [alpha1=P] [alpha2=P]
    The layers are those of the frame's `layers` line (the later on top); BG.png shows behind them.  b=: the shutter, a
    finite float32 >= 0 written with %.9g, and the sample count, 1 .. MAX_BLUR_SAMPLES.  m=: the camera at frame 1 and at
    frame 2 as in a bg line, twelve finite float32 written with %.9g (`m` empty: both the identity).  rgb1 / alpha1: the
    frame exposed around t = 0; rgb2 / alpha2: around t = 1.  `out`: {key: path} in line order.  At least one output;
    anything else -- an unknown or repeated key, a missing `=`, an empty value, a wrong count of numbers -- is an error."""
    rgb: str
    layers: list
    bg: str
    shutter: float
    samples: int
    m: tuple
    out: dict


def parse_blur(tokens):
    if len(tokens) < 3 or tokens[0] != BLUR_WORD:
        raise ValueError("not a blur line: %r" % " ".join(tokens))
    n = int(tokens[2]) if _UINT.match(tokens[2]) else 0
    if not 1 <= n <= 255 or len(tokens) < 4 + 2 * n:
        raise ValueError("blur line: 1..255 layers, a mask and a flow each, then the background: %r" % " ".join(tokens))
    if any("=" in t for t in tokens[1:4 + 2 * n]):
        raise ValueError("blur line: a path expected where a token is: %r" % " ".join(tokens))
    out, b, m = {}, None, None
    for t in tokens[4 + 2 * n:]:
        k, eq, v = t.partition("=")
        if not (eq and v and k in ("b", "m") + BLUR_KEYS) or k in out or (k == "b" and b is not None) or (k == "m" and m is not None):
            raise ValueError("blur line: bad or repeated token %r" % t)
        if k == "b":
            e, _, count = v.partition(",")
            with np.errstate(over="ignore"):
                e = _bg_numbers(e)
            if len(e) != 1 or not (math.isfinite(e[0]) and e[0] >= 0) or not _UINT.match(count) or not 1 <= int(count) <= MAX_BLUR_SAMPLES:
                raise ValueError("blur line: b= takes a shutter >= 0 and 1..%d samples: %r" % (MAX_BLUR_SAMPLES, t))
            b = (e[0], int(count))
        elif k == "m":
            with np.errstate(over="ignore"):
                m = _bg_numbers(v)
            if len(m) != 12 or not all(math.isfinite(q) for q in m):
                raise ValueError("blur line: m= takes 12 finite numbers, M1 then M2: %r" % t)
        else:
            out[k] = v
    if b is None:
        raise ValueError("blur line without b=: %r" % " ".join(tokens))
    if not out:
        raise ValueError("blur line without an output: %r" % " ".join(tokens))
    return BlurLine(tokens[1], [(tokens[3 + 2 * l], tokens[4 + 2 * l]) for l in range(n)], tokens[3 + 2 * n], b[0], b[1],
                    m or (), out)


def blur_line(item):
    """the inverse of parse_blur: b=, m= if the line has maps, then the outputs in the order of BLUR_KEYS"""
    tok = [BLUR_WORD, item.rgb, str(len(item.layers))] + [p for pair in item.layers for p in pair] + [item.bg]
    tok.append("b=%.9g,%d" % (float(np.float32(item.shutter)), item.samples))
    if len(item.m):
        tok.append("m=" + ",".join("%.9g" % float(np.float32(v)) for v in item.m))
    return " ".join(tok + ["%s=%s" % (k, item.out[k]) for k in BLUR_KEYS if item.out.get(k)])


def run_blur(state, spec):
    """one `blur` line: read the frame's RGB, every layer's mask and flow and the background picture once, one
    opt.blur_layers per frame the line asks for (rgb1 / alpha1: centre 0, rgb2 / alpha2: centre 1), write the outputs (rgb:
    RGB PNG; alpha: 8-bit L PNG)"""
    from . import opt
    rgb, bg = load_rgb(spec.rgb), load_rgb(spec.bg)
    masks = np.stack([load_mask_red(m) for m, _ in spec.layers])
    flows = np.stack([flo.flow_read(f) for _, f in spec.layers])
    if masks.shape[1:] != rgb.shape[:2] or flows.shape[1:3] != rgb.shape[:2]:
        raise ValueError("blur line: image, mask and flow sizes differ")
    maps = (spec.m[:6], spec.m[6:]) if len(spec.m) else None
    for frame, centre in (("1", 0.0), ("2", 1.0)):
        want = tuple(k for k in ("rgb", "alpha") if k + frame in spec.out)
        if not want:
            continue
        r, a = opt.blur_layers(state, rgb, masks, flows, centre, spec.shutter, spec.samples, bg=bg, maps=maps, want=want)
        if r is not None:
            Image.fromarray(r).save(spec.out["rgb" + frame])
        if a is not None:
            save_occ(a, spec.out["alpha" + frame])


LIGHT_MAX_R, LIGHT_MAX_SHIFT = 16, 64      # ARAPFLOW_LIGHT_MAX_R, ARAPFLOW_LIGHT_MAX_SHIFT of include/arap_opt.h


class LightFrame(NamedTuple):
    """one frame's light (ArapFlow_LightFrame, DESIGN.md "Relit frames"), 19 numbers in this order: seed, 32 bits; m, six
    float32 (pixel -> field point); amp >= 0; vig, 0 .. 1; gain, three float32 > 0; gamma > 0; sh_dx, sh_dy, integers of
    magnitude <= LIGHT_MAX_SHIFT; sh_r, 0 .. LIGHT_MAX_R; sh_g, 0 .. 256; sigma0, sigma1 >= 0; every float finite"""
    seed: int
    m: tuple
    amp: float
    vig: float
    gain: tuple
    gamma: float
    sh_dx: int
    sh_dy: int
    sh_r: int
    sh_g: int
    sigma0: float
    sigma1: float


LIGHT_NEUTRAL = LightFrame(0, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0), 0.0, 0.0, (1.0, 1.0, 1.0), 1.0, 0, 0, 0, 0, 0.0, 0.0)


def light_frame_ok(q):
    """whether a LightFrame lies in the ranges ArapFlow_LightTables accepts"""
    fl = tuple(q.m) + (q.amp, q.vig) + tuple(q.gain) + (q.gamma, q.sigma0, q.sigma1)
    if len(q.m) != 6 or len(q.gain) != 3 or not all(math.isfinite(v) for v in fl):
        return False
    if not (0 <= q.seed <= 0xffffffff and q.amp >= 0 and 0 <= q.vig <= 1 and min(q.gain) > 0 and q.gamma > 0):
        return False
    if not (q.sigma0 >= 0 and q.sigma1 >= 0 and abs(q.sh_dx) <= LIGHT_MAX_SHIFT and abs(q.sh_dy) <= LIGHT_MAX_SHIFT):
        return False
    return 0 <= q.sh_r <= LIGHT_MAX_R and 0 <= q.sh_g <= 256


def light_is_neutral(q):
    """whether a LightFrame returns its input bytes: no field, no vignette, the identity tone curve, no shadow, no noise"""
    return (q.amp, q.vig, tuple(q.gain), q.gamma, q.sh_g, q.sigma0, q.sigma1) == (0, 0, (1, 1, 1), 1, 0, 0, 0)


class LightLine(NamedTuple):
    """a `light` line (DESIGN.md "Relit frames"), recognised by its first word: the relit variant of one pair
        light RGB1 MASK1 RGB2 COVER2 l=<frame 1>;<frame 2> [rgb1=P] [rgb2=P]
    RGB1 / RGB2: the pair's finished frames; MASK1: frame 1's mask in the solver's convention (red channel, object: == 0);
    COVER2: frame 2's warped mask, read as a cover (red channel, object: != 0).  A frame of l= is the 19 numbers of
    LightFrame, comma separated: the seed, sh_dx, sh_dy, sh_r and sh_g integers, the floats written with %.9g.  rgb1 /
    rgb2: the relit frames.  `out`: {key: path} in line order.  At least one output; anything else -- an unknown or
    repeated key, a missing `=`, an empty value, a wrong count of numbers, a number out of range or non-finite -- is an
    error."""
    rgb1: str
    mask1: str
    rgb2: str
    cover2: str
    frames: tuple
    out: dict


_INT = re.compile(r"-?[0-9]{1,10}$")


def _light_frame(text):
    q = text.split(",")
    if len(q) != 19 or not _UINT.match(q[0]) or not all(_INT.match(v) for v in q[13:15]) or not all(_UINT.match(v) for v in q[15:17]):
        return None
    with np.errstate(over="ignore"):            # (a number beyond float32 becomes inf, refused below)
        fl = _bg_numbers(",".join(q[1:13] + q[17:]))
    if len(fl) != 14:
        return None
    f = LightFrame(int(q[0]), fl[:6], fl[6], fl[7], fl[8:11], fl[11], int(q[13]), int(q[14]), int(q[15]), int(q[16]), fl[12], fl[13])
    return f if light_frame_ok(f) else None


def parse_light(tokens):
    if not tokens or tokens[0] != LIGHT_WORD:
        raise ValueError("not a light line: %r" % " ".join(tokens))
    if len(tokens) < 5 or any("=" in t for t in tokens[1:5]):
        raise ValueError("light line: two frames, a mask and a cover, then the tokens: %r" % " ".join(tokens))
    out, frames = {}, None
    for t in tokens[5:]:
        k, eq, v = t.partition("=")
        if not (eq and v and (k == "l" or k in LIGHT_KEYS)) or k in out or (k == "l" and frames is not None):
            raise ValueError("light line: bad or repeated token %r" % t)
        if k == "l":
            frames = tuple(_light_frame(q) for q in v.split(";"))
            if len(frames) != 2 or None in frames:
                raise ValueError("light line: l= takes two frames of 19 numbers in their ranges: %r" % t)
        else:
            out[k] = v
    if frames is None:
        raise ValueError("light line without l=: %r" % " ".join(tokens))
    if not out:
        raise ValueError("light line without an output: %r" % " ".join(tokens))
    return LightLine(tokens[1], tokens[2], tokens[3], tokens[4], frames, out)


def light_line(item):
    """the inverse of parse_light: l=, then the outputs in the order of LIGHT_KEYS"""
    f32 = lambda v: "%.9g" % float(np.float32(v))
    nums = lambda q: ["%d" % q.seed] + [f32(v) for v in tuple(q.m) + (q.amp, q.vig) + tuple(q.gain) + (q.gamma,)] + \
        ["%d" % v for v in (q.sh_dx, q.sh_dy, q.sh_r, q.sh_g)] + [f32(q.sigma0), f32(q.sigma1)]
    tok = [LIGHT_WORD, item.rgb1, item.mask1, item.rgb2, item.cover2, "l=" + ";".join(",".join(nums(q)) for q in item.frames)]
    return " ".join(tok + ["%s=%s" % (k, item.out[k]) for k in LIGHT_KEYS if item.out.get(k)])


def run_light(state, spec):
    """one `light` line: read the frame(s) the line asks for with their masks, one opt.relight each (rgb1: frame 1 under
    the first description, MASK1 in the solver's convention; rgb2: frame 2 under the second, COVER2 as a cover), write the
    outputs as RGB PNGs"""
    from . import opt
    for key, rgb_path, mask_path, frame, is_mask in (("rgb1", spec.rgb1, spec.mask1, spec.frames[0], True),
                                                     ("rgb2", spec.rgb2, spec.cover2, spec.frames[1], False)):
        if key not in spec.out:
            continue
        rgb, cover = load_rgb(rgb_path), load_mask_red(mask_path)
        if cover.shape != rgb.shape[:2]:
            raise ValueError("light line: image and mask sizes differ")
        Image.fromarray(opt.relight(state, rgb, cover, frame, cover_is_mask=is_mask)).save(spec.out[key])


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


class SegLine(NamedTuple):
    """a `seg` line (DESIGN.md "Segment maps"), recognised by its first word: the segment maps of one pair
        seg n MASK_1 FLO_1 ... MASK_n FLO_n s=<tau>,<radius> [m=<12 numbers: M1 then M2>]
            [idx1=P] [idx2=P] [mb1=P] [mb2=P] [dist1=P] [dist2=P]
    The layers are those of the frame's `layers` line (the later on top).  s=: the jump threshold tau, a finite float32
    >= 0 written with %.9g, and the radius, 0 .. SEG_MAX_RADIUS.  m=: the camera at frame 1 and at frame 2 as in a bg line,
    twelve finite float32 written with %.9g (`m` empty: a static background).  `out`: {key: path} in line order; every
    file is an 8-bit L PNG: idx the raw label, mb 0 / 255, dist the integer square root of the squared distance and 255
    for "further than the radius".  At least one output; anything else -- an unknown or repeated key, a missing `=`, an
    empty value, a wrong count of numbers, a non-finite number, a negative tau, a radius above SEG_MAX_RADIUS -- is an
    error."""
    layers: list
    tau: float
    radius: int
    m: tuple
    out: dict


def parse_seg(tokens):
    if len(tokens) < 2 or tokens[0] != SEG_WORD:
        raise ValueError("not a seg line: %r" % " ".join(tokens))
    n = int(tokens[1]) if _UINT.match(tokens[1]) else 0
    if not 1 <= n <= 255 or len(tokens) < 2 + 2 * n:
        raise ValueError("seg line: 1..255 layers, a mask and a flow each: %r" % " ".join(tokens))
    if any("=" in t for t in tokens[2:2 + 2 * n]):
        raise ValueError("seg line: a path expected where a token is: %r" % " ".join(tokens))
    out, s, m = {}, None, None
    for t in tokens[2 + 2 * n:]:
        k, eq, v = t.partition("=")
        if not (eq and v and k in ("s", "m") + SEG_KEYS) or k in out or (k == "s" and s is not None) or (k == "m" and m is not None):
            raise ValueError("seg line: bad or repeated token %r" % t)
        if k == "s":
            tau, _, radius = v.partition(",")
            with np.errstate(over="ignore"):
                tau = _bg_numbers(tau)
            if len(tau) != 1 or not (math.isfinite(tau[0]) and tau[0] >= 0) or not _UINT.match(radius) or int(radius) > SEG_MAX_RADIUS:
                raise ValueError("seg line: s= takes a tau >= 0 and a radius 0..%d: %r" % (SEG_MAX_RADIUS, t))
            s = (tau[0], int(radius))
        elif k == "m":
            with np.errstate(over="ignore"):
                m = _bg_numbers(v)
            if len(m) != 12 or not all(math.isfinite(q) for q in m):
                raise ValueError("seg line: m= takes 12 finite numbers, M1 then M2: %r" % t)
        else:
            out[k] = v
    if s is None:
        raise ValueError("seg line without s=: %r" % " ".join(tokens))
    if not out:
        raise ValueError("seg line without an output: %r" % " ".join(tokens))
    return SegLine([(tokens[2 + 2 * l], tokens[3 + 2 * l]) for l in range(n)], s[0], s[1], m or (), out)


def seg_line(item):
    """the inverse of parse_seg: s=, m= if the line has maps, then the outputs in the order of SEG_KEYS"""
    tok = [SEG_WORD, str(len(item.layers))] + [p for pair in item.layers for p in pair]
    tok.append("s=%.9g,%d" % (float(np.float32(item.tau)), item.radius))
    if len(item.m):
        tok.append("m=" + ",".join("%.9g" % float(np.float32(v)) for v in item.m))
    return " ".join(tok + ["%s=%s" % (k, item.out[k]) for k in SEG_KEYS if item.out.get(k)])


def seg_dist_png(d2):
    """a distance map as its file shows it: the integer square root of the uint16 squared distance, 255 for the sentinel
    65535 (isqrt(65535) = 255; every other value is <= 254^2)"""
    # (exact: the float64 root of an integer below 2^16 is an integer or at least 2^-9 away from one)
    return np.floor(np.sqrt(np.asarray(d2, np.uint16).astype(np.float64))).astype(np.uint8)


def run_seg(state, spec):
    """one `seg` line: read every layer's mask and flow, one opt.seg_maps for the outputs the line asks for, write them as
    8-bit L PNGs (SegLine)"""
    from . import opt
    masks = np.stack([load_mask_red(m) for m, _ in spec.layers])
    flows = np.stack([flo.flow_read(f) for _, f in spec.layers])
    if flows.shape[:3] != masks.shape:
        raise ValueError("seg line: mask and flow sizes differ")
    M1, M2 = (spec.m[:6], spec.m[6:]) if len(spec.m) else (None, None)
    r = opt.seg_maps(state, masks, flows, tau=spec.tau, radius=spec.radius, M1=M1, M2=M2, which=tuple(spec.out))
    for k, path in spec.out.items():
        save_occ(seg_dist_png(r[k]) if k.startswith("dist") else r[k], path)


class ScoreLine(NamedTuple):
    """a `score` line (DESIGN.md "Flow scoring"), recognised by its first word: the error table of one estimate
        score GT.flo EST.flo [occ=PNG] [dist=PNG] [skip=PNG] [mask=PNG] out=TXT
    occ: an occlusion map, non-zero = occluded; dist: the 8-bit distance file of a seg line (dist_from_png); skip: non-zero
    = left out (a fold map); mask: a frame-1 object mask in the solver's convention, red != 0 is not object and left out
    too.  `planes`: {key: path} of those given, `out` the text file (format_score).  Anything else -- an unknown or
    repeated key, an empty value, no out=, fewer than two paths -- is an error."""
    gt: str
    est: str
    planes: dict
    out: str


def _score_tokens(word, what, keys, tokens):
    """the {key: value} of a score, tscore, fscore, lscore or mscore line after its two paths, `what` files"""
    if len(tokens) < 3 or tokens[0] != word or "=" in tokens[1] or "=" in tokens[2]:
        raise ValueError("%s line: two %s files expected: %r" % (word, what, " ".join(tokens)))
    got = {}
    for t in tokens[3:]:
        k, eq, v = t.partition("=")
        if not (eq and v and k in keys) or k in got:
            raise ValueError("%s line: bad or repeated token %r" % (word, t))
        got[k] = v
    if "out" not in got:
        raise ValueError("%s line without out=: %r" % (word, " ".join(tokens)))
    return got


def parse_score(tokens):
    got = _score_tokens(SCORE_WORD, "flow", SCORE_KEYS + ("out",), tokens)
    out = got.pop("out")
    return ScoreLine(tokens[1], tokens[2], got, out)


def score_line(item):
    """the inverse of parse_score: the planes in the order of SCORE_KEYS, then out="""
    return " ".join([SCORE_WORD, item.gt, item.est] + ["%s=%s" % (k, item.planes[k]) for k in SCORE_KEYS if item.planes.get(k)] +
                    ["out=" + item.out])


def dist_from_png(u8):
    """the squared distance a seg line's 8-bit distance file stands for: d * d, 255 -> 65535.  Not seg_dist_png's inverse,
    but floor(sqrt(d2)) < r is d2 < r * r, so every pixel is in the band of the d2 the file was made from"""
    d = np.asarray(u8, np.uint8).astype(np.uint16)
    return np.where(d == 255, np.uint16(65535), d * d).astype(np.uint16)


def _load_score_planes(word, planes, like, like_path):
    """{key: the red channel of its file} of a line's planes, each of the size of the array `like` read from `like_path`"""
    plane = {}
    for k, path in planes.items():
        plane[k] = load_mask_red(path)
        if plane[k].shape != like.shape[:2]:
            raise ValueError("%s line: %s differs in size from %s" % (word, path, like_path))
    return plane


def _write_text(path, text):
    with open(path, "w") as f:
        f.write(text)


def run_score(state, spec):
    """one `score` line: read the two flows and the planes given, one opt.flow_score, write the table as text"""
    from . import opt
    gt, est = flo.flow_read(spec.gt), flo.flow_read(spec.est)
    if gt.shape != est.shape:
        raise ValueError("score line: %s and %s differ in size" % (spec.gt, spec.est))
    plane = _load_score_planes(SCORE_WORD, spec.planes, gt, spec.gt)
    skip = None
    if "skip" in plane or "mask" in plane:
        skip = np.zeros(gt.shape[:2], np.uint8)
        for k in ("skip", "mask"):
            if k in plane:
                skip |= (plane[k] != 0).astype(np.uint8)
    dist = dist_from_png(plane["dist"]) if "dist" in plane else None
    table = opt.flow_score(state, gt, est, occ=plane.get("occ"), dist=dist, skip=skip)["table"][0]
    _write_text(spec.out, format_score(table))
    return table


class TScoreLine(NamedTuple):
    """a `tscore` line (DESIGN.md "Track scoring"), recognised by its first word: the TAP-Vid table of one estimated track
    file against a generated one
        tscore GT.trk EST.trk [s=SX,SY] out=TXT
    the two files agree in W, H, F and P; s: the factors the error is taken under, finite and > 0 (float32; (1, 1) without
    it; written with %.9g); out: the text file (format_track_score).  Anything else -- an unknown or repeated key, an empty
    value, no out=, fewer than two paths -- is an error."""
    gt: str
    est: str
    scale: tuple
    out: str


def parse_tscore(tokens):
    got = _score_tokens(TSCORE_WORD, "track", ("s", "out"), tokens)
    scale = (1.0, 1.0)
    if "s" in got:
        with np.errstate(over="ignore"):
            scale = _bg_numbers(got["s"])
        if len(scale) != 2 or not all(math.isfinite(q) and q > 0 for q in scale):
            raise ValueError("tscore line: s= takes two finite factors > 0: %r" % ("s=" + got["s"]))
    return TScoreLine(tokens[1], tokens[2], scale, got["out"])


def tscore_line(item):
    """the inverse of parse_tscore: s= unless it is (1, 1), then out="""
    sx, sy = (float(np.float32(v)) for v in item.scale)
    return " ".join([TSCORE_WORD, item.gt, item.est] + (["s=%.9g,%.9g" % (sx, sy)] if (sx, sy) != (1.0, 1.0) else []) +
                    ["out=" + item.out])


def run_tscore(state, spec):
    """one `tscore` line: read the two track files, one opt.track_score, write the table as text"""
    from . import opt, trk
    gt, est = trk.read(spec.gt), trk.read(spec.est)
    if (gt["W"], gt["H"]) != (est["W"], est["H"]) or gt["pos"].shape != est["pos"].shape:
        raise ValueError("tscore line: %s and %s differ in W, H, F or P" % (spec.gt, spec.est))
    table = opt.track_score(state, gt["pos"], gt["occ"], est["pos"], est["occ"], scale=spec.scale)
    _write_text(spec.out, format_track_score(table))
    return table


class ChainLine(NamedTuple):
    """a `chain` line (DESIGN.md "Track scoring"), recognised by its first word: an estimated track file from per-link
    flow estimates
        chain PTS.trk L FLO_1 .. FLO_L [bwd=B_1,..,B_L] out=OUT.trk
    PTS.trk: the query points are its frame 0 (a points file, or a whole track file); FLO_j: the estimated flow from
    sequence frame j-1 to j; bwd: the L estimated flows back, for the forward-backward check; OUT.trk has L + 1 frames
    and PTS.trk's W, H, which every flow must have.  1 <= L < 64.  Anything else -- an unknown or repeated key, an empty
    value, a wrong count, no out= -- is an error."""
    points: str
    flows: tuple
    bwd: tuple
    out: str


def parse_chain(tokens):
    if len(tokens) < 3 or tokens[0] != CHAIN_WORD or "=" in tokens[1]:
        raise ValueError("not a chain line: %r" % " ".join(tokens))
    L = int(tokens[2]) if _UINT.match(tokens[2]) else 0
    if not 1 <= L < TSCORE_MAX_FRAMES or len(tokens) < 3 + L or any("=" in t for t in tokens[3:3 + L]):
        raise ValueError("chain line: 1..%d links, a flow file each: %r" % (TSCORE_MAX_FRAMES - 1, " ".join(tokens)))
    bwd, out = None, None
    for t in tokens[3 + L:]:
        k, eq, v = t.partition("=")
        if not (eq and v and k in ("bwd", "out")) or (k == "bwd" and bwd is not None) or (k == "out" and out is not None):
            raise ValueError("chain line: bad or repeated token %r" % t)
        if k == "out":
            out = v
        else:
            bwd = tuple(v.split(","))
            if len(bwd) != L or not all(bwd):
                raise ValueError("chain line: bwd= takes %d files: %r" % (L, t))
    if out is None:
        raise ValueError("chain line without out=: %r" % " ".join(tokens))
    return ChainLine(tokens[1], tuple(tokens[3:3 + L]), bwd or (), out)


def chain_line(item):
    """the inverse of parse_chain"""
    return " ".join([CHAIN_WORD, item.points, str(len(item.flows))] + list(item.flows) +
                    (["bwd=" + ",".join(item.bwd)] if item.bwd else []) + ["out=" + item.out])


def run_chain(state, spec):
    """one `chain` line: read the points and the flows, one opt.chain_flows, write the track file"""
    from . import opt, trk
    pts = trk.read(spec.points)
    W, H = pts["W"], pts["H"]
    flows = [flo.flow_read(p) for p in spec.flows]
    bwd = [flo.flow_read(p) for p in spec.bwd]
    for path, a in zip(spec.flows + spec.bwd, flows + bwd):
        if a.shape[:2] != (H, W):
            raise ValueError("chain line: %s differs in size from %s" % (path, spec.points))
    pos, occ = opt.chain_flows(state, np.stack(flows), pts["pos"][0], bwd=np.stack(bwd) if bwd else None)
    trk.write(spec.out, W, H, pos, occ)


class FScoreLine(NamedTuple):
    """an `fscore` line (DESIGN.md "Frame scoring"), recognised by its first word: the PSNR / SSIM table of one estimate
        fscore REF.png EST.png [occ=PNG] [dist=PNG] [skip=PNG] [obj=PNG] out=TXT
    occ: an occlusion map, non-zero = occluded; dist: the 8-bit distance file of a seg line (dist_from_png); skip: non-zero
    = left out; obj: an object mask in the solver's convention, red == 0 is object, anything else background; all in the
    pixel grid of REF.  `planes`: {key: path} of those given, `out` the text file (format_frame_score).  Anything else --
    an unknown or repeated key, an empty value, no out=, fewer than two paths -- is an error."""
    ref: str
    est: str
    planes: dict
    out: str


def parse_fscore(tokens):
    got = _score_tokens(FSCORE_WORD, "frame", FSCORE_KEYS + ("out",), tokens)
    out = got.pop("out")
    return FScoreLine(tokens[1], tokens[2], got, out)


def fscore_line(item):
    """the inverse of parse_fscore: the planes in the order of FSCORE_KEYS, then out="""
    return " ".join([FSCORE_WORD, item.ref, item.est] + ["%s=%s" % (k, item.planes[k]) for k in FSCORE_KEYS if item.planes.get(k)] +
                    ["out=" + item.out])


def run_fscore(state, spec):
    """one `fscore` line: read the two frames and the planes given, one opt.frame_score, write the table as text"""
    from . import opt
    ref, est = load_rgb(spec.ref), load_rgb(spec.est)
    if ref.shape != est.shape:
        raise ValueError("fscore line: %s and %s differ in size" % (spec.ref, spec.est))
    plane = _load_score_planes(FSCORE_WORD, spec.planes, ref, spec.ref)
    if "dist" in plane:
        plane["dist"] = dist_from_png(plane["dist"])
    table = opt.frame_score(state, ref, est, **plane)["table"][0]
    _write_text(spec.out, format_frame_score(table))
    return table


class LScoreLine(NamedTuple):
    """an `lscore` line (DESIGN.md "Map scoring"), recognised by its first word: the DAVIS J / F table of one estimated
    label map
        lscore GT.png EST.png l=<L> r=<radius> [skip=PNG] out=TXT
    GT, EST: label maps in the format of Index1 / Index2 (the red channel; 0 = no object); l=: the labels scored, 1..255;
    r=: the tolerance of the boundary match, 0 .. SEG_MAX_RADIUS; skip: non-zero = left out.  `skip` is None when not
    given, `out` the text file (format_label_score).  Anything else -- an unknown or repeated key, an empty value, no
    out=, no l= or r=, a number out of range, fewer than two paths -- is an error."""
    gt: str
    est: str
    L: int
    radius: int
    skip: Optional[str]
    out: str


class MScoreLine(NamedTuple):
    """an `mscore` line (DESIGN.md "Map scoring"), recognised by its first word: the precision / recall table of one
    estimated occlusion or motion-boundary map
        mscore GT.png EST.png [t=<thr,...> r=<radius>] [skip=PNG] out=TXT
    GT: non-zero = positive; EST: a score 0..255 (the red channel of both); t=: 1 to MSCORE_MAX_THR thresholds 1..255 for
    the tolerant boundary match, with r= its radius, 0 .. SEG_MAX_RADIUS -- both or neither; skip: non-zero = left out.
    `thr` is () and `radius` None without t=; `out` the text file (format_map_score).  Anything else is an error."""
    gt: str
    est: str
    thr: tuple
    radius: Optional[int]
    skip: Optional[str]
    out: str


def _score_uint(word, text, low, high):
    if text is None or not _UINT.match(text) or not low <= int(text) <= high:
        raise ValueError("%s line: a number %d..%d expected, not %r" % (word, low, high, text))
    return int(text)


def parse_lscore(tokens):
    got = _score_tokens(LSCORE_WORD, "map", ("l", "r", "skip", "out"), tokens)
    return LScoreLine(tokens[1], tokens[2], _score_uint(LSCORE_WORD, got.get("l"), 1, 255),
                      _score_uint(LSCORE_WORD, got.get("r"), 0, SEG_MAX_RADIUS), got.get("skip"), got["out"])


def lscore_line(item):
    """the inverse of parse_lscore: l=, r=, skip= if given, out="""
    return " ".join([LSCORE_WORD, item.gt, item.est, "l=%d" % item.L, "r=%d" % item.radius] +
                    (["skip=" + item.skip] if item.skip else []) + ["out=" + item.out])


def parse_mscore(tokens):
    got = _score_tokens(MSCORE_WORD, "map", ("t", "r", "skip", "out"), tokens)
    if ("t" in got) != ("r" in got):
        raise ValueError("mscore line: t= and r= come together: %r" % " ".join(tokens))
    thr, radius = (), None
    if "t" in got:
        thr = tuple(_score_uint(MSCORE_WORD, v, 1, 255) for v in got["t"].split(","))
        radius = _score_uint(MSCORE_WORD, got["r"], 0, SEG_MAX_RADIUS)
        if len(thr) > MSCORE_MAX_THR:
            raise ValueError("mscore line: at most %d thresholds: %r" % (MSCORE_MAX_THR, got["t"]))
    return MScoreLine(tokens[1], tokens[2], thr, radius, got.get("skip"), got["out"])


def mscore_line(item):
    """the inverse of parse_mscore: t= and r= if it has thresholds, skip= if given, out="""
    return " ".join([MSCORE_WORD, item.gt, item.est] +
                    (["t=" + ",".join("%d" % t for t in item.thr), "r=%d" % item.radius] if item.thr else []) +
                    (["skip=" + item.skip] if item.skip else []) + ["out=" + item.out])


def _load_score_maps(word, spec):
    gt = load_mask_red(spec.gt)
    plane = _load_score_planes(word, dict([("est", spec.est)] + ([("skip", spec.skip)] if spec.skip else [])), gt, spec.gt)
    return gt, plane["est"], plane.get("skip")


def run_lscore(state, spec):
    """one `lscore` line: read the maps, one opt.label_score, write the table as text"""
    from . import opt
    gt, est, skip = _load_score_maps(LSCORE_WORD, spec)
    table = opt.label_score(state, gt, est, spec.L, spec.radius, skip=skip)["table"][0]
    _write_text(spec.out, format_label_score(table))
    return table


def run_mscore(state, spec):
    """one `mscore` line: read the maps, one opt.map_score, write the score as text"""
    from . import opt
    gt, est, skip = _load_score_maps(MSCORE_WORD, spec)
    r = opt.map_score(state, gt, est, skip=skip, thr=spec.thr, radius=spec.radius or 0)
    score = dict(hist=r["hist"][0], thr=tuple(spec.thr), match=r["match"][0])
    _write_text(spec.out, format_map_score(score))
    return score


class InterpLine(NamedTuple):
    """an `interp` line (DESIGN.md "Frames from flows"), recognised by its first word: the in-between frames of a pair
    from a flow estimate
        interp A.png B.png FWD.flo s=I1,I2,.. n=N [bwd=BWD.flo] [src=1] out=PREFIX
    A, B: frame 1 and frame 2; FWD: the estimated flow A -> B; bwd: the estimated flow B -> A; the times are (float)I /
    (float)N, the ramp's own alpha_i: 1 to INTERP_MAX_TIMES steps, distinct and ascending, 1 <= I < N; written:
    PREFIX_sII.png (mid_files' naming) and, with src=1, PREFIX_sII_src.png, the source map.  Anything else -- an unknown
    or repeated key, an empty value, no s=, n= or out=, fewer than three paths -- is an error."""
    a: str
    b: str
    fwd: str
    steps: tuple
    n: int
    bwd: str
    src: bool
    out: str


def parse_interp(tokens):
    if len(tokens) < 4 or tokens[0] != INTERP_WORD or any("=" in t for t in tokens[1:4]):
        raise ValueError("interp line: two frame files and a flow file expected: %r" % " ".join(tokens))
    got = {}
    for t in tokens[4:]:
        k, eq, v = t.partition("=")
        if not (eq and v and k in ("s", "n", "bwd", "src", "out")) or k in got:
            raise ValueError("interp line: bad or repeated token %r" % t)
        got[k] = v
    if "s" not in got or "n" not in got or "out" not in got:
        raise ValueError("interp line without s=, n= or out=: %r" % " ".join(tokens))
    n = int(got["n"]) if _UINT.match(got["n"]) and int(got["n"]) < 1 << 32 else 0
    steps = tuple(int(v) if _UINT.match(v) else 0 for v in got["s"].split(","))
    if not (1 <= len(steps) <= INTERP_MAX_TIMES and steps[0] >= 1 and steps[-1] < n and all(a < b for a, b in zip(steps, steps[1:]))):
        raise ValueError("interp line: s=I1,I2,.. n=N with 1 <= I1 < I2 < .. < N, at most %d steps: %r" % (INTERP_MAX_TIMES, " ".join(tokens)))
    if got.get("src", "1") != "1":
        raise ValueError("interp line: src=1 or no src=: %r" % " ".join(tokens))
    return InterpLine(tokens[1], tokens[2], tokens[3], steps, n, got.get("bwd", ""), "src" in got, got["out"])


def interp_line(item):
    """the inverse of parse_interp: s=, n=, bwd=, src=, out= in that order"""
    return " ".join([INTERP_WORD, item.a, item.b, item.fwd, "s=" + ",".join("%d" % i for i in item.steps), "n=%d" % item.n] +
                    (["bwd=" + item.bwd] if item.bwd else []) + (["src=1"] if item.src else []) + ["out=" + item.out])


def interp_files(prefix, step):
    """the files of an `interp` line for ramp step `step`: the frame (mid_files' name) and its source map"""
    return dict(rgb=mid_files(prefix, step)["rgb"], src="%s_s%02d_src.png" % (prefix, step))


def interp_times(steps, n):
    """the times of an interp line, float32: (float)I / (float)N"""
    return np.array([np.float32(i) / np.float32(n) for i in steps], np.float32)


def run_interp(state, spec):
    """one `interp` line: read the two frames and the flows, one opt.interp_frames, write a frame (and a source map) per step"""
    from . import opt
    a, b = load_rgb(spec.a), load_rgb(spec.b)
    if a.shape != b.shape:
        raise ValueError("interp line: %s and %s differ in size" % (spec.a, spec.b))
    fwd = flo.flow_read(spec.fwd)
    bwd = flo.flow_read(spec.bwd) if spec.bwd else None
    for path, f in ((spec.fwd, fwd), (spec.bwd, bwd)):
        if f is not None and f.shape[:2] != a.shape[:2]:
            raise ValueError("interp line: %s differs in size from %s" % (path, spec.a))
    out, src = opt.interp_frames(state, a, b, fwd, interp_times(spec.steps, spec.n), bwd=bwd, want_src=True)
    for k, i in enumerate(spec.steps):
        names = interp_files(spec.out, i)
        Image.fromarray(out[k]).save(names["rgb"])
        if spec.src:
            Image.fromarray(src[k], "L").save(names["src"])
    return out, src


def parse_line(line):
    """a list line, as text or as its tokens -> SolveLine, or parse_layers' dict when its first word is `layers`, a
    BgLine when it is `bg`, a TexLine when it is `tex`, a TrkLine when it is `trk`, a BlurLine when it is `blur`, a
    LightLine when it is `light`, a SegLine when it is `seg`, a ScoreLine when it is `score`, a TScoreLine when it is
    `tscore`, a ChainLine when it is `chain`, an FScoreLine when it is `fscore`, an InterpLine when it is `interp`, an
    LScoreLine when it is `lscore`, an MScoreLine when it is `mscore`"""
    tok = line.split() if isinstance(line, str) else list(line)
    if tok and tok[0] == LSCORE_WORD:
        return parse_lscore(tok)
    if tok and tok[0] == MSCORE_WORD:
        return parse_mscore(tok)
    if tok and tok[0] == INTERP_WORD:
        return parse_interp(tok)
    if tok and tok[0] == FSCORE_WORD:
        return parse_fscore(tok)
    if tok and tok[0] == TSCORE_WORD:
        return parse_tscore(tok)
    if tok and tok[0] == CHAIN_WORD:
        return parse_chain(tok)
    if tok and tok[0] == SCORE_WORD:
        return parse_score(tok)
    if tok and tok[0] == SEG_WORD:
        return parse_seg(tok)
    if tok and tok[0] == LIGHT_WORD:
        return parse_light(tok)
    if tok and tok[0] == BLUR_WORD:
        return parse_blur(tok)
    if tok and tok[0] == TRK_WORD:
        return parse_trk(tok)
    if tok and tok[0] == TEX_WORD:
        return parse_tex(tok)
    if tok and tok[0] == LAYERS_WORD:
        return parse_layers(tok)
    if tok and tok[0] == BG_WORD:
        return parse_bg(tok)
    if len(tok) < 6:
        raise ValueError("list line needs 6 paths: %r" % line)
    return SolveLine(*tok[:6], extra=parse_extra(tok[6:]))


def format_line(item):
    """the inverse of parse_line: the text of a list line, optional tokens in the order of extra_tokens / layers_line"""
    if isinstance(item, SolveLine):
        return " ".join(list(item[:6]) + extra_tokens(item.extra))
    if isinstance(item, BgLine):
        return bg_line(item)
    if isinstance(item, TexLine):
        return tex_line(item)
    if isinstance(item, TrkLine):
        return trk_line(item)
    if isinstance(item, BlurLine):
        return blur_line(item)
    if isinstance(item, LightLine):
        return light_line(item)
    if isinstance(item, SegLine):
        return seg_line(item)
    if isinstance(item, ScoreLine):
        return score_line(item)
    if isinstance(item, TScoreLine):
        return tscore_line(item)
    if isinstance(item, ChainLine):
        return chain_line(item)
    if isinstance(item, FScoreLine):
        return fscore_line(item)
    if isinstance(item, LScoreLine):
        return lscore_line(item)
    if isinstance(item, MScoreLine):
        return mscore_line(item)
    if isinstance(item, InterpLine):
        return interp_line(item)
    return layers_line(item["rgb"], item["layers"], item["out"])


def done_token(item):
    """the path `arap_deform --serve` reports a line done by: a solve's flow, a layers line's first output token, the
    first of a bg line's bg_outputs, a tex, blur, light or seg line's first output token, a trk line's track file, a score,
    tscore, chain, fscore, lscore or mscore line's out= file, an interp line's out= prefix"""
    if isinstance(item, (TrkLine, ScoreLine, TScoreLine, ChainLine, FScoreLine, InterpLine, LScoreLine, MScoreLine)):
        return item.out
    if isinstance(item, (BlurLine, LightLine, SegLine)):
        return next(iter(item.out.values()))
    if isinstance(item, BgLine):
        return bg_outputs(item)[0]
    if isinstance(item, TexLine):
        return next(iter(item.out.values()))
    return item.flow if isinstance(item, SolveLine) else next(iter(item["out"].values()))


def read_list_items(path):
    """every non-blank line of a list file in order, parsed (parse_line)"""
    with open(path) as f:
        return [parse_line(line) for line in f if line.strip()]


def run_layers(state, spec):
    """one `layers` line: read the frame's RGB and every layer's mask / flow, one opt.warp_layers, write what the line
    asks for (occ / occ_bwd: 8-bit L PNG; bwd: .flo; rgb2: RGB PNG; mask2: 1-bit PNG as a solve's warped mask; mid:
    run_layers_mid)"""
    from . import opt
    rgb = load_rgb(spec["rgb"])
    masks = [load_mask_red(m) for m, _ in spec["layers"]]
    flows = [flo.flow_read(f) for _, f in spec["layers"]]
    for m, f in zip(masks, flows):
        if m.shape != rgb.shape[:2] or f.shape[:2] != rgb.shape[:2]:
            raise ValueError("layers line: image, mask and flow sizes differ")
    out = spec["out"]
    if "mid" in out:
        run_layers_mid(state, spec, rgb, np.stack(masks), np.stack(flows))
    if not set(out) - {"mid"}:
        return
    r = opt.warp_layers(state, rgb, np.stack(masks), np.stack(flows), bwd="bwd" in out, occ_bwd="occ_bwd" in out,
                        occ="occ" in out)
    if "rgb2" in out:
        Image.fromarray(r["warped_rgb"]).save(out["rgb2"])
    if "mask2" in out:
        save_mask(r["warped_mask"], out["mask2"])
    if "bwd" in out:
        flo.flow_write(out["bwd"], r["backward_flow"])
    if "occ_bwd" in out:
        save_occ(r["occlusion_bwd"], out["occ_bwd"])
    if "occ" in out:
        save_occ(r["occlusion"], out["occ"])


def run_background(state, spec):
    """one `bg` line: read the background picture, the pair's frames, masks, flow and the object-side maps the line
    names, one opt.background, write what the line asks for (RGB: RGB PNG; flows: .flo; occlusions: 8-bit L PNG); then,
    with mid=, the sequence pass run_background_seq"""
    from . import opt
    bg, rgb1, rgb2 = load_rgb(spec.bg), load_rgb(spec.rgb1), load_rgb(spec.rgb2)
    mask_red = load_mask_red(spec.mask1)
    cover2 = np.where(load_mask_red(spec.mask2) != 0, 255, 0).astype(np.uint8)
    fl = flo.flow_read(spec.flow)
    inp = dict(occ=None, bwd=None, occ_bwd=None)
    if "occ" in spec.inputs:
        inp["occ"] = np.array(Image.open(spec.inputs["occ"]).convert("L"))
    if "bwd" in spec.inputs:
        inp["bwd"] = flo.flow_read(spec.inputs["bwd"])
    if "occ_bwd" in spec.inputs:
        inp["occ_bwd"] = np.array(Image.open(spec.inputs["occ_bwd"]).convert("L"))
    H, W = mask_red.shape
    for a in (rgb1, rgb2, cover2, fl) + tuple(v for v in inp.values() if v is not None):
        if a.shape[:2] != (H, W):
            raise ValueError("bg line: image, mask and flow sizes differ")
    names = dict(zip(("out_rgb1", "out_rgb2", "flow_full"), spec.out))
    names.update(occ_full=spec.outs.get("occ_out"), bwd_full=spec.outs.get("bwd_out"),
                 occ_bwd_full=spec.outs.get("occ_bwd_out"))
    want = [k for k in opt.BG_OUTPUTS if names.get(k)]
    if want:
        r = opt.background(state, bg, spec.m[:6], spec.m[6:], rgb1, mask_red, rgb2, cover2, fl, want=want, **inp)
    for k in want:
        if k.startswith("out_rgb"):
            Image.fromarray(r[k]).save(names[k])
        elif k in ("flow_full", "bwd_full"):
            flo.flow_write(names[k], r[k])
        else:
            save_occ(r[k], names[k])
    if spec.mid:
        run_background_seq(state, spec, bg, mask_red, cover2)


def run_background_seq(state, spec, bg, mask_red, cover2):
    """the mid= / mm= / mid_out= tokens of a `bg` line (DESIGN.md "Moving background over in-between frames"): the
    frames are frame 1, the snapshots of mid= and frame 2; one opt.background_seq over them writes the files of
    mid_bg_files -- every in-between frame, every link's flow and, with occ= on the line, every link's occlusion.  The
    composites of frame 1 and frame 2 stay with out=."""
    from . import opt
    steps, prefix = parse_mid(spec.mid)
    H, W = mask_red.shape

    def read(path, load):
        if not osp.exists(path):
            raise ValueError("bg line: snapshot %s is missing" % path)
        a = load(path)
        if a.shape[:2] != (H, W):
            raise ValueError("bg line: %s differs in size from %s" % (path, spec.mask1))
        return a
    files = [mid_files(prefix, i) for i in steps]
    covers = [None] + [np.where(read(f["mask"], load_mask_red) != 0, 255, 0).astype(np.uint8) for f in files] + [cover2]
    rgbs = [None] + [read(f["rgb"], load_rgb) for f in files] + [None]
    flows = [read(files[0]["flow"], flo.flow_read)] + [read(f["step"], flo.flow_read) for f in files]
    occs = None
    if "occ" in spec.inputs:
        gray = lambda q: np.array(Image.open(q).convert("L"))
        occs = [read(mid_layer_files(prefix, i)["occ"], gray) for i in (0,) + steps]
    maps = np.asarray(spec.m[:6] + spec.mm + spec.m[6:], np.float32).reshape(-1, 6)
    r = opt.background_seq(state, bg, maps, mask_red, covers, rgbs, flows, occs)
    for k, i in enumerate((0,) + steps):
        out = mid_bg_files(spec.mid_out, i)
        if k:
            Image.fromarray(r["out_rgb"][k]).save(out["rgb"])
        flo.flow_write(out["step"], r["flow_full"][k])
        if occs is not None:
            save_occ(r["occ_full"][k], out["occ"])


def owner_flow(masks, flows):
    """the composite frame-1 flow of n layers, masks (n, H, W) red channels and flows (n, H, W, 2): per frame-1 pixel v
    the flow of owner(v), the largest l with masks[l][v] == 0, and (0, 0) where no layer owns v.  The owner rule of
    the layered warp -- not the warped-mask selection merge_segments keeps for a frame's final .flo."""
    obj = np.asarray(masks) == 0
    n = obj.shape[0]
    top = (n - 1) - np.argmax(obj[::-1], axis=0)
    flow = np.take_along_axis(np.asarray(flows, np.float32), top[None, ..., None], axis=0)[0]
    flow[~obj.any(0)] = 0
    return flow


def run_layers_mid(state, spec, rgb, masks, flows):
    """the mid= token of a `layers` line (DESIGN.md "Layered in-between frames").  Layer l's state after ramp step i is
    the file mid_files(stem_l, i)["flow"], stem_l = FLO_l without its `.flo`; after the last snapshot comes the layers'
    final flow.  Per snapshot one opt.warp_layers_step, written as mid_files(PREFIX, i): the owner_flow of the snapshot,
    the composite in-between frame and mask, the step flow; with occ= on the line also the link occlusions of
    mid_layer_files, steps 0 (frame 1 -> first snapshot, opt.warp_layers' occlusion) and i."""
    from . import opt
    out = spec["out"]
    steps, prefix = parse_mid(out["mid"])
    states = []
    for i in steps:
        per = []
        for _, f in spec["layers"]:
            if not f.endswith(".flo"):
                raise ValueError("layers line: mid= needs flows named *.flo, got %s" % f)
            snap = mid_files(f[:-4], i)["flow"]
            if not osp.exists(snap):
                raise ValueError("layers line: snapshot %s is missing" % snap)
            per.append(flo.flow_read(snap))
            if per[-1].shape != flows[0].shape:
                raise ValueError("layers line: %s differs in size from %s" % (snap, spec["rgb"]))
        states.append(np.stack(per))
    states.append(flows)
    occ = "occ" in out
    if occ:
        save_occ(opt.warp_layers(state, None, masks, states[0])["occlusion"], mid_layer_files(prefix, 0)["occ"])
    for k, i in enumerate(steps):
        r = opt.warp_layers_step(state, rgb, masks, states[k], states[k + 1], step=True, occ=occ)
        f = mid_files(prefix, i)
        flo.flow_write(f["flow"], owner_flow(masks, states[k]))
        Image.fromarray(r["warped_rgb"]).save(f["rgb"])
        save_mask(r["warped_mask"], f["mask"])
        flo.flow_write(f["step"], r["step"])
        if occ:
            save_occ(r["occlusion_step"], mid_layer_files(prefix, i)["occ"])


def save_occ(occ, path):
    """an occlusion map as an 8-bit L PNG, 0 / 255"""
    Image.fromarray(np.ascontiguousarray(occ, np.uint8), "L").save(path)


def load_rgb(path):
    return np.array(Image.open(path).convert("RGB"))


# the lines of a diag file: ArapFlow_MeshStats in the struct's order, without `reserved` (DESIGN.md "Fold diagnostics")
DIAG_COUNTS = ("vertices", "outside", "triangles", "folded", "nonfinite")
DIAG_FLOATS = ("det_min", "det_max", "disp2_max")


def format_diag(stats):
    """the text of a diag file: eight lines `name value`, counts in decimal, floats as printf's %.9g of the float32
    (inf, -inf as printf writes them); the C++ worker writes the same bytes"""
    return "".join(["%s %d\n" % (k, int(stats[k])) for k in DIAG_COUNTS] +
                   ["%s %.9g\n" % (k, float(np.float32(stats[k]))) for k in DIAG_FLOATS])


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


def load_mask_red(path):
    """red channel of the mask PNG (CombinedSolver.h:213,234): 0 = deformable object"""
    return np.array(Image.open(path).convert("RGB"))[..., 0]


def save_mask(mask, path):
    """LodePNG writes the 0/255 warped mask as a 1-bit image: np.array(Image.open()) of
    it is bool, which para_gen.py's flatten relies on only through != 0 / == 0."""
    Image.fromarray(np.ascontiguousarray(mask) > 0).save(path)


FILL_MIN, FILL_MAX = 8, 32     # frames per solve call: at least / at most (see deform_list)


def _load_line(ln):
    """loadData (main.cpp:116-138) of one solve line: RGB, red channel of the mask, constraint rows"""
    from . import opt
    return load_rgb(ln.rgb), load_mask_red(ln.mask), opt.load_constraints(ln.constraints)


def _save_result(ln, r):
    Image.fromarray(r["warped_rgb"]).save(ln.out_rgb)
    save_mask(r["warped_mask"], ln.out_mask)
    flo.flow_write(ln.flow, r["flow"])
    extra = ln.extra
    if "bwd" in extra:
        flo.flow_write(extra["bwd"], r["backward_flow"])
    if "occ_bwd" in extra:
        save_occ(r["occlusion_bwd"], extra["occ_bwd"])
    if "occ" in extra:
        save_occ(r["occlusion"], extra["occ"])
    if "diag" in extra:
        with open(extra["diag"], "w") as f:
            f.write(format_diag(r["mesh_stats"]))
    if "fold" in extra:
        save_occ(r["fold"], extra["fold"])
    if "mid" in extra:
        steps, prefix = parse_mid(extra["mid"])
        for i, m in zip(steps, r["mid"]):
            f = mid_files(prefix, i)
            flo.flow_write(f["flow"], m["flow"])
            Image.fromarray(m["rgb"]).save(f["rgb"])
            save_mask(m["mask"], f["mask"])
            flo.flow_write(f["step"], m["step"])


def batch_snapshots(batch):
    """the snapshot steps of a batch of SolveLines: those of its mid= lines, which must all name the same; () if none
    asks"""
    steps = ()
    for ln in batch:
        if "mid" in ln.extra:
            own = parse_mid(ln.extra["mid"])[0]
            if steps and own != steps:
                raise ValueError("mid= steps %s differ from the batch's %s: %s" % (own, steps, ln.flow))
            steps = own
    return steps


class _Lane:
    """one of deform_list's two alternating solvers and the lines of the batch it holds: `batch` is filled as frames are
    accepted into the solver's slots and emptied when their results are handed on (drain), nowhere else"""

    def __init__(self):
        self.solver, self.batch = None, []
        self.snaps = ()                # the snapshot steps in effect in `solver` (batch_snapshots)
        self.diag = False              # fold diagnostics in effect in `solver`


def deform_list(state, lines, num_iter=19, non_linear_iter=8, linear_iter=400, max_batch=FILL_MAX, verbose=True):
    """arap_deform over a list of SolveLines (main.cpp:223-238).  Frames of equal size are solved together: the library
    gives every solve a group of the resident launch's workgroups sized by its active tiles, and a launch costs the
    same however full it is, so frames are added to a batch while they still fit ONE launch (8 DAVIS-shaped 854x480
    frames, ~24 --multseg segment solves); FILL_MIN frames per call when the resident path does not apply.
    The GPU does not wait for the host (the structure of arap_flow_amd/host/arap_deform.cpp): two solver objects
    alternate; while one batch is solved the next is decoded (worker threads) and uploaded into the other object, and
    the previous batch's results are read from pinned memory and encoded (worker threads)."""
    from concurrent.futures import ThreadPoolExecutor
    from . import opt
    state.use_own_stream()
    ahead = 2 * max_batch
    with ThreadPoolExecutor(max_workers=8) as pool:
        loading = {}

        def frame_at(k):
            for q in range(k, min(len(lines), k + ahead + 1)):
                if q not in loading:
                    loading[q] = pool.submit(_load_line, lines[q])
            return loading[k].result()

        writing = []
        lanes = [_Lane(), _Lane()]
        size = None

        def drain(lane):
            """wait for the lane's solve, hand copies of its results to the writer threads"""
            if not lane.batch:
                return
            lane.solver.wait()
            for b, ln in enumerate(lane.batch):
                r = lane.solver.host_results(b)
                res = {k: v.copy() for k, v in r.items() if v is not None}
                if "mid" in ln.extra:
                    res["mid"] = [{k: v.copy() for k, v in lane.solver.host_snapshot(b, q).items()}
                                  for q in range(len(parse_mid(ln.extra["mid"])[0]))]
                writing.append(pool.submit(_save_result, ln, res))
                if verbose:
                    print("Saved")                                          # main.cpp:159
            lane.batch = []
            while len(writing) > 48:
                writing.pop(0).result()

        i, cur = 0, 0
        while i < len(lines):
            rgb0 = frame_at(i)[0]
            H, W = rgb0.shape[:2]
            if size != (W, H):
                for lane in lanes:
                    drain(lane)
                    if lane.solver is not None:
                        lane.solver.close()
                if size is not None and verbose:
                    print("Warning: Input image has different size to one in the prebuilt plan.\n"
                          "To avoid re-building the plan and to save time, put images of the same size in the "
                          "same list.\nStarting to re-build plan...")      # CombinedSolver.h:151-153
                for lane in lanes:
                    lane.solver = opt.FrameSolver(state, W, H, batch=max_batch)
                    lane.snaps, lane.diag = (), False
                size = (W, H)
            lane, other = lanes[cur], lanes[cur ^ 1]
            solver, batch = lane.solver, lane.batch                     # (empty: drained a round ago)
            j = i
            while j < len(lines) and len(batch) < max_batch:
                ln = lines[j]
                rgb, mask, cons = frame_at(j)
                if rgb.shape[:2] != (H, W):
                    break
                if mask.shape != (H, W):
                    raise ValueError("mask %s has another size than %s" % (ln.mask, ln.rgb))
                b = len(batch)
                solver.set_frame(b, mask, cons, rgb=rgb, border_pins=True)
                if b > 0:
                    launches = solver.launches_for(b + 1)
                    if launches > 1 or (launches == 0 and b >= FILL_MIN):
                        break                                   # this frame opens the next batch (its slot is re-set)
                batch.append(ln)
                del loading[j]                                  # the device holds it now
                j += 1
            want = set().union(*[ln.extra for ln in batch])
            solver.set_outputs(backward=bool(want & {"bwd", "occ_bwd"}), occlusion="occ" in want)
            steps = batch_snapshots(batch)                      # on iff a line asks: plain batches run nothing new
            if steps != lane.snaps:
                solver.set_snapshots(steps)
                lane.snaps = steps
            diag = bool(want & {"diag", "fold"})                # likewise: set only to turn it on, or off again
            if diag != lane.diag:
                solver.set_diag(diag)
                lane.diag = diag
            solver.solve_async(len(batch), num_iter, non_linear_iter, linear_iter, warp=True, download=True)
            drain(other)                                               # the previous batch, while this one is being solved
            cur ^= 1
            i = j
        for lane in (lanes[cur], lanes[cur ^ 1]):
            drain(lane)
        for f in writing:
            f.result()
        for lane in lanes:
            if lane.solver is not None:
                lane.solver.close()


def warp_files(state, rgb_path, mask_path, flo_path, out_rgb_path, out_mask_path, extra=None):
    """warp_image (ARAP/warping/src/main.cpp:302-336); `extra` ({key: path}, parse_extra): the optional outputs"""
    from . import opt
    rgb, mask, fl = load_rgb(rgb_path), load_mask_red(mask_path), flo.flow_read(flo_path)
    if fl.shape[:2] != mask.shape or rgb.shape[:2] != mask.shape:
        raise ValueError("image, mask and flow sizes differ")
    if extra and {"diag", "fold"} & set(extra):
        d = opt.warp_diag(state, mask, fl, fold="fold" in extra)
        if "diag" in extra:
            with open(extra["diag"], "w") as f:
                f.write(format_diag(d["stats"]))
        if "fold" in extra:
            save_occ(d["fold"], extra["fold"])
    if extra and set(extra) - {"diag", "fold"}:
        r = opt.warp_image_ex(state, rgb, mask, fl, backward=bool({"bwd", "occ_bwd"} & set(extra)),
                              occlusion="occ" in extra)
        Image.fromarray(r["warped_rgb"]).save(out_rgb_path)
        save_mask(r["warped_mask"], out_mask_path)
        if "bwd" in extra:
            flo.flow_write(extra["bwd"], r["backward_flow"])
        if "occ_bwd" in extra:
            save_occ(r["occlusion_bwd"], extra["occ_bwd"])
        if "occ" in extra:
            save_occ(r["occlusion"], extra["occ"])
        return
    wrgb, wmsk = opt.warp_image(state, rgb, mask, fl)
    Image.fromarray(wrgb).save(out_rgb_path)
    save_mask(wmsk, out_mask_path)


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
