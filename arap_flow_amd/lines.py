"""The list line: the unit of work between para_gen.py, arap_deform.py and `arap_deform --serve`, as text and as a typed item.

Pure text: the standard library and numpy, nothing of the GPU, of image files or of libarapopt.so.  A line is a solve (six
paths and optional output tokens) or, by its first word, one of the other forms.  FORMS at the end of this file is the table
of them all -- a form's word, its type, its parser, its writer and the path a worker reports it done by -- and parse_line,
format_line and done_token are lookups in it; a new form is one more entry.  run_lines.py has the executor of every type.
The C++ twin, host/list_line.h, is an independent reading of the same grammar; the line_tool tests hold the two side by side.
"""
import math
import re
from operator import attrgetter
from typing import Callable, NamedTuple, Optional

import numpy as np

from .scores import TSCORE_MAX_FRAMES, MSCORE_MAX_THR

# the limits of include/arap_opt.h that the grammar checks
MAX_SNAPSHOTS = 8            # ARAPFLOW_MAX_SNAPSHOTS
MAX_BLUR_SAMPLES = 32        # ARAPFLOW_MAX_BLUR_SAMPLES
SEG_MAX_RADIUS = 254         # ARAPFLOW_SEG_MAX_RADIUS
INTERP_MAX_TIMES = 32        # ARAPFLOW_INTERP_MAX_TIMES
LIGHT_MAX_R, LIGHT_MAX_SHIFT = 16, 64      # ARAPFLOW_LIGHT_MAX_R, ARAPFLOW_LIGHT_MAX_SHIFT
TEX_KINDS = ("checker", "brick", "voronoi", "noise", "wave")         # ARAPFLOW_TEX_*: a kind's number is its index

# every form's first word (a solve line has none) and its optional keys, in the order its writer puts them
LAYERS_WORD, BG_WORD, TEX_WORD, TRK_WORD, BLUR_WORD, LIGHT_WORD, SEG_WORD = "layers", "bg", "tex", "trk", "blur", "light", "seg"
SCORE_WORD, TSCORE_WORD, CHAIN_WORD, FSCORE_WORD, INTERP_WORD = "score", "tscore", "chain", "fscore", "interp"
LSCORE_WORD, MSCORE_WORD = "lscore", "mscore"
EXTRA_KEYS = ("bwd", "occ", "occ_bwd", "mid", "diag", "fold")
LAYER_KEYS = ("occ", "bwd", "occ_bwd", "rgb2", "mask2", "mid")
BG_IN_KEYS = ("occ", "bwd", "occ_bwd")                               # optional object-side inputs of a bg line
BG_OUT_KEYS = ("occ_out", "bwd_out", "occ_bwd_out")                  # the full maps made from them
TEX_KEYS = ("rgb1", "rgb2", "mask2")
BLUR_KEYS = ("rgb1", "rgb2", "alpha1", "alpha2")
LIGHT_KEYS = ("rgb1", "rgb2")
SEG_KEYS = ("idx1", "idx2", "mb1", "mb2", "dist1", "dist2")
SCORE_KEYS = ("occ", "dist", "skip", "mask")
FSCORE_KEYS = ("occ", "dist", "skip", "obj")


# ------------------------------------------------------------------------------------------------------
# the readers and writers the forms share
# ------------------------------------------------------------------------------------------------------
_UINT = re.compile(r"[0-9]{1,10}$")
_INT = re.compile(r"-?[0-9]{1,10}$")


def _text(tokens):
    return " ".join(tokens)


def _uint(text):
    """an unsigned decimal number, or -1 for anything else"""
    return int(text) if _UINT.match(text) else -1


def _floats(text):
    """comma separated numbers as float32 values; () when one of them is no number (a number beyond float32 becomes inf)"""
    try:
        with np.errstate(over="ignore"):
            return tuple(float(np.float32(float(q))) for q in text.split(","))
    except ValueError:
        return ()


def _finite(values):
    return all(math.isfinite(v) for v in values)


def _f32(v):
    """a float32 as a line writes it"""
    return "%.9g" % float(np.float32(v))


def _outputs(keys, out):
    """the tokens of the outputs {key: path}, in the order of `keys`"""
    return ["%s=%s" % (k, out[k]) for k in keys if out.get(k)]


def _layer_head(word, tokens, at, first=None, width=2, fixed=0, count=_uint, paths=True):
    """the head `n MASK_1 FLO_1 ... MASK_n FLO_n` of a layers, tex, blur, seg or trk line: the count at tokens[at], 1..255,
    then from tokens[first] (at + 1 unless given) `width` paths per layer and `fixed` more after the last -> (the layers as
    tuples of `width` paths, the index of the first token after them).  With `paths`, no token before that index holds a `=`."""
    if len(tokens) <= at or tokens[0] != word:
        raise ValueError("not a %s line: %r" % (word, _text(tokens)))
    n, first = count(tokens[at]), at + 1 if first is None else first
    end = first + width * n + fixed
    if not 1 <= n <= 255 or len(tokens) < end:
        raise ValueError("%s line: 1..255 layers, %d paths each and %d after them: %r" % (word, width, fixed, _text(tokens)))
    if paths and any("=" in t for t in tokens[1:end]):
        raise ValueError("%s line: a path expected where a token is: %r" % (word, _text(tokens)))
    return [tuple(tokens[first + width * l:first + width * (l + 1)]) for l in range(n)], end


def _head_tokens(layers):
    """the inverse of _layer_head for layers of two paths: the count, then every layer's mask and flow"""
    return [str(len(layers))] + [p for pair in layers for p in pair]


def _key_values(word, tokens, keys):
    """the (key, value) of every KEY=VALUE token in turn; an unknown key, a missing `=` and an empty value are errors"""
    for t in tokens:
        k, eq, v = t.partition("=")
        if not (eq and v and k in keys):
            raise ValueError("%s line: bad token %r" % (word, t))
        yield k, v


def _keyed(word, tokens, keys, need=()):
    """the strict tail of a line: {key: value} in line order of its KEY=VALUE tokens (_key_values); a repeated key is an
    error too, and so is a line without one of the keys of `need`"""
    got = {}
    for k, v in _key_values(word, tokens, keys):
        if k in got:
            raise ValueError("%s line: repeated token %s=%s" % (word, k, v))
        got[k] = v
    for k in need:
        if k not in got:
            raise ValueError("%s line without %s=: %r" % (word, k, _text(tokens)))
    return got


def _outs_of(word, got, keys):
    """the outputs {key: path} among a line's tokens `got`, in line order; at least one"""
    out = {k: v for k, v in got.items() if k in keys}
    if not out:
        raise ValueError("%s line without an output" % word)
    return out


def _camera(word, value, finite=True):
    """the value of a camera token m=: twelve float32, M1 then M2, finite unless told otherwise"""
    m = _floats(value)
    if len(m) != 12 or (finite and not _finite(m)):
        raise ValueError("%s line: m= takes 12 %snumbers, M1 then M2: %r" % (word, "finite " if finite else "", value))
    return m


def _camera_tokens(m):
    """the m= token of a blur or seg line's camera, none for a line without one"""
    return ["m=" + ",".join(_f32(v) for v in m)] if len(m) else []


def _float_uint(word, key, value, low, high):
    """the value of b= or s=: a finite float32 >= 0 and an unsigned integer low..high, comma separated"""
    f, _, i = value.partition(",")
    f = _floats(f)
    if len(f) != 1 or not (math.isfinite(f[0]) and f[0] >= 0) or not low <= _uint(i) <= high:
        raise ValueError("%s line: %s= takes a number >= 0 and an integer %d..%d: %r" % (word, key, low, high, value))
    return f[0], int(i)


def _uint_in(word, text, low, high):
    if text is None or not low <= _uint(text) <= high:
        raise ValueError("%s line: a number %d..%d expected, not %r" % (word, low, high, text))
    return int(text)


# ------------------------------------------------------------------------------------------------------
# the mid= token and the file names that go with it
# ------------------------------------------------------------------------------------------------------
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


# ------------------------------------------------------------------------------------------------------
# the solve line and the `layers` line: the two forms that are deliberately loose
# ------------------------------------------------------------------------------------------------------
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


def parse_extra(tokens):
    """optional tokens after a line's paths: bwd=PATH.flo, occ=PATH.png, occ_bwd=PATH.png, mid=I1,I2,..:PREFIX,
    diag=PATH.txt, fold=PATH.png (DESIGN.md "Fold diagnostics") -> {key: value}.  Any other token is ignored, and so is an
    empty value (a line's tokens after the sixth always were); a malformed mid= token is an error (parse_mid)."""
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
    return _outputs(EXTRA_KEYS, extra)


def parse_solve(tokens):
    if len(tokens) < 6:
        raise ValueError("list line needs 6 paths: %r" % _text(tokens))
    return SolveLine(*tokens[:6], extra=parse_extra(tokens[6:]))


def solve_line(item):
    """the inverse of parse_solve"""
    return _text(list(item[:6]) + extra_tokens(item.extra))


class LayersLine(NamedTuple):
    """a `layers` line (DESIGN.md "Layered warp"), recognised by its first word: the layered warp of one frame
        layers RGB n MASK_1 FLO_1 ... MASK_n FLO_n [occ=P] [bwd=P] [occ_bwd=P] [rgb2=P] [mask2=P] [mid=I1,I2,..:PREFIX]
    `layers`: [(mask, flo)] in layer order (the later on top); `out`: {key: path} in line order, a repeated key keeping its
    first place and its last value.  At least one output; anything else after the layers is an error (a new line form has
    no old meaning to keep)."""
    rgb: str
    layers: list
    out: dict


def parse_layers(tokens):
    layers, end = _layer_head(LAYERS_WORD, tokens, 2, count=int, paths=False)      # (int: the count as Python reads one)
    out = {}
    for k, v in _key_values(LAYERS_WORD, tokens[end:], LAYER_KEYS):
        if k == "mid":
            parse_mid(v)
        out[k] = v
    return LayersLine(tokens[1], layers, _outs_of(LAYERS_WORD, out, LAYER_KEYS))


def layers_line(item):
    """the inverse of parse_layers; outputs in the order of LAYER_KEYS"""
    return _text([LAYERS_WORD, item.rgb] + _head_tokens(item.layers) + _outputs(LAYER_KEYS, item.out))


# ------------------------------------------------------------------------------------------------------
# the `bg` line
# ------------------------------------------------------------------------------------------------------
class BgLine(NamedTuple):
    """a `bg` line (DESIGN.md "Moving background"), recognised by its first word: the full-frame pass of one pair
        bg BG.png RGB1.png MASK1.png RGB2.png MASK2.png FLOW.flo m=<12 numbers> [mid=I1,..,In:PREFIX mm=<6n numbers>]
           [occ=IN] [bwd=IN] [occ_bwd=IN] out=RGB1_OUT.png,RGB2_OUT.png,FLOW_OUT.flo [occ_out=..] [bwd_out=..]
           [occ_bwd_out=..] [mid_out=PREFIX_OUT]
    MASK1: the solver's mask (red 0 = object); MASK2: a warped mask (non-zero = object).  `m`: M1 then M2, twelve
    float32 written with %.9g, comma separated.  `out`: three paths, any of them empty (not wanted).  `inputs` / `outs`:
    {key: path} over BG_IN_KEYS / BG_OUT_KEYS; an output needs its input.  At least one output.  A repeated token
    replaces the earlier one.
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


def parse_bg(tokens):
    if len(tokens) < 7 or tokens[0] != BG_WORD:
        raise ValueError("not a %s line: %r" % (BG_WORD, _text(tokens)))
    m, out, inputs, outs = None, ("", "", ""), {}, {}
    mid, mm, mid_out = "", None, ""
    for k, v in _key_values(BG_WORD, tokens[7:], ("m", "mid", "mm", "mid_out", "out") + BG_IN_KEYS + BG_OUT_KEYS):
        if k == "m":
            m = _camera(BG_WORD, v, finite=False)
        elif k == "mid":
            parse_mid(v)
            mid = v
        elif k == "mm":
            mm = _floats(v)
        elif k == "mid_out":
            mid_out = v
        elif k == "out":
            out = tuple(v.split(","))
            if len(out) != 3:
                raise ValueError("bg line: out= takes RGB1_OUT,RGB2_OUT,FLOW_OUT (a place may be empty): %r" % v)
        elif k in BG_IN_KEYS:
            inputs[k] = v
        else:
            outs[k] = v
    if m is None:
        raise ValueError("bg line without m=: %r" % _text(tokens))
    for k in outs:
        if k[:-len("_out")] not in inputs:
            raise ValueError("bg line: %s= needs %s=" % (k, k[:-len("_out")]))
    if mid or mm is not None or mid_out:
        if not (mid and mm is not None and mid_out):
            raise ValueError("bg line: mid=, mm= and mid_out= come together: %r" % _text(tokens))
        if len(mm) != 6 * len(parse_mid(mid)[0]):
            raise ValueError("bg line: mm= takes six numbers per index of mid=: %r" % _text(tokens))
    if not any(out) and not outs and not mid_out:
        raise ValueError("bg line without an output: %r" % _text(tokens))
    return BgLine(*tokens[1:7], m=m, inputs=inputs, out=out, outs=outs, mid=mid, mm=mm or (), mid_out=mid_out)


def bg_line(item):
    """the inverse of parse_bg; optional tokens in the order mid=, mm=, BG_IN_KEYS, out=, BG_OUT_KEYS, mid_out="""
    tok = [BG_WORD] + list(item[:6]) + ["m=" + ",".join("%.9g" % v for v in item.m)]
    if item.mid:
        tok += ["mid=" + item.mid, "mm=" + ",".join("%.9g" % v for v in item.mm)]
    tok += _outputs(BG_IN_KEYS, item.inputs)
    if any(item.out):
        tok.append("out=" + ",".join(item.out))
    return _text(tok + _outputs(BG_OUT_KEYS, item.outs) + (["mid_out=" + item.mid_out] if item.mid_out else []))


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


# ------------------------------------------------------------------------------------------------------
# the forms over a frame's layers: `tex`, `trk`, `blur`, `seg`
# ------------------------------------------------------------------------------------------------------
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


def _tex_layer(text):
    q = text.split(",")
    if len(q) != 19 or not all(_UINT.match(v) for v in q[:2] + q[10:]):
        return None
    ints = [int(v) for v in q[:2] + q[10:]]
    fl = _floats(",".join(q[2:10]))
    if len(fl) != 8 or not _finite(fl):
        return None
    if ints[0] >= len(TEX_KINDS) or ints[1] > 0xffffffff or max(ints[2:]) > 255:
        return None
    return TexLayer(ints[0], ints[1], fl[:6], fl[6], fl[7], tuple(ints[2:5]), tuple(ints[5:8]), tuple(ints[8:11]))


def parse_tex(tokens):
    layers, end = _layer_head(TEX_WORD, tokens, 2, paths=False)
    got = _keyed(TEX_WORD, tokens[end:], ("t",) + TEX_KEYS, need=("t",))
    tex = tuple(_tex_layer(q) for q in got["t"].split(";"))
    if len(tex) != len(layers) or None in tex:
        raise ValueError("tex line: t= takes %d layers of 19 numbers: %r" % (len(layers), got["t"]))
    return TexLine(tokens[1], layers, tex, _outs_of(TEX_WORD, got, TEX_KEYS))


def tex_line(item):
    """the inverse of parse_tex: t=, then the outputs in the order of TEX_KEYS"""
    nums = lambda q: ["%d" % q.kind, "%d" % q.seed] + [_f32(v) for v in tuple(q.m) + (q.p0, q.p1)] + \
        ["%d" % c for c in tuple(q.c0) + tuple(q.c1) + tuple(q.c2)]
    return _text([TEX_WORD, item.rgb] + _head_tokens(item.layers) + ["t=" + ";".join(",".join(nums(q)) for q in item.tex)] +
                 _outputs(TEX_KEYS, item.out))


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
    T = _uint(tokens[3]) if len(tokens) > 3 else 0
    if not 1 <= T <= MAX_SNAPSHOTS + 1:
        raise ValueError("%s line: 1..%d states: %r" % (TRK_WORD, MAX_SNAPSHOTS + 1, _text(tokens)))
    layers, end = _layer_head(TRK_WORD, tokens, 2, first=4, width=T + 1)
    out = _keyed(TRK_WORD, tokens[end:], ("out",), need=("out",))["out"]
    return TrkLine(tokens[1], [(q[0], q[1:]) for q in layers], out)


def trk_line(item):
    """the inverse of parse_trk"""
    tok = [TRK_WORD, item.points, str(len(item.layers)), str(len(item.layers[0][1]))]
    for mask, flows in item.layers:
        tok += [mask] + list(flows)
    return _text(tok + ["out=" + item.out])


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
    layers, end = _layer_head(BLUR_WORD, tokens, 2, fixed=1)
    got = _keyed(BLUR_WORD, tokens[end:], ("b", "m") + BLUR_KEYS, need=("b",))
    shutter, samples = _float_uint(BLUR_WORD, "b", got["b"], 1, MAX_BLUR_SAMPLES)
    m = _camera(BLUR_WORD, got["m"]) if "m" in got else ()
    return BlurLine(tokens[1], layers, tokens[end - 1], shutter, samples, m, _outs_of(BLUR_WORD, got, BLUR_KEYS))


def blur_line(item):
    """the inverse of parse_blur: b=, m= if the line has maps, then the outputs in the order of BLUR_KEYS"""
    tok = [BLUR_WORD, item.rgb] + _head_tokens(item.layers) + [item.bg, "b=%s,%d" % (_f32(item.shutter), item.samples)]
    return _text(tok + _camera_tokens(item.m) + _outputs(BLUR_KEYS, item.out))


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
    layers, end = _layer_head(SEG_WORD, tokens, 1)
    got = _keyed(SEG_WORD, tokens[end:], ("s", "m") + SEG_KEYS, need=("s",))
    tau, radius = _float_uint(SEG_WORD, "s", got["s"], 0, SEG_MAX_RADIUS)
    m = _camera(SEG_WORD, got["m"]) if "m" in got else ()
    return SegLine(layers, tau, radius, m, _outs_of(SEG_WORD, got, SEG_KEYS))


def seg_line(item):
    """the inverse of parse_seg: s=, m= if the line has maps, then the outputs in the order of SEG_KEYS"""
    tok = [SEG_WORD] + _head_tokens(item.layers) + ["s=%s,%d" % (_f32(item.tau), item.radius)]
    return _text(tok + _camera_tokens(item.m) + _outputs(SEG_KEYS, item.out))


# ------------------------------------------------------------------------------------------------------
# the `light` line
# ------------------------------------------------------------------------------------------------------
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
    if len(q.m) != 6 or len(q.gain) != 3 or not _finite(fl):
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


def _light_frame(text):
    q = text.split(",")
    if len(q) != 19 or not _UINT.match(q[0]) or not all(_INT.match(v) for v in q[13:15]) or not all(_UINT.match(v) for v in q[15:17]):
        return None
    fl = _floats(",".join(q[1:13] + q[17:]))
    if len(fl) != 14:
        return None
    f = LightFrame(int(q[0]), fl[:6], fl[6], fl[7], fl[8:11], fl[11], int(q[13]), int(q[14]), int(q[15]), int(q[16]), fl[12], fl[13])
    return f if light_frame_ok(f) else None


def _paths_head(word, what, tokens, n):
    """a line's `n` leading paths, `what`: none of them holds a `=`"""
    if len(tokens) <= n or tokens[0] != word or any("=" in t for t in tokens[1:n + 1]):
        raise ValueError("%s line: %s expected, then the tokens: %r" % (word, what, _text(tokens)))


def parse_light(tokens):
    _paths_head(LIGHT_WORD, "two frames, a mask and a cover", tokens, 4)
    got = _keyed(LIGHT_WORD, tokens[5:], ("l",) + LIGHT_KEYS, need=("l",))
    frames = tuple(_light_frame(q) for q in got["l"].split(";"))
    if len(frames) != 2 or None in frames:
        raise ValueError("light line: l= takes two frames of 19 numbers in their ranges: %r" % got["l"])
    return LightLine(*tokens[1:5], frames, _outs_of(LIGHT_WORD, got, LIGHT_KEYS))


def light_line(item):
    """the inverse of parse_light: l=, then the outputs in the order of LIGHT_KEYS"""
    nums = lambda q: ["%d" % q.seed] + [_f32(v) for v in tuple(q.m) + (q.amp, q.vig) + tuple(q.gain) + (q.gamma,)] + \
        ["%d" % v for v in (q.sh_dx, q.sh_dy, q.sh_r, q.sh_g)] + [_f32(q.sigma0), _f32(q.sigma1)]
    tok = [LIGHT_WORD, item.rgb1, item.mask1, item.rgb2, item.cover2, "l=" + ";".join(",".join(nums(q)) for q in item.frames)]
    return _text(tok + _outputs(LIGHT_KEYS, item.out))


# ------------------------------------------------------------------------------------------------------
# the score family, `chain` and `interp`: leading paths, a strict tail, out=
# ------------------------------------------------------------------------------------------------------
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
    _paths_head(word, "two %s files" % what, tokens, 2)
    return _keyed(word, tokens[3:], keys + ("out",), need=("out",))


def parse_score(tokens):
    got = _score_tokens(SCORE_WORD, "flow", SCORE_KEYS, tokens)
    out = got.pop("out")
    return ScoreLine(tokens[1], tokens[2], got, out)


def score_line(item):
    """the inverse of parse_score: the planes in the order of SCORE_KEYS, then out="""
    return _text([SCORE_WORD, item.gt, item.est] + _outputs(SCORE_KEYS, item.planes) + ["out=" + item.out])


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
    got = _score_tokens(TSCORE_WORD, "track", ("s",), tokens)
    scale = _floats(got["s"]) if "s" in got else (1.0, 1.0)
    if len(scale) != 2 or not all(math.isfinite(q) and q > 0 for q in scale):
        raise ValueError("tscore line: s= takes two finite factors > 0: %r" % got["s"])
    return TScoreLine(tokens[1], tokens[2], scale, got["out"])


def tscore_line(item):
    """the inverse of parse_tscore: s= unless it is (1, 1), then out="""
    s = [_f32(v) for v in item.scale]
    return _text([TSCORE_WORD, item.gt, item.est] + (["s=" + ",".join(s)] if s != ["1", "1"] else []) + ["out=" + item.out])


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
    got = _score_tokens(FSCORE_WORD, "frame", FSCORE_KEYS, tokens)
    out = got.pop("out")
    return FScoreLine(tokens[1], tokens[2], got, out)


def fscore_line(item):
    """the inverse of parse_fscore: the planes in the order of FSCORE_KEYS, then out="""
    return _text([FSCORE_WORD, item.ref, item.est] + _outputs(FSCORE_KEYS, item.planes) + ["out=" + item.out])


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


def parse_lscore(tokens):
    got = _score_tokens(LSCORE_WORD, "map", ("l", "r", "skip"), tokens)
    return LScoreLine(tokens[1], tokens[2], _uint_in(LSCORE_WORD, got.get("l"), 1, 255),
                      _uint_in(LSCORE_WORD, got.get("r"), 0, SEG_MAX_RADIUS), got.get("skip"), got["out"])


def lscore_line(item):
    """the inverse of parse_lscore: l=, r=, skip= if given, out="""
    return _text([LSCORE_WORD, item.gt, item.est, "l=%d" % item.L, "r=%d" % item.radius] +
                 (["skip=" + item.skip] if item.skip else []) + ["out=" + item.out])


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


def parse_mscore(tokens):
    got = _score_tokens(MSCORE_WORD, "map", ("t", "r", "skip"), tokens)
    if ("t" in got) != ("r" in got):
        raise ValueError("mscore line: t= and r= come together: %r" % _text(tokens))
    thr, radius = (), None
    if "t" in got:
        thr = tuple(_uint_in(MSCORE_WORD, v, 1, 255) for v in got["t"].split(","))
        radius = _uint_in(MSCORE_WORD, got["r"], 0, SEG_MAX_RADIUS)
        if len(thr) > MSCORE_MAX_THR:
            raise ValueError("mscore line: at most %d thresholds: %r" % (MSCORE_MAX_THR, got["t"]))
    return MScoreLine(tokens[1], tokens[2], thr, radius, got.get("skip"), got["out"])


def mscore_line(item):
    """the inverse of parse_mscore: t= and r= if it has thresholds, skip= if given, out="""
    return _text([MSCORE_WORD, item.gt, item.est] +
                 (["t=" + ",".join("%d" % t for t in item.thr), "r=%d" % item.radius] if item.thr else []) +
                 (["skip=" + item.skip] if item.skip else []) + ["out=" + item.out])


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
    L = _uint(tokens[2]) if len(tokens) > 2 else 0
    if not 1 <= L < TSCORE_MAX_FRAMES:
        raise ValueError("%s line: 1..%d links expected: %r" % (CHAIN_WORD, TSCORE_MAX_FRAMES - 1, _text(tokens)))
    _paths_head(CHAIN_WORD, "a points file, the count and %d flow files" % L, tokens, 2 + L)
    got = _keyed(CHAIN_WORD, tokens[3 + L:], ("bwd", "out"), need=("out",))
    bwd = tuple(got["bwd"].split(",")) if "bwd" in got else ()
    if "bwd" in got and (len(bwd) != L or not all(bwd)):
        raise ValueError("chain line: bwd= takes %d files: %r" % (L, got["bwd"]))
    return ChainLine(tokens[1], tuple(tokens[3:3 + L]), bwd, got["out"])


def chain_line(item):
    """the inverse of parse_chain"""
    return _text([CHAIN_WORD, item.points, str(len(item.flows))] + list(item.flows) +
                 (["bwd=" + ",".join(item.bwd)] if item.bwd else []) + ["out=" + item.out])


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
    _paths_head(INTERP_WORD, "two frame files and a flow file", tokens, 3)
    got = _keyed(INTERP_WORD, tokens[4:], ("s", "n", "bwd", "src", "out"), need=("s", "n", "out"))
    n, steps = _uint(got["n"]), tuple(_uint(v) for v in got["s"].split(","))
    if not (len(steps) <= INTERP_MAX_TIMES and 1 <= steps[0] and steps[-1] < n < 1 << 32 and all(a < b for a, b in zip(steps, steps[1:]))):
        raise ValueError("interp line: s=I1,I2,.. n=N with 1 <= I1 < I2 < .. < N, at most %d steps: %r" % (INTERP_MAX_TIMES, _text(tokens)))
    if got.get("src", "1") != "1":
        raise ValueError("interp line: src=1 or no src=: %r" % _text(tokens))
    return InterpLine(tokens[1], tokens[2], tokens[3], steps, n, got.get("bwd", ""), "src" in got, got["out"])


def interp_line(item):
    """the inverse of parse_interp: s=, n=, bwd=, src=, out= in that order"""
    return _text([INTERP_WORD, item.a, item.b, item.fwd, "s=" + ",".join("%d" % i for i in item.steps), "n=%d" % item.n] +
                 (["bwd=" + item.bwd] if item.bwd else []) + (["src=1"] if item.src else []) + ["out=" + item.out])


def interp_files(prefix, step):
    """the files of an `interp` line for ramp step `step`: the frame (mid_files' name) and its source map"""
    return dict(rgb=mid_files(prefix, step)["rgb"], src="%s_s%02d_src.png" % (prefix, step))


def interp_times(steps, n):
    """the times of an interp line, float32: (float)I / (float)N"""
    return np.array([np.float32(i) / np.float32(n) for i in steps], np.float32)


# ------------------------------------------------------------------------------------------------------
# the table of forms
# ------------------------------------------------------------------------------------------------------
class Form(NamedTuple):
    """one form of list line: its first word (None: the solve line, the form of every line without a known first word),
    the type of its item, its parser (tokens -> item), its writer (item -> text), and `done`, the path `arap_deform
    --serve` reports the item done by.  (How an item is run: run_lines.RUN, by type.)"""
    word: Optional[str]
    type: type
    parse: Callable
    write: Callable
    done: Callable


def _first_out(item):
    """the first output token ON THE LINE"""
    return next(iter(item.out.values()))


_out = attrgetter("out")                # an out= file, or an interp line's out= prefix
FORMS = {f.word: f for f in (
    Form(None, SolveLine, parse_solve, solve_line, attrgetter("flow")),
    Form(LAYERS_WORD, LayersLine, parse_layers, layers_line, _first_out),
    Form(BG_WORD, BgLine, parse_bg, bg_line, lambda item: bg_outputs(item)[0]),
    Form(TEX_WORD, TexLine, parse_tex, tex_line, _first_out),
    Form(TRK_WORD, TrkLine, parse_trk, trk_line, _out),
    Form(BLUR_WORD, BlurLine, parse_blur, blur_line, _first_out),
    Form(LIGHT_WORD, LightLine, parse_light, light_line, _first_out),
    Form(SEG_WORD, SegLine, parse_seg, seg_line, _first_out),
    Form(SCORE_WORD, ScoreLine, parse_score, score_line, _out),
    Form(TSCORE_WORD, TScoreLine, parse_tscore, tscore_line, _out),
    Form(CHAIN_WORD, ChainLine, parse_chain, chain_line, _out),
    Form(FSCORE_WORD, FScoreLine, parse_fscore, fscore_line, _out),
    Form(INTERP_WORD, InterpLine, parse_interp, interp_line, _out),
    Form(LSCORE_WORD, LScoreLine, parse_lscore, lscore_line, _out),
    Form(MSCORE_WORD, MScoreLine, parse_mscore, mscore_line, _out))}
FORM_OF = {f.type: f for f in FORMS.values()}


def parse_line(line):
    """a list line, as text or as its tokens -> the item of the form its first word names in FORMS"""
    tok = line.split() if isinstance(line, str) else list(line)
    return FORMS.get(tok[0] if tok else None, FORMS[None]).parse(tok)


def format_line(item):
    """the inverse of parse_line: the text of a list line, as its form's writer puts it"""
    return FORM_OF[type(item)].write(item)


def done_token(item):
    """the path `arap_deform --serve` reports a line done by (Form.done)"""
    return FORM_OF[type(item)].done(item)


def read_list_items(path):
    """every non-blank line of a list file in order, parsed (parse_line)"""
    with open(path) as f:
        return [parse_line(line) for line in f if line.strip()]
