"""The executors of the list lines of lines.py: image and flow files in, one or a few calls into arap_flow_amd.opt (the
GPU), files out.

  run_list                  a whole list in order: runs of solve lines through deform_list, any other line through RUN
  RUN                       the `run` column of lines.FORMS: a line's type -> its run_* function
  deform_list               ARAP/deformation/src/main.cpp:162-241  (arap_deform over a list of solves)
  warp_files                ARAP/warping/src/main.cpp:302-336      (warp_image)
`opt` is imported inside the functions that need it: this module is importable without libarapopt.so.
"""
import os.path as osp
from itertools import groupby

import numpy as np
from PIL import Image

from . import flo
from .lines import (SolveLine, LayersLine, BgLine, TexLine, TrkLine, BlurLine, LightLine, SegLine, ScoreLine, TScoreLine,
                    ChainLine, FScoreLine, InterpLine, LScoreLine, MScoreLine, LAYERS_WORD, TEX_WORD, TRK_WORD, BLUR_WORD,
                    SEG_WORD, SCORE_WORD, FSCORE_WORD, LSCORE_WORD, MSCORE_WORD, parse_mid, mid_files, mid_layer_files,
                    mid_bg_files, interp_files, interp_times)
from .scores import format_score, format_track_score, format_frame_score, format_label_score, format_map_score


# ------------------------------------------------------------------------------------------------------
# the files the executors share
# ------------------------------------------------------------------------------------------------------
def load_rgb(path):
    return np.array(Image.open(path).convert("RGB"))


def load_mask_red(path):
    """red channel of the mask PNG (CombinedSolver.h:213,234): 0 = deformable object"""
    return np.array(Image.open(path).convert("RGB"))[..., 0]


def save_mask(mask, path):
    """LodePNG writes the 0/255 warped mask as a 1-bit image: np.array(Image.open()) of
    it is bool, which para_gen.py's flatten relies on only through != 0 / == 0."""
    Image.fromarray(np.ascontiguousarray(mask) > 0).save(path)


def save_occ(occ, path):
    """an occlusion map as an 8-bit L PNG, 0 / 255"""
    Image.fromarray(np.ascontiguousarray(occ, np.uint8), "L").save(path)


def seg_dist_png(d2):
    """a distance map as its file shows it: the integer square root of the uint16 squared distance, 255 for the sentinel
    65535 (isqrt(65535) = 255; every other value is <= 254^2)"""
    # (exact: the float64 root of an integer below 2^16 is an integer or at least 2^-9 away from one)
    return np.floor(np.sqrt(np.asarray(d2, np.uint16).astype(np.float64))).astype(np.uint8)


def dist_from_png(u8):
    """the squared distance a seg line's 8-bit distance file stands for: d * d, 255 -> 65535.  Not seg_dist_png's inverse,
    but floor(sqrt(d2)) < r is d2 < r * r, so every pixel is in the band of the d2 the file was made from"""
    d = np.asarray(u8, np.uint8).astype(np.uint16)
    return np.where(d == 255, np.uint16(65535), d * d).astype(np.uint16)


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


# the lines of a diag file: ArapFlow_MeshStats in the struct's order, without `reserved` (DESIGN.md "Fold diagnostics")
DIAG_COUNTS = ("vertices", "outside", "triangles", "folded", "nonfinite")
DIAG_FLOATS = ("det_min", "det_max", "disp2_max")


def format_diag(stats):
    """the text of a diag file: eight lines `name value`, counts in decimal, floats as printf's %.9g of the float32
    (inf, -inf as printf writes them); the C++ worker writes the same bytes.  (pipeline.parse_diag reads it back.)"""
    return "".join(["%s %d\n" % (k, int(stats[k])) for k in DIAG_COUNTS] +
                   ["%s %.9g\n" % (k, float(np.float32(stats[k]))) for k in DIAG_FLOATS])


def _write_text(path, text):
    with open(path, "w") as f:
        f.write(text)


def _load_layers(word, layers, shape, what, masks=True, flows=True):
    """the masks (red channels) and the flows of a layer list [(mask, flo)], each stacked (None when not asked for); every
    one has the size `shape[:2]` -- without a `shape`, the first mask's -- or the line is refused: `what` sizes differ"""
    m = [load_mask_red(q) for q, _ in layers] if masks else []
    f = [flo.flow_read(q) for _, q in layers] if flows else []
    shape = m[0].shape if shape is None else tuple(shape[:2])
    if any(a.shape[:2] != shape for a in m + f):
        raise ValueError("%s line: %s sizes differ" % (word, what))
    return np.stack(m) if masks else None, np.stack(f) if flows else None


# ------------------------------------------------------------------------------------------------------
# one function per form
# ------------------------------------------------------------------------------------------------------
def run_layers(state, spec):
    """one `layers` line: read the frame's RGB and every layer's mask / flow, one opt.warp_layers, write what the line
    asks for (occ / occ_bwd: 8-bit L PNG; bwd: .flo; rgb2: RGB PNG; mask2: 1-bit PNG as a solve's warped mask; mid:
    run_layers_mid)"""
    from . import opt
    rgb = load_rgb(spec.rgb)
    masks, flows = _load_layers(LAYERS_WORD, spec.layers, rgb.shape, "image, mask and flow")
    out = spec.out
    if "mid" in out:
        run_layers_mid(state, spec, rgb, masks, flows)
    if not set(out) - {"mid"}:
        return
    r = opt.warp_layers(state, rgb, masks, flows, bwd="bwd" in out, occ_bwd="occ_bwd" in out, occ="occ" in out)
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


def run_layers_mid(state, spec, rgb, masks, flows):
    """the mid= token of a `layers` line (DESIGN.md "Layered in-between frames").  Layer l's state after ramp step i is
    the file mid_files(stem_l, i)["flow"], stem_l = FLO_l without its `.flo`; after the last snapshot comes the layers'
    final flow.  Per snapshot one opt.warp_layers_step, written as mid_files(PREFIX, i): the owner_flow of the snapshot,
    the composite in-between frame and mask, the step flow; with occ= on the line also the link occlusions of
    mid_layer_files, steps 0 (frame 1 -> first snapshot, opt.warp_layers' occlusion) and i."""
    from . import opt
    out = spec.out
    steps, prefix = parse_mid(out["mid"])
    states = []
    for i in steps:
        per = []
        for _, f in spec.layers:
            if not f.endswith(".flo"):
                raise ValueError("layers line: mid= needs flows named *.flo, got %s" % f)
            snap = mid_files(f[:-4], i)["flow"]
            if not osp.exists(snap):
                raise ValueError("layers line: snapshot %s is missing" % snap)
            per.append(flo.flow_read(snap))
            if per[-1].shape != flows[0].shape:
                raise ValueError("layers line: %s differs in size from %s" % (snap, spec.rgb))
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


def run_texture(state, spec):
    """one `tex` line: read the frame's RGB and every layer's mask (and, for rgb2 / mask2, flow) once, one opt.texture
    and, if rgb2 or mask2 is wanted, one opt.warp_layers on its result; write what the line asks for (rgb1, rgb2: RGB
    PNG; mask2: 1-bit PNG as a solve's warped mask)"""
    from . import opt
    rgb = load_rgb(spec.rgb)
    masks, _ = _load_layers(TEX_WORD, spec.layers, rgb.shape, "image and mask", flows=False)
    out = spec.out
    rgb1 = opt.texture(state, rgb, masks, spec.tex)
    if "rgb1" in out:
        Image.fromarray(rgb1).save(out["rgb1"])
    if "rgb2" in out or "mask2" in out:
        _, flows = _load_layers(TEX_WORD, spec.layers, rgb.shape, "image and flow", masks=False)
        r = opt.warp_layers(state, rgb1, masks, flows, occ=False)
        if "rgb2" in out:
            Image.fromarray(r["warped_rgb"]).save(out["rgb2"])
        if "mask2" in out:
            save_mask(r["warped_mask"], out["mask2"])


def run_tracks(state, spec):
    """one `trk` line: read the points, every layer's mask and its T state flows, one opt.track_points, write the track
    file: frame 0 the points themselves (occ by in_frame), frames 1 .. T the states"""
    from . import opt, trk
    pts = trk.read(spec.points)
    if pts["pos"].shape[0] != 1:
        raise ValueError("trk line: %s is no points file (%d frames)" % (spec.points, pts["pos"].shape[0]))
    W, H = pts["W"], pts["H"]
    masks, _ = _load_layers(TRK_WORD, spec.layers, (H, W), "points and mask", flows=False)
    flows = np.stack([_load_layers(TRK_WORD, [(m, fl[s]) for m, fl in spec.layers], (H, W), "mask and flow", masks=False)[1]
                      for s in range(len(spec.layers[0][1]))])
    r = opt.track_points(state, masks, flows, pts["pos"][0])
    first = np.where(trk.in_frame(pts["pos"][0], W, H), 0, 255).astype(np.uint8)
    trk.write(spec.out, W, H, np.concatenate([pts["pos"], r["pos"]]), np.concatenate([first[None], r["occ"]]))


def run_blur(state, spec):
    """one `blur` line: read the frame's RGB, every layer's mask and flow and the background picture once, one
    opt.blur_layers per frame the line asks for (rgb1 / alpha1: centre 0, rgb2 / alpha2: centre 1), write the outputs (rgb:
    RGB PNG; alpha: 8-bit L PNG)"""
    from . import opt
    rgb, bg = load_rgb(spec.rgb), load_rgb(spec.bg)
    masks, flows = _load_layers(BLUR_WORD, spec.layers, rgb.shape, "image, mask and flow")
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


def run_seg(state, spec):
    """one `seg` line: read every layer's mask and flow, one opt.seg_maps for the outputs the line asks for, write them as
    8-bit L PNGs (SegLine)"""
    from . import opt
    masks, flows = _load_layers(SEG_WORD, spec.layers, None, "mask and flow")
    M1, M2 = (spec.m[:6], spec.m[6:]) if len(spec.m) else (None, None)
    r = opt.seg_maps(state, masks, flows, tau=spec.tau, radius=spec.radius, M1=M1, M2=M2, which=tuple(spec.out))
    for k, path in spec.out.items():
        save_occ(seg_dist_png(r[k]) if k.startswith("dist") else r[k], path)


def _load_score_planes(word, planes, like, like_path):
    """{key: the red channel of its file} of a line's planes, each of the size of the array `like` read from `like_path`"""
    plane = {}
    for k, path in planes.items():
        plane[k] = load_mask_red(path)
        if plane[k].shape != like.shape[:2]:
            raise ValueError("%s line: %s differs in size from %s" % (word, path, like_path))
    return plane


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


def run_tscore(state, spec):
    """one `tscore` line: read the two track files, one opt.track_score, write the table as text"""
    from . import opt, trk
    gt, est = trk.read(spec.gt), trk.read(spec.est)
    if (gt["W"], gt["H"]) != (est["W"], est["H"]) or gt["pos"].shape != est["pos"].shape:
        raise ValueError("tscore line: %s and %s differ in W, H, F or P" % (spec.gt, spec.est))
    table = opt.track_score(state, gt["pos"], gt["occ"], est["pos"], est["occ"], scale=spec.scale)
    _write_text(spec.out, format_track_score(table))
    return table


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


# ------------------------------------------------------------------------------------------------------
# the solve lines of a list: arap_deform
# ------------------------------------------------------------------------------------------------------
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
        _write_text(extra["diag"], format_diag(r["mesh_stats"]))
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


# the `run` column of lines.FORMS: how a line that is no solve is run, run(state, item)
RUN = {LayersLine: run_layers, BgLine: run_background, TexLine: run_texture, TrkLine: run_tracks, BlurLine: run_blur,
       LightLine: run_light, SegLine: run_seg, ScoreLine: run_score, TScoreLine: run_tscore, ChainLine: run_chain,
       FScoreLine: run_fscore, InterpLine: run_interp, LScoreLine: run_lscore, MScoreLine: run_mscore}


def run_list(state, lines, num_iter, non_linear_iter, linear_iter):
    """a list's lines in order: every run of solve lines goes to deform_list, the batched solver; any other line runs
    (RUN) once the run before it is solved and written -- its inputs may be their outputs -- and prints `Saved`"""
    for solves, run in groupby(lines, lambda ln: type(ln) is SolveLine):
        if solves:
            deform_list(state, list(run), num_iter, non_linear_iter, linear_iter)
            continue
        for ln in run:
            RUN[type(ln)](state, ln)
            print("Saved")


def warp_files(state, rgb_path, mask_path, flo_path, out_rgb_path, out_mask_path, extra=None):
    """warp_image (ARAP/warping/src/main.cpp:302-336); `extra` ({key: path}, parse_extra): the optional outputs"""
    from . import opt
    rgb, mask, fl = load_rgb(rgb_path), load_mask_red(mask_path), flo.flow_read(flo_path)
    if fl.shape[:2] != mask.shape or rgb.shape[:2] != mask.shape:
        raise ValueError("image, mask and flow sizes differ")
    if extra and {"diag", "fold"} & set(extra):
        d = opt.warp_diag(state, mask, fl, fold="fold" in extra)
        if "diag" in extra:
            _write_text(extra["diag"], format_diag(d["stats"]))
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
