"""Numpy twin of DESIGN.md "Training clips" (arap_flow_amd/csrc/arap_clip.h, ArapFlow_AugmentClips), written from that
text: plain float32 numpy, one operator per IEEE operation in the order of the parentheses.  What the feature shares with
"Training batches" -- apply, the taps, mix, the image, the flow of a link with its used / bad-tap rule and guard, the
tables' expressions -- is imported from tests/aug_ref.py, not restated.  `tables` is the Python statement of
ArapFlow_ClipTables; a comparison with the device passes the library's own tables (opt.clip_tables) so that the C
library's pow is stated once.  A frame is (T, gain, gamma, erase, fill), opt.ClipFrame's order."""
import numpy as np

import aug_ref
from aug_ref import F

OUTPUTS = ("video", "flows", "valid", "tracks", "vis")
FLT_MAX = np.finfo(F).max


def tables(frame, scale=(1, 1, 1), bias=(0, 0, 0)):
    """(P f32[6], lut f32[3,256]) of a frame: aug_ref.tables' P2 and lut[1] of a sample whose second frame it is.  A frame
    the library refuses (det(T) == 0 included, for every frame) is a ValueError."""
    T, gain, gamma = frame[:3]
    P, lut = aug_ref.tables((T, T, gain, gamma, gain, gamma), scale, bias)
    return P, lut[1]


def erased(frame, w, h):
    """bool[h,w]: the output pixels inside any of the frame's rectangles"""
    return aug_ref.erased((None,) * 6 + (frame[3],), w, h)


def track(pos, occ, P, frame, w, h):
    """pos f32[P,2], occ u8[P] of one frame -> (tracks f32[P,2], vis bool[P], reasons {name: bool[P]})"""
    P = np.asarray(P, F)
    px, py = np.asarray(pos, F)[:, 0], np.asarray(pos, F)[:, 1]
    ox, oy = (P[0] * px + P[1] * py) + P[2], (P[3] * px + P[4] * py) + P[5]
    fin = (np.abs(ox) <= FLT_MAX) & (np.abs(oy) <= FLT_MAX)                       # False on NaN
    ox, oy = np.where(fin, ox, F(0)), np.where(fin, oy, F(0))
    left, right, above, below = ox < 0, ox > F(w - 1), oy < 0, oy > F(h - 1)
    inn = fin & ~left & ~right & ~above & ~below
    rx = np.where(inn, np.floor(ox + F(0.5)), 0).astype(np.int64)
    ry = np.where(inn, np.floor(oy + F(0.5)), 0).astype(np.int64)
    hit = np.zeros(len(px), bool)
    for x0, y0, x1, y1 in frame[3]:
        hit |= (rx >= x0) & (rx < x1) & (ry >= y0) & (ry < y1)
    hit &= inn
    hidden = np.asarray(occ) != 0
    why = {"occ": hidden, "left": fin & left, "right": fin & right, "above": fin & above, "below": fin & below, "erased": hit,
           "nonfinite": ~fin}
    return np.stack([ox, oy], -1).astype(F), ~hidden & inn & ~hit, why


def augment(frames, samples, size, links=(), flows=None, skip=None, pos=None, occ=None, scale=(1, 1, 1), bias=(0, 0, 0), tau=1.0,
            want=None, tables=tables, reasons=False):
    """ArapFlow_AugmentClips on numpy arrays: frames u8[B,T,H,W,3], flows f32[B,L,H,W,2], skip u8[B,L,H,W] or None, pos
    f32[B,T,P,2], occ u8[B,T,P]; samples: B lists of T frames -> {name: array} of the outputs `want` names (by default
    every one whose inputs are given): video f32[B,T,3,h,w], flows f32[B,L,2,h,w], valid u8[B,L,h,w], tracks f32[B,T,P,2],
    vis u8[B,T,P]; with `reasons` also {"reasons": [per clip [per frame {occ, left, right, above, below, erased,
    nonfinite: bool[P]}]]}."""
    w, h = size
    if want is None:
        given = {"video": frames is not None, "flows": flows is not None, "valid": flows is not None, "tracks": pos is not None,
                 "vis": pos is not None and occ is not None}
        want = tuple(k for k in OUTPUTS if given[k])
    links = [tuple(l) for l in links]
    out = {k: [] for k in want}
    why = []
    with np.errstate(all="ignore"):
        for b, clip in enumerate(samples):
            tabs = [tables(f, scale, bias) for f in clip]
            row = {k: [] for k in want}
            if "video" in want:
                for t, f in enumerate(clip):
                    img = aug_ref.image(np.asarray(frames[b][t]), tabs[t][1], f[0], w, h)
                    row["video"].append(np.where(erased(f, w, h)[None], np.asarray(f[4], F)[:, None, None], img).astype(F))
            if "flows" in want or "valid" in want:
                for l, (i, j) in enumerate(links):
                    o, valid, _ = aug_ref.flow_of(np.asarray(flows[b][l], F), None if skip is None else np.asarray(skip[b][l]),
                                                  clip[i][0], tabs[j][0], w, h, tau)
                    if "flows" in want:
                        row["flows"].append(o)
                    if "valid" in want:
                        row["valid"].append(np.where(valid, 255, 0).astype(np.uint8))
            if "tracks" in want or "vis" in want or reasons:
                per_frame = []
                for t, f in enumerate(clip):
                    flags = np.zeros(len(pos[b][t]), np.uint8) if occ is None else occ[b][t]
                    o, vis, r = track(pos[b][t], flags, tabs[t][0], f, w, h)
                    per_frame.append(r)
                    if "tracks" in want:
                        row["tracks"].append(o)
                    if "vis" in want:
                        row["vis"].append(np.where(vis, 255, 0).astype(np.uint8))
                why.append(per_frame)
            for k in want:
                out[k].append(row[k])
    T, L = len(samples[0]), len(links)
    P = 0 if pos is None else np.shape(pos)[2]
    form = {"video": ((T, 3, h, w), F), "flows": ((L, 2, h, w), F), "valid": ((L, h, w), np.uint8), "tracks": ((T, P, 2), F),
            "vis": ((T, P), np.uint8)}
    res = {k: np.asarray(v, form[k][1]).reshape((len(samples),) + form[k][0]) for k, v in out.items()}
    if reasons:
        res["reasons"] = why
    return res


def as_augment(state, frames, samples, size, links=(), flows=None, skip=None, pos=None, occ=None, scale=(1, 1, 1), bias=(0, 0, 0),
               tau=1.0, want=None, out=None, tables=tables):
    """the twin behind opt.augment_clips' signature, on host tensors or arrays -> {name: host tensor}: what
    data.ClipLoader takes as `augment` (state: unused)"""
    import torch
    host = lambda a: None if a is None else np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a)
    r = augment(host(frames), samples, size, links=links, flows=host(flows), skip=host(skip), pos=host(pos), occ=host(occ),
                scale=scale, bias=bias, tau=tau, want=want, tables=tables)
    return {k: torch.from_numpy(v) for k, v in r.items()}


def write_clip_tree(root, n, W, H, steps=(4, 9, 14), P=5, seed=0, named_root=None, occ_every=2, tracks=True, layers=True):
    """a `--mid K --tracks P` tree in miniature under `root`: n pairs of W x H in two sequences; per pair the two frames,
    its flow and (every `occ_every`-th pair) OUT/Occ; under OUT/Mid/<seq>/ per ramp step II the in-between frame
    <frame>_sII.png, the flow from frame 1 <frame>_sII.flo and the link flow <frame>_sII_step.flo, with `layers` also the
    links' occlusions <frame>_sII_occ.png (step 0: the link frame 1 -> first snapshot) for the even pairs; with `tracks`
    OUT/Tracks/<seq>/<frame>.trk of len(steps) + 2 frames and P points.  all_files.list names the files under
    `named_root` (default: root).  Returns per pair dict(frames u8[T,H,W,3], step f32[T-1,H,W,2] (link t -> t+1), first
    f32[T-1,H,W,2] (0 -> k), occ_step [T-1 of u8[H,W] or None], occ_pair u8[H,W] or None, pos, occ)."""
    import os
    import os.path as osp
    from PIL import Image
    from arap_flow_amd import flo, lines, trk
    rng = np.random.default_rng(seed)
    named_root = named_root or root
    T = len(steps) + 2

    def put(d, seq, name, write):
        os.makedirs(osp.join(root, d, seq), exist_ok=True)
        write(osp.join(root, d, seq, name))
        return osp.join(named_root, d, seq, name)
    png = lambda a: (lambda p: Image.fromarray(a).save(p))
    made, listed = [], []
    ys, xs = np.mgrid[0:H, 0:W]
    for i in range(n):
        seq, stem = "seq%d" % (i % 2), "%05d" % i
        frames = rng.integers(0, 256, (T, H, W, 3)).astype(np.uint8)
        field = lambda k: (np.stack([xs * 0.03 + i + k, ys * 0.05 - i - k], -1) + rng.integers(-8, 9, (H, W, 2)) / 64.0).astype(F)
        first = np.stack([field(k) for k in range(1, T)])                       # 0 -> k; the last one is the pair's flow
        step = np.stack([first[0]] + [field(10 + k) for k in range(1, T - 1)])  # t -> t + 1; link 0 is the first snapshot's flow
        first[T - 2][i % H, (3 * i + 1) % W] = np.nan
        item = dict(frames=frames, step=step, first=first, occ_step=[None] * (T - 1), occ_pair=None, pos=None, occ=None)
        names = [put("inpRGB", seq, stem + ".png", png(frames[0])), put("wRGB", seq, stem + ".png", png(frames[T - 1])),
                 put("Flow", seq, stem + ".flo", lambda p: flo.flow_write(p, first[T - 2]))]
        listed.append(" ".join(names))
        prefix = osp.join(root, "Mid", seq, stem)
        os.makedirs(osp.dirname(prefix), exist_ok=True)
        for k, s in enumerate(steps):
            files = lines.mid_files(prefix, s)
            Image.fromarray(frames[k + 1]).save(files["rgb"])
            flo.flow_write(files["flow"], first[k])
            flo.flow_write(files["step"], step[k + 1])
        if layers and i % 2 == 0:
            for k, s in enumerate((0,) + tuple(steps)):
                a = np.where(rng.random((H, W)) < 0.1, 255, 0).astype(np.uint8)
                item["occ_step"][k] = a
                Image.fromarray(a).save(lines.mid_layer_files(prefix, s)["occ"])
        if i % occ_every == 0:
            a = np.where(rng.random((H, W)) < 0.1, 255, 0).astype(np.uint8)
            item["occ_pair"] = a
            put("Occ", seq, stem + ".png", png(a))
        if tracks:
            pos = (rng.uniform(-2, 1, (T, P, 2)) + rng.uniform(0, 1, (1, P, 2)) * [W, H]).astype(F)
            occ = np.where(rng.random((T, P)) < 0.2, 255, 0).astype(np.uint8)
            item["pos"], item["occ"] = pos, occ
            put("Tracks", seq, stem + ".trk", lambda p: trk.write(p, W, H, pos, occ))
        made.append(item)
    open(osp.join(root, "all_files.list"), "w").write("\n".join(listed))
    return made
