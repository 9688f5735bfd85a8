"""Numpy twin of DESIGN.md "Moving background over in-between frames" (k_bg_seq in arap_flow_amd/csrc/arap_bg.h).  By the
section's identity I2 link f of a sequence is tests/bg_ref.background on the pair (F_f, F_{f+1}) with the own mask of a
later frame given in the solver's convention, where(cover_f != 0, 0, 255); so the twin is a loop over the links plus the
last frame's composite, and states nothing of its own about a pixel.  The point maps are an input, as in bg_ref."""
import ctypes

import numpy as np

import bg_ref

F = np.float32
OUTPUTS = ("out_rgb", "flow_full", "occ_full")
# the shapes of tests/test_gpu_background_seq.py: (W, H, bgW, bgH, (window left, top), frames).  67x9: partial blocks in x
# and y, a first, two middle and a last frame; 130x70 with 10 frames: several blocks each way, the argument table full
SIZES = {"67x9": (67, 9, 80, 23, (6, 7), 4), "130x70": (130, 70, 150, 90, (10, 10), 10)}


def own_mask(cover):
    """a cover (object: != 0) as a solver mask (object: == 0)"""
    return np.where(cover != 0, 0, 255).astype(np.uint8)


def background_seq(bg, maps, Gs, mask_red, covers, rgbs, flows, occs=None):
    """every output of ArapFlow_BackgroundSeq whose input is given: {name: list}, out_rgb per frame, flow_full and occ_full
    per link, None where the input is missing.  maps [m][6]; Gs [m - 1][6], the point map of every link; covers[0] is not
    read."""
    m = len(maps)
    occs = [None] * (m - 1) if occs is None else occs
    out = dict(out_rgb=[None] * m, flow_full=[None] * (m - 1), occ_full=[None] * (m - 1))
    for f in range(m - 1):
        own = mask_red if f == 0 else own_mask(covers[f])
        last = f == m - 2
        r = bg_ref.background(bg, maps[f], maps[f + 1], Gs[f], bg_ref.IDENTITY, rgbs[f], own,
                              rgbs[f + 1] if last else None, covers[f + 1], flows[f], occs[f])
        out["out_rgb"][f] = r.get("out_rgb1")
        out["flow_full"][f], out["occ_full"][f] = r.get("flow_full"), r.get("occ_full")
        if last:
            out["out_rgb"][f + 1] = r.get("out_rgb2")
    return out


def library_G(Ma, Mb):
    """the G of ArapFlow_BackgroundMaps(Ma, Mb): the library's own bits (host only, no GPU)"""
    from arap_flow_amd import build
    lib = ctypes.CDLL(build.build())
    fn = lib.ArapFlow_BackgroundMaps
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.POINTER(ctypes.c_float)] * 4
    arr = lambda m: (ctypes.c_float * 6)(*[float(v) for v in np.asarray(m, F)])
    g, gi = (ctypes.c_float * 6)(), (ctypes.c_float * 6)()
    if fn(arr(Ma), arr(Mb), g, gi) != 0:
        raise ValueError("ArapFlow_BackgroundMaps refuses the maps")
    return np.array(g[:], F)


def link_maps(maps, G=library_G):
    return [G(maps[f], maps[f + 1]) for f in range(len(maps) - 1)]


def camera(M1, m, W, H, deg=3.0, scale=1.02, shift=(2.5, -1.25)):
    """m sampling maps from M1 on: frame f at the fraction f / (m - 1) of a similarity about the frame centre"""
    centre = ((W - 1) / 2.0, (H - 1) / 2.0)
    maps = [np.asarray(M1, F)]
    for f in range(1, m):
        t = f / (m - 1.0)
        maps.append(bg_ref.compose(M1, bg_ref.similarity(t * deg, scale ** t, (t * shift[0], t * shift[1]), centre)))
    return np.stack(maps)


def seq_case(W, H, bw, bh, m, seed=0):
    """m frames for the tests, seeded: bg_ref.ellipse_case is frame 0 (solver mask, rgb, bg); frame f >= 1 has its own
    random rgb and as cover the ellipse moved on by (1, 0) per frame and grown a little, so that covers differ from frame
    to frame; link f has a synthetic object-side flow that depends on f and is 0 off the object of F_f, and a random
    object-side occlusion (off the object it is not read)."""
    c = bg_ref.ellipse_case(W, H, bw, bh, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    ys, xs = np.mgrid[0:H, 0:W]
    covers, rgbs, flows, occs = [None], [c["rgb1"]], [], []
    for f in range(1, m):
        inside = ((xs - 0.45 * W - f) / ((0.22 + 0.004 * f) * W)) ** 2 + ((ys - 0.5 * H) / (0.3 * H)) ** 2 <= 1
        covers.append(np.where(inside, 255, 0).astype(np.uint8))
        rgbs.append(rng.integers(0, 256, (H, W, 3)).astype(np.uint8))
    for f in range(m - 1):
        obj = c["mask_red"] == 0 if f == 0 else covers[f] != 0
        fl = np.stack([1.25 + 0.125 * f + 0.02 * (ys - H / 2), -0.5 + 0.03 * (xs - W / 2) - 0.0625 * f], -1).astype(F)
        fl[~obj] = 0
        flows.append(fl)
        occs.append(np.where(rng.integers(0, 2, (H, W)) != 0, 255, 0).astype(np.uint8))
    out = dict(bg=c["bg"], mask_red=c["mask_red"], covers=covers, rgbs=rgbs, flows=flows, occs=occs, W=W, H=H, m=m)
    for v in out.values():
        for a in (v if isinstance(v, list) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return out


def sized_case(name):
    """the case of SIZES[name] with its camera: seq_case plus `maps`"""
    W, H, bw, bh, (left, top), m = SIZES[name]
    c = seq_case(W, H, bw, bh, m, seed=W)
    c["maps"] = camera(np.array([1, 0, left, 0, 1, top], F), m, W, H)
    return c


def link_coverage(c, Gs, f):
    """what link f of case c exercises: counts of object pixels and, among the background pixels of F_f, of targets that
    leave the frame, targets hidden by the next cover, and visible ones"""
    W, H = c["W"], c["H"]
    obj = c["mask_red"] == 0 if f == 0 else c["covers"][f] != 0
    px, py = bg_ref.apply_map(Gs[f], W, H)
    inside = (px >= 0) & (px <= F(W - 1)) & (py >= 0) & (py <= F(H - 1))
    hid = bg_ref.hidden(px, py, c["covers"][f + 1] != 0, W, H)
    return dict(object=int(obj.sum()), background=int((~obj).sum()), leaves=int((~obj & ~inside).sum()),
                covered=int((~obj & inside & hid).sum()), visible=int((~obj & ~hid).sum()))
