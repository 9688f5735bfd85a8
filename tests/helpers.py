"""Shared builders for the parity tests."""
import numpy as np


def random_problem(W, H, seed, generic_urshape=True, mask_frac=0.25, ncons=12):
    """Random masked problem with non-zero angles, generic UrShape, a negative-target constraint and
    a duplicate-source constraint (tier T1)."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    grid = np.stack([xs, ys], -1).astype(np.float64)
    M = (rng.random((H, W)) < mask_frac).astype(np.float64) * 255.0
    U = grid + (rng.normal(size=(H, W, 2)) * 0.3 if generic_urshape else 0.0)
    O = U + rng.normal(size=(H, W, 2)) * 0.5
    A = rng.normal(size=(H, W)) * 0.4
    C = -np.ones((H, W, 2))
    for _ in range(ncons):
        x, y = rng.integers(0, W), rng.integers(0, H)
        C[y, x] = np.array([x, y]) + rng.normal(size=2) * 2 + 3.0
    C[H // 2, W // 3] = [-0.5, 4.0]          # negative coordinate: silently inactive (arap_plan.t:22)
    C[H // 3, W // 2] = [0.0, 0.0]           # exactly zero is valid (greatereq)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    return dict(O=f32(O), A=f32(A), U=f32(U), C=f32(C), M=f32(M), wf=np.float32(10.0), wr=np.float32(0.1))


def para_gen_flags(extra):
    """para_gen.py's parsed flags for a run over precomputed matches, plus the arguments in `extra`"""
    import para_gen
    return para_gen.parse(["--input", "in", "--output", "out", "--matches", "m"] + extra)


RECORDING_WORKER = r'''
import os, shutil, sys
# stand-in for arap_deform (no GPU), for every form of line para_gen hands out: a line is logged, REFUSED (exit 3) when a
# file it reads is not there yet (or no longer), and answered by a placeholder at every output path it names -- real
# pictures, flows and diag files where para_gen's back end reads them (tests/helpers.py: recording_worker)
import numpy as np
from PIL import Image
sys.path.insert(0, %r)
from arap_flow_amd import flo as F, pipeline
from arap_flow_amd.run_lines import format_diag
LOG = %r

def layer_files(layers):
    return [q for mask, flows in layers for q in [mask] + ([flows] if isinstance(flows, str) else list(flows))]

def snapshots(token):
    steps, prefix = pipeline.parse_mid(token)
    return steps, [pipeline.mid_files(prefix, i) for i in steps]

def reads(it):
    if isinstance(it, pipeline.SolveLine):
        return list(it[:3])
    if isinstance(it, pipeline.LayersLine):
        mids = [q for _, flo in it.layers for f in snapshots("%%s:%%s" %% (it.out["mid"].split(":")[0], flo[:-4]))[1]
                for q in f.values()] if "mid" in it.out else []
        return [it.rgb] + layer_files(it.layers) + mids
    if isinstance(it, pipeline.BgLine):
        mids = []
        if it.mid:
            steps, files = snapshots(it.mid)
            mids = [q for f in files for q in f.values()]
            if "occ" in it.inputs:
                prefix = pipeline.parse_mid(it.mid)[1]
                mids += [pipeline.mid_layer_files(prefix, i)["occ"] for i in (0,) + tuple(steps)]
        return list(it[:6]) + list(it.inputs.values()) + mids
    if isinstance(it, pipeline.TrkLine):
        return [it.points] + layer_files(it.layers)
    if isinstance(it, pipeline.LightLine):
        return list(it[:4])
    if isinstance(it, pipeline.BlurLine):
        return [it.rgb, it.bg] + layer_files(it.layers)
    if isinstance(it, pipeline.TexLine):
        return [it.rgb] + layer_files(it.layers)
    return layer_files(it.layers)                       # a seg line

def put(path, like, shape):
    """a placeholder of the kind the path's name asks for; a picture that is there already (a bg line's own frame) stays"""
    if path.endswith(".flo"):
        F.flow_write(path, np.zeros(shape + (2,), np.float32))
    elif path.endswith(".txt"):
        open(path, "w").write(format_diag(dict(vertices=4, outside=0, triangles=2, folded=0, nonfinite=0,
                                               det_min=1.0, det_max=1.0, disp2_max=0.0)))
    elif path.endswith(".png") and like is not None:
        if not os.path.exists(path):
            shutil.copy(like, path)
    else:
        open(path, "w").write("placeholder\n")

def run(line):
    it = pipeline.parse_line(line)
    with open(LOG, "a") as log:
        log.write(line.rstrip("\n") + "\n")
    for q in reads(it):
        if not os.path.exists(q):
            print("%%s line before (or after) its input %%s" %% (type(it).__name__, q), flush=True)
            sys.exit(3)
    if isinstance(it, pipeline.SolveLine):
        m = np.array(Image.open(it.mask).convert("RGB"))[..., 0]
        F.flow_write(it.flow, np.zeros(m.shape + (2,), np.float32))
        shutil.copy(it.rgb, it.out_rgb)
        Image.fromarray(m == 0).save(it.out_mask)
        for k, q in it.extra.items():
            if k == "mid":
                for f in snapshots(q)[1]:
                    F.flow_write(f["flow"], np.zeros(m.shape + (2,), np.float32)); F.flow_write(f["step"], np.zeros(m.shape + (2,), np.float32))
                    shutil.copy(it.rgb, f["rgb"]); Image.fromarray(m == 0).save(f["mask"])
            elif q.endswith(".png"):
                Image.fromarray(np.zeros(m.shape, np.uint8)).save(q)
            else:
                put(q, None, m.shape)
        return
    if isinstance(it, pipeline.BgLine):
        like, outs = it.rgb2, pipeline.bg_outputs(it)
    elif isinstance(it, pipeline.TrkLine):
        like, outs = None, [it.out]
    else:
        like = it.rgb1 if isinstance(it, pipeline.LightLine) else getattr(it, "rgb", None) or it.layers[0][0]
        outs = [q for k, q in it.out.items() if k != "mid"]
        if "mid" in it.out:                             # a layers line: the merged snapshots and, with occ=, the link occlusions
            steps, files = snapshots(it.out["mid"])
            outs += [q for f in files for q in f.values()]
            if "occ" in it.out:
                outs += [pipeline.mid_layer_files(pipeline.parse_mid(it.out["mid"])[1], i)["occ"] for i in (0,) + tuple(steps)]
    shape = np.array(Image.open(like if like else it.layers[0][0])).shape[:2]
    for q in outs:
        put(q, like, shape)

if sys.argv[1] == "--serve":
    print("Ready", flush=True)
    for line in sys.stdin:
        run(line)
        print("Done " + pipeline.done_token(pipeline.parse_line(line)), flush=True)
else:
    for l in open(sys.argv[1]).read().splitlines():
        if l.strip(): run(l)
'''


def recording_worker(path, log, root):
    """writes RECORDING_WORKER to `path` (its log at `log`, this repository at `root`) -> the --arap_bin that runs it"""
    import sys
    with open(str(path), "w") as f:
        f.write(RECORDING_WORKER % (str(root), str(log)))
    return "%s %s" % (sys.executable, path)


def rel_l2(a, b):
    a = np.asarray(a, np.float64).ravel()
    b = np.asarray(b, np.float64).ravel()
    den = np.sqrt((b * b).sum())
    return np.sqrt(((a - b) ** 2).sum()) / (den if den > 0 else 1.0)


def neg_det_quads(flow, act):
    """number of mesh quads (all four corners active) whose lower-left triangle is inverted"""
    H, W = act.shape
    ys, xs = np.mgrid[0:H, 0:W]
    P = flow + np.stack([xs, ys], -1)
    a = P[:-1, 1:] - P[:-1, :-1]
    b = P[1:, :-1] - P[:-1, :-1]
    det = a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]
    q = act[:-1, :-1] & act[:-1, 1:] & act[1:, :-1] & act[1:, 1:]
    return int(((det < 0) & q).sum())


def warp_live_case():
    """input of the warp test against the reference's warp_image on a fresh random folded flow (tests/test_oracle.py);
    the binary's outputs on it are kept in tests/golden/warp_live/ (tests/golden/make_golden.py)"""
    rng = np.random.default_rng(5)
    W, H = 70, 50
    rgb = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    mask = np.where(rng.random((H, W)) < 0.15, 255, 0).astype(np.uint8)
    fl = (rng.normal(size=(H, W, 2)) * 3.0).astype(np.float32)
    fl[mask != 0] = 0
    return rgb, mask, fl


def run_ref_warp(ref, rgb, mask, fl, d):
    """the reference's warp_image (oracle/_ref/) on (rgb, mask, fl), files in directory d -> (warped rgb, warped mask)"""
    import os
    import subprocess
    from PIL import Image
    from arap_flow_amd import flo
    p = lambda n: os.path.join(str(d), n)
    Image.fromarray(rgb).save(p("i.png"))
    Image.fromarray(np.stack([mask] * 3, -1)).save(p("m.png"))
    flo.flow_write(p("f.flo"), fl)
    subprocess.check_call([ref, p("i.png"), p("m.png"), p("f.flo"), p("o.png"), p("om.png")], stdout=subprocess.DEVNULL)
    return np.array(Image.open(p("o.png")).convert("RGB")), np.array(Image.open(p("om.png")).convert("L"))


def load_cat512(golden_dir):
    import os
    from PIL import Image
    from arap_flow_amd import flo, opt
    d = os.path.join(golden_dir, "cat512")
    rgb = np.array(Image.open(os.path.join(d, "cat512_iRGB.png")).convert("RGB"))
    mred = np.array(Image.open(os.path.join(d, "cat512_iMsk.png")).convert("RGBA"))[..., 0]
    cons = opt.load_constraints(os.path.join(d, "cat512_iCstr.txt"))
    gflow = flo.flow_read(os.path.join(d, "cat512_iFlo.flo"))
    wrgb = np.array(Image.open(os.path.join(d, "cat512_wRGB.png")).convert("RGB"))
    wmsk = np.array(Image.open(os.path.join(d, "cat512_wMsk.png")).convert("L"))
    return dict(rgb=rgb, mask_red=mred, constraints=cons, golden_flow=gflow, golden_wrgb=wrgb, golden_wmsk=wmsk)


def t4_bands(golden_dir):
    """Tier T4 acceptance bands from the committed calibration table tests/golden/t4_variants.json (made by
    tests/golden/make_t4_variants.py): 39 trajectories besides the product's own -- seven other arithmetic variants of
    the CPU oracle (f32 / f64, sequential / float64 sums, libm / spec trig, fused multiply-adds on / off), 20 runs of the
    product's arithmetic and 12 of f32_sum64_libm_nofma from an initial Angle perturbed by N(0, 1e-6 rad), all on the
    reference's cat512 fixture, full 19/8/400 schedule.  Every one of them is a correct evaluation of the reference's
    algorithm; the bands are EMPIRICAL: what those 39 span, widened by 10 % (the product's own row is left out, so no band
    is drawn around the value under test):
      cost      : [0.9 x smallest, 1.1 x largest] final cost (they scatter over 52.9 .. 63.4, mean 58.7, standard
                  deviation 2.4: the final cost of this unconverged schedule is a random variable of the rounding
                  trajectory; a 1e-6 rad perturbation of the start moves it by up to 13 %)
      rel_l2    : 1.1 x the largest rel-L2 to the reference golden (0.0117; 7 of the 39 exceed SURVEY 8c's 1e-2)
      median_px : 1.1 x their largest median error
      handle_px : 2e-4 px, SURVEY 8c's bound (the product measures 1.8e-4; 10 of the 39 correct trajectories sit at
                  2.1e-4 .. 7.6e-4, so this bound is as tight as the algorithm's own scatter allows)"""
    import json
    import os
    tab = json.load(open(os.path.join(golden_dir, "t4_variants.json")))
    others = [v for k, v in tab["variants"].items() if k != tab["product_variant"]]
    for key in tab:
        if key.startswith("perturbed_starts_"):
            others += list(tab[key].values())
    costs = [v["final_cost"] for v in others]
    return dict(cost=(0.9 * min(costs), 1.1 * max(costs)),
                rel_l2=1.1 * max(v["rel_l2_vs_golden"] for v in others),
                median_px=1.1 * max(v["median_px_vs_golden"] for v in others),
                handle_px=2e-4, quads=5, table=tab, n=len(others))
