"""GPU: motion-blurred frames (ArapFlow_BlurLayers, DESIGN.md "Motion blur") through opt.blur_layers against the numpy twin
tests/blur_ref.py, byte for byte, and against the existing rasteriser (the integer mean of S opt.warp_layers calls).

Shapes: 70x9 (two block columns and three block rows of the 64x4 blocks, the last one partial each way) and 130x70
(several full blocks), one layer and three overlapping ones, folded flows with whole-pixel shifts that throw the layers
over each other and partly out of frame (occ_layers_ref.layered_case).  Sample counts straddle the chunk carry:
1, 2, 5, G, G + 1 (a last chunk of one sample), 32 (four full chunks).  The kernels have no other size-dependent path."""
import ctypes as C

import numpy as np
import pytest
import torch

import bg_ref
import blur_ref
import occ_layers_ref
from arap_flow_amd import capi, opt

pytestmark = pytest.mark.gpu
F = np.float32
G = capi.BLUR_CHUNK
CASES = {"70x9-n1": (70, 9, 1), "70x9-n3": (70, 9, 3), "130x70-n3": (130, 70, 3)}
SAMPLES = (1, 2, 5, G, G + 1, 32)


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name, (W, H, n) in CASES.items():
        rgb, masks, flows = occ_layers_ref.layered_case(W, H, n, seed=W + n, overlap=True)
        rng = np.random.default_rng(7 * W + n)
        flows_a = (rng.normal(size=flows.shape) * 0.75).astype(F)
        flows_a[masks != 0] = 0
        bg = rng.integers(0, 256, (H + 13, W + 9, 3)).astype(np.uint8)
        # a rotated and scaled camera that moves during the exposure
        Ma = bg_ref.similarity(4.0, 1.05, (3.5, 2.25), (W / 2, H / 2))
        Mb = bg_ref.similarity(-3.0, 0.95, (5.0, 4.5), (W / 2, H / 2))
        c = dict(W=W, H=H, n=n, rgb=rgb, masks=masks, flows=flows, flows_a=flows_a, bg=bg, Ma=Ma, Mb=Mb)
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        out[name] = c
    return out


def same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    assert got.tobytes() == want.tobytes(), "%d bytes differ" % int((got != want).sum())


RENDERS = {}             # (flows_b, flows_a) by identity -> blur_ref's cache of per-time renders


def twin(c, centre, shutter, S, flows_a=None, bg=False):
    kw = dict(bg=c["bg"], Ma=c["Ma"], Mb=c["Mb"]) if bg else {}
    zero = flows_a is None or not np.any(flows_a)
    cache = RENDERS.setdefault((id(c["flows"]), None if zero else id(flows_a)), {})
    return blur_ref.blur_ref(c["rgb"], c["masks"], c["flows"], centre, shutter, S, flows_a=flows_a, cache=cache, **kw)


def gpu(st, c, centre, shutter, S, flows_a=None, bg=False, **kw):
    if bg:
        kw.update(bg=c["bg"], maps=(c["Ma"], c["Mb"]))
    return opt.blur_layers(st, c["rgb"], c["masks"], c["flows"], centre, shutter, S, flows_a=flows_a, **kw)


@pytest.mark.parametrize("S", SAMPLES)
@pytest.mark.parametrize("name", ["70x9-n1", "70x9-n3"])
def test_twin_small(gpu_state, cases, name, S):
    """every centre and shutter, with and without the moving camera, at the small shape"""
    c = cases[name]
    for centre in (0.0, 1.0):
        for shutter in (0.5, 1.0):
            for bg in (False, True):
                got, want = gpu(gpu_state, c, centre, shutter, S, bg=bg), twin(c, centre, shutter, S, bg=bg)
                same(got[0], want[0])
                same(got[1], want[1])
                assert S == 1 or (want[1] > 0).any() and (want[1] < 255).any()     # partly covered pixels exist


@pytest.mark.parametrize("S", SAMPLES)
def test_twin_large(gpu_state, cases, S):
    """the same at 130x70: several full blocks in both directions"""
    c = cases["130x70-n3"]
    for centre in (0.0, 1.0):
        for shutter in (0.5, 1.0):
            for bg in (False, True):
                got, want = gpu(gpu_state, c, centre, shutter, S, bg=bg), twin(c, centre, shutter, S, bg=bg)
                same(got[0], want[0])
                same(got[1], want[1])


@pytest.mark.parametrize("name", list(CASES))
def test_first_state(gpu_state, cases, name):
    """flows_a NULL and an array of zeros give the same bytes; a real first state around c = 0.5, over the chunk carry"""
    c = cases[name]
    zeros = np.zeros_like(c["flows"])
    for S in (5, G + 1):
        want = twin(c, 0.5, 1.0, S, bg=True)
        for fa in (None, zeros):
            got = gpu(gpu_state, c, 0.5, 1.0, S, flows_a=fa, bg=True)
            same(got[0], want[0])
            same(got[1], want[1])
        got, want = gpu(gpu_state, c, 0.5, 1.0, S, flows_a=c["flows_a"], bg=True), twin(c, 0.5, 1.0, S, flows_a=c["flows_a"], bg=True)
        same(got[0], want[0])
        same(got[1], want[1])
        assert got[0].tobytes() != gpu(gpu_state, c, 0.5, 1.0, S, bg=True)[0].tobytes()      # the first state matters


@pytest.mark.parametrize("S", (2, G + 1))
@pytest.mark.parametrize("name", ["70x9-n3", "130x70-n3"])
def test_mean_of_warps(gpu_state, cases, name, S):
    """without the twin: the integer mean of S opt.warp_layers calls on the numpy-interpolated flows"""
    c = cases[name]
    H, W = c["H"], c["W"]
    total, cnt = np.zeros((H, W, 3), np.int64), np.zeros((H, W), np.int64)
    for t in blur_ref.times(1.0, 0.5, S):
        r = opt.warp_layers(gpu_state, c["rgb"], c["masks"], blur_ref.mix(c["flows_a"], c["flows"], t), occ=False)
        total += r["warped_rgb"]
        cnt += r["warped_mask"] != 0
    rgb, alpha = gpu(gpu_state, c, 1.0, 0.5, S, flows_a=c["flows_a"])
    same(rgb, blur_ref.mean_rgb(total, S))
    same(alpha, blur_ref.mean_alpha(cnt, S))


@pytest.mark.parametrize("name", list(CASES))
def test_one_sample_is_the_warp(gpu_state, cases, name):
    """S = 1, c = 1, no bg: ArapFlow_WarpLayers(flows_b), whatever the shutter"""
    c = cases[name]
    r = opt.warp_layers(gpu_state, c["rgb"], c["masks"], c["flows"], occ=False)
    for shutter in (0.0, 0.5, 1.0):
        rgb, alpha = gpu(gpu_state, c, 1.0, shutter, 1)
        same(rgb, r["warped_rgb"])
        same(alpha, r["warped_mask"])


@pytest.mark.parametrize("S", (5, G + 1))
def test_still_camera(gpu_state, cases, S):
    """Ma == Mb: a pixel no sample covers shows opt.background's background sample, alpha is 255 exactly where every sample
    covers the pixel"""
    c = cases["130x70-n3"]
    rgb, alpha = opt.blur_layers(gpu_state, c["rgb"], c["masks"], c["flows"], 1.0, 1.0, S, bg=c["bg"], maps=(c["Ma"], c["Ma"]))
    want = twin(dict(c, Mb=c["Ma"]), 1.0, 1.0, S, bg=True)
    same(rgb, want[0])
    same(alpha, want[1])
    H, W = c["H"], c["W"]
    nothing = np.full((H, W), 255, np.uint8)                       # a frame 1 without object: every pixel is background
    back = opt.background(gpu_state, c["bg"], c["Ma"], c["Ma"], np.zeros((H, W, 3), np.uint8), nothing, None,
                          np.zeros((H, W), np.uint8), None, want=["out_rgb1"])["out_rgb1"]
    never = alpha == 0
    assert never.any()
    same(rgb[never], back[never])
    cover = np.stack([opt.warp_layers(gpu_state, None, c["masks"], blur_ref.mix(None, c["flows"], t), occ=False)["warped_mask"]
                      for t in blur_ref.times(1.0, 1.0, S)]) != 0
    assert cover.all(0).any()
    assert ((alpha == 255) == cover.all(0)).all()


def test_either_output_alone_and_two_runs(gpu_state, cases):
    c = cases["70x9-n3"]
    S = G + 1
    both = gpu(gpu_state, c, 0.0, 1.0, S, bg=True)
    again = gpu(gpu_state, c, 0.0, 1.0, S, bg=True)
    same(again[0], both[0])
    same(again[1], both[1])
    rgb, none = gpu(gpu_state, c, 0.0, 1.0, S, bg=True, want=("rgb",))
    assert none is None
    same(rgb, both[0])
    none, alpha = gpu(gpu_state, c, 0.0, 1.0, S, bg=True, want=("alpha",))
    assert none is None
    same(alpha, both[1])


@pytest.mark.parametrize("S", (3, G + 1))
def test_keys_left_clean(gpu_state, cases, S):
    """a warp_layers call before and after a blur on the same state is unchanged"""
    c = cases["70x9-n3"]
    before = opt.warp_layers(gpu_state, c["rgb"], c["masks"], c["flows"], bwd=True, occ_bwd=True)
    gpu(gpu_state, c, 1.0, 1.0, S, bg=True)
    after = opt.warp_layers(gpu_state, c["rgb"], c["masks"], c["flows"], bwd=True, occ_bwd=True)
    for k in before:
        same(after[k], before[k])


def test_scratch_is_cleared_by_the_call(gpu_state, cases):
    """a scratch buffer full of ones gives the bytes of a fresh one, and the keys are zero again after the call"""
    c = cases["70x9-n3"]
    W, H, n, S = c["W"], c["H"], c["n"], G + 1
    lib = gpu_state.lib
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = [up(c[k]) for k in ("rgb", "masks", "flows")]
    rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    alpha = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    nbytes = int(lib.ArapFlow_BlurLayersScratchBytes(W, H, n, S))
    assert nbytes >= (G + 1) * 8 * W * H
    scratch = torch.full((nbytes,), 255, dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    rc = lib.ArapFlow_BlurLayers(gpu_state.handle, W, H, n, p(d[0]), p(d[1]), None, p(d[2]), 1.0, 0.5, S, None, 0, 0, None, None,
                                 p(rgb), p(alpha), p(scratch))
    assert rc == 0
    torch.cuda.synchronize()
    want = gpu(gpu_state, c, 1.0, 0.5, S)
    same(rgb.cpu().numpy(), want[0])
    same(alpha.cpu().numpy(), want[1])
    assert not scratch[:G * 8 * W * H].any().item()


def test_bad_arguments(gpu_state, cases):
    """every bad argument returns -1 and leaves the outputs untouched"""
    c = cases["70x9-n3"]
    W, H, n, S = c["W"], c["H"], c["n"], 5
    lib = gpu_state.lib
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = {k: up(c[k]) for k in ("rgb", "masks", "flows", "flows_a", "bg")}
    out_rgb = torch.full((H, W, 3), 77, dtype=torch.uint8, device="cuda")
    out_alpha = torch.full((H, W), 77, dtype=torch.uint8, device="cuda")
    scratch = torch.zeros(int(lib.ArapFlow_BlurLayersScratchBytes(W, H, n, 32)), dtype=torch.uint8, device="cuda")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    m6 = lambda m: None if m is None else (C.c_float * 6)(*[float(v) for v in m])
    bgH, bgW = c["bg"].shape[:2]
    good = dict(state=gpu_state.handle, W=W, H=H, n=n, rgb=d["rgb"], masks=d["masks"], flows_a=d["flows_a"], flows_b=d["flows"],
                centre=1.0, shutter=0.5, samples=S, bg=d["bg"], bgW=bgW, bgH=bgH, Ma=c["Ma"], Mb=c["Mb"], out_rgb=out_rgb,
                out_alpha=out_alpha, scratch=scratch)

    def call(**change):
        a = dict(good, **change)
        return lib.ArapFlow_BlurLayers(a["state"], a["W"], a["H"], a["n"], p(a["rgb"]), p(a["masks"]), p(a["flows_a"]),
                                       p(a["flows_b"]), a["centre"], a["shutter"], a["samples"], p(a["bg"]), a["bgW"], a["bgH"],
                                       m6(a["Ma"]), m6(a["Mb"]), p(a["out_rgb"]), p(a["out_alpha"]), p(a["scratch"]))
    nan, inf = float("nan"), float("inf")
    bad_map = np.array(c["Ma"])
    bad_map[4] = nan
    bad = [dict(state=None), dict(rgb=None), dict(masks=None), dict(flows_b=None), dict(scratch=None),
           dict(out_rgb=None, out_alpha=None), dict(n=0), dict(n=256), dict(W=0), dict(H=0), dict(W=1 << 16, H=1 << 15),
           dict(samples=0), dict(samples=33), dict(shutter=nan), dict(shutter=inf), dict(shutter=-0.5), dict(centre=nan),
           dict(centre=inf), dict(Ma=None), dict(Mb=None), dict(bgW=0), dict(bgH=0), dict(Ma=bad_map), dict(Mb=bad_map),
           dict(out_rgb=d["rgb"]), dict(out_alpha=d["masks"]), dict(out_rgb=d["flows"]), dict(out_alpha=d["flows_a"]),
           dict(out_rgb=d["bg"]), dict(out_alpha=scratch)]
    torch.cuda.synchronize()
    for change in bad:
        assert call(**change) == -1, change
    torch.cuda.synchronize()
    assert (out_rgb == 77).all().item() and (out_alpha == 77).all().item()
    for k in ("rgb", "masks", "flows", "flows_a", "bg"):
        same(d[k].cpu().numpy(), np.ascontiguousarray(c[k]))
    assert lib.ArapFlow_BlurLayersScratchBytes(W, H, n, 0) == 0 and lib.ArapFlow_BlurLayersScratchBytes(W, H, n, 33) == 0
    assert lib.ArapFlow_BlurLayersScratchBytes(W, H, 0, S) == 0 and lib.ArapFlow_BlurLayersScratchBytes(1 << 16, 1 << 15, n, S) == 0
    assert call() == 0                                                     # and the good call is good
    torch.cuda.synchronize()
    want = twin(c, 1.0, 0.5, S, flows_a=c["flows_a"], bg=True)
    same(out_rgb.cpu().numpy(), want[0])
    same(out_alpha.cpu().numpy(), want[1])
    with pytest.raises(ValueError):
        opt.blur_layers(gpu_state, c["rgb"], c["masks"], c["flows"], 1.0, 0.5, 33)
    with pytest.raises(ValueError):
        opt.blur_layers(gpu_state, c["rgb"], c["masks"], c["flows"], 1.0, -1.0, 3)


def test_blur_pair(gpu_state, cases):
    c = cases["70x9-n3"]
    (r1, a1), (r2, a2) = opt.blur_pair(gpu_state, c["rgb"], c["masks"], c["flows"], 0.5, 9, bg=c["bg"], maps=(c["Ma"], c["Mb"]))
    for (r, a), centre in (((r1, a1), 0.0), ((r2, a2), 1.0)):
        want = twin(c, centre, 0.5, 9, bg=True)
        same(r, want[0])
        same(a, want[1])
