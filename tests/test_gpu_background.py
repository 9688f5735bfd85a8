"""GPU: the moving background (ArapFlow_Background, DESIGN.md "Moving background") through the C ABI against the numpy
twin tests/bg_ref.py, fed with the library's own point maps (ArapFlow_BackgroundMaps).

Shapes: a 67x9 frame over an 80x23 picture (W no multiple of 64, H no multiple of 4, one partial block each way) and a
130x70 frame over a 150x90 picture (several blocks each way).  The kernels have no other size-dependent path."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import bg_ref
from arap_flow_amd import opt, pipeline

pytestmark = pytest.mark.gpu
F = np.float32
SIZES = {"67x9": (67, 9, 80, 23, (6, 7)), "130x70": (130, 70, 150, 90, (10, 10))}
INPUTS = ("rgb1", "mask_red", "rgb2", "cover2", "flow", "occ", "bwd", "occ_bwd")
NEEDS = dict(out_rgb1="rgb1", out_rgb2="rgb2", flow_full="flow", occ_full="occ", bwd_full="bwd", occ_bwd_full="occ_bwd")


@pytest.fixture(scope="module")
def cases(gpu_state):
    """per size: the ellipse pair, its warp (cover2, rgb2 and the object-side maps from opt.warp_image_ex) and M1"""
    out = {}
    for name, (W, H, bw, bh, (left, top)) in SIZES.items():
        c = bg_ref.ellipse_case(W, H, bw, bh, seed=W)
        r = opt.warp_image_ex(gpu_state, c["rgb1"], c["mask_red"], c["flow"])
        c.update(rgb2=r["warped_rgb"], cover2=r["warped_mask"], occ=r["occlusion"], bwd=r["backward_flow"],
                 occ_bwd=r["occlusion_bwd"], M1=np.array([1, 0, left, 0, 1, top], F), W=W, H=H, win=(left, top))
        assert (c["cover2"] != 0).any() and (c["cover2"] == 0).any() and (c["occ_bwd"] == 255).any()
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        out[name] = c
    return out


def run(state, c, M2, want=None):
    return opt.background(state, c["bg"], c["M1"], M2, c["rgb1"], c["mask_red"], c["rgb2"], c["cover2"], c["flow"],
                          occ=c["occ"], bwd=c["bwd"], occ_bwd=c["occ_bwd"], want=want)


def twin(c, M2):
    G, Ginv = opt.background_maps(c["M1"], M2)
    return bg_ref.background(c["bg"], c["M1"], M2, G, Ginv, c["rgb1"], c["mask_red"], c["rgb2"], c["cover2"], c["flow"],
                             c["occ"], c["bwd"], c["occ_bwd"])


def assert_same(got, want):
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), "%s: %d differ" % (k, int((got[k] != want[k]).sum()))


def centre(c):
    return ((c["W"] - 1) / 2.0, (c["H"] - 1) / 2.0)


def test_background_maps(cases):
    c = cases["67x9"]
    M2 = bg_ref.compose(c["M1"], bg_ref.similarity(3.0, 1.02, (2.5, -1.25), centre(c)))
    G, Ginv = opt.background_maps(c["M1"], M2)
    wg, wgi = bg_ref.maps_f64(c["M1"], M2)
    assert G.dtype == Ginv.dtype == F
    assert np.abs(G - wg).max() <= 1e-6 * np.abs(wg).max() and np.abs(Ginv - wgi).max() <= 1e-6 * np.abs(wgi).max()
    for M in (c["M1"], M2):
        G, Ginv = opt.background_maps(M, M)
        assert G.tobytes() == Ginv.tobytes() == bg_ref.IDENTITY.tobytes()
    with pytest.raises(ValueError):
        opt.background_maps(c["M1"], [1, 2, 0, 2, 4, 0])


@pytest.mark.parametrize("size", list(SIZES))
def test_similarity_equals_twin(gpu_state, cases, size):
    c = cases[size]
    M2 = bg_ref.compose(c["M1"], bg_ref.similarity(3.0, 1.02, (2.5, -1.25), centre(c)))
    got = run(gpu_state, c, M2)
    assert_same(got, twin(c, M2))
    bgpix = c["mask_red"] != 0
    assert np.abs(got["flow_full"][bgpix]).max() > 1 and (got["occ_full"][bgpix] == 255).any()


@pytest.mark.parametrize("size", list(SIZES))
def test_same_map_is_the_static_background(gpu_state, cases, size):
    c = cases[size]
    got = run(gpu_state, c, c["M1"])
    left, top = c["win"]
    win = c["bg"][top:top + c["H"], left:left + c["W"]]
    assert np.array_equal(got["out_rgb1"], pipeline.add_bg(c["rgb1"], np.where(c["mask_red"] == 0, 1, 0), win))
    assert np.array_equal(got["out_rgb2"], pipeline.add_bg(c["rgb2"], c["cover2"], win))
    for k, src in (("flow_full", "flow"), ("occ_full", "occ"), ("bwd_full", "bwd"), ("occ_bwd_full", "occ_bwd")):
        assert got[k].tobytes() == c[src].tobytes(), k


@pytest.mark.parametrize("size", list(SIZES))
def test_integer_shift(gpu_state, cases, size):
    c = cases[size]
    W, H = c["W"], c["H"]
    left, top = c["win"]
    dx, dy = 3, -2
    M2 = c["M1"] + np.array([0, 0, dx, 0, 0, dy], F)          # frame 2 looks (dx, dy) further into the picture
    got = run(gpu_state, c, M2)
    bg1, cov = c["mask_red"] != 0, c["cover2"] != 0
    assert (got["flow_full"][bg1] == np.array([-dx, -dy], F)).all()
    assert (got["bwd_full"][~cov] == np.array([dx, dy], F)).all()
    crop = c["bg"][top + dy:top + dy + H, left + dx:left + dx + W]
    assert np.array_equal(got["out_rgb2"][~cov], crop[~cov]) and np.array_equal(got["out_rgb2"][cov], c["rgb2"][cov])
    # forward occlusion of the background by slicing: the target (x - dx, y - dy) is outside the frame or on cover2
    hid = np.ones((H, W), bool)
    ys, xs = slice(max(0, dy), H + min(0, dy)), slice(max(0, dx), W + min(0, dx))
    yt, xt = slice(max(0, -dy), H + min(0, -dy)), slice(max(0, -dx), W + min(0, -dx))
    hid[ys, xs] = cov[yt, xt]
    assert np.array_equal(got["occ_full"][bg1] == 255, hid[bg1])
    assert np.array_equal(got["occ_full"][~bg1], c["occ"][~bg1])


def test_targets_outside_frame_and_picture(gpu_state, cases):
    c = cases["67x9"]
    M2 = bg_ref.compose(c["M1"], bg_ref.similarity(0.0, 3.0, (0.0, 0.0), (0.0, 0.0)))
    got = run(gpu_state, c, M2)
    assert_same(got, twin(c, M2))
    assert np.isfinite(got["flow_full"]).all() and np.isfinite(got["bwd_full"]).all()
    sx, sy = bg_ref.apply_map(M2, c["W"], c["H"])
    bh, bw = c["bg"].shape[:2]
    assert ((sx > bw - 1) | (sy > bh - 1)).mean() > 0.5                     # most samples are clamped
    qx, qy = bg_ref.apply_map(opt.background_maps(c["M1"], M2)[1], c["W"], c["H"])
    assert ((qx > c["W"] - 1) | (qy > c["H"] - 1)).mean() > 0.5             # most backward targets leave the frame
    assert (got["occ_bwd_full"][c["cover2"] == 0] == 255).mean() > 0.5


def test_every_subset_of_outputs(gpu_state, cases):
    c = cases["67x9"]
    M2 = bg_ref.compose(c["M1"], bg_ref.similarity(3.0, 1.02, (2.5, -1.25), centre(c)))
    full = run(gpu_state, c, M2)
    for n in range(1, 6):
        for want in itertools.combinations(opt.BG_OUTPUTS, n):
            assert_same(run(gpu_state, c, M2, want=list(want)), {k: full[k] for k in want})


def raw_call(state, c, M1, M2, want, drop=(), bg_size=None):
    """ArapFlow_Background on device tensors: (return code, inputs on the device, outputs prefilled with 0xA5)"""
    W, H = c["W"], c["H"]
    dev = {k: torch.from_numpy(np.array(c[k])).cuda() for k in INPUTS + ("bg",)}
    shape = dict(out_rgb1=(H, W, 3), out_rgb2=(H, W, 3), flow_full=(H, W, 8), occ_full=(H, W), bwd_full=(H, W, 8),
                 occ_bwd_full=(H, W))
    outs = {k: torch.full(shape[k], 0xA5, dtype=torch.uint8, device="cuda") for k in want}
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    m = lambda v: (C.c_float * 6)(*[float(q) for q in v])
    bw, bh = bg_size or (c["bg"].shape[1], c["bg"].shape[0])
    torch.cuda.synchronize()
    rc = state.lib.ArapFlow_Background(state.handle, W, H, p(None if "bg" in drop else dev["bg"]), bw, bh, m(M1), m(M2),
                                       *[p(None if k in drop else dev[k]) for k in INPUTS],
                                       *[p(outs.get(k)) for k in opt.BG_OUTPUTS])
    torch.cuda.synchronize()
    return rc, dev, outs


def test_bad_arguments_launch_nothing(gpu_state, cases):
    c = cases["67x9"]
    M2 = bg_ref.compose(c["M1"], bg_ref.similarity(3.0, 1.02, (2.5, -1.25), centre(c)))
    every = list(opt.BG_OUTPUTS)
    bad = [dict(want=every, drop=(NEEDS[k],)) for k in every]              # an output whose input is missing
    bad += [dict(want=every, drop=(k,)) for k in ("bg", "mask_red", "cover2")]
    bad += [dict(want=[]), dict(want=every, bg_size=(0, 23)), dict(want=every, bg_size=(80, 0))]
    bad += [dict(want=every, M2=m) for m in ([1, 2, 0, 2, 4, 0], [np.nan, 0, 0, 0, 1, 0], [1, 0, 0, 0, 1, np.inf])]
    for kw in bad:
        rc, _, outs = raw_call(gpu_state, c, c["M1"], kw.pop("M2", M2), **kw)
        assert rc == -1, kw
        for k, t in outs.items():
            assert bool((t == 0xA5).all()), (kw, k)                         # nothing ran
    lib, h = gpu_state.lib, gpu_state.handle
    m = (C.c_float * 6)(1, 0, 0, 0, 1, 0)
    one = C.c_void_p(256)                                                   # (never dereferenced: the sizes are refused)
    assert lib.ArapFlow_Background(None, 8, 8, one, 8, 8, m, m, *[one] * 14) == -1
    assert lib.ArapFlow_Background(h, 0, 8, one, 8, 8, m, m, *[one] * 14) == -1
    assert lib.ArapFlow_Background(h, 8, 0, one, 8, 8, m, m, *[one] * 14) == -1
    assert lib.ArapFlow_Background(h, 1 << 16, 1 << 15, one, 8, 8, m, m, *[one] * 14) == -1      # W * H = 2^31
    # through the Python wrapper a refused call is a ValueError
    with pytest.raises(ValueError):
        opt.background(gpu_state, c["bg"], c["M1"], M2, c["rgb1"], c["mask_red"], c["rgb2"], c["cover2"], c["flow"],
                       want=["occ_full"])


def test_inputs_unchanged_and_repeatable(gpu_state, cases):
    c = cases["130x70"]
    M2 = bg_ref.compose(c["M1"], bg_ref.similarity(3.0, 1.02, (2.5, -1.25), centre(c)))
    rc, dev, a = raw_call(gpu_state, c, c["M1"], M2, list(opt.BG_OUTPUTS))
    assert rc == 0
    for k in INPUTS + ("bg",):
        assert np.array_equal(dev[k].cpu().numpy(), c[k]), k
    rc, _, b = raw_call(gpu_state, c, c["M1"], M2, list(opt.BG_OUTPUTS))
    assert rc == 0
    for k in opt.BG_OUTPUTS:
        assert torch.equal(a[k], b[k]), k
    want = twin(c, M2)
    for k in opt.BG_OUTPUTS:
        assert a[k].cpu().numpy().tobytes() == want[k].tobytes(), k
