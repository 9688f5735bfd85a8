"""GPU: random textures (ArapFlow_Texture, DESIGN.md "Random textures") through the C ABI against the numpy twin
tests/tex_ref.py, byte for byte, and the random-texture twin of a pair (opt.retexture_pair) against the warps it is made of.

Shapes: 70x9 (two block columns and three block rows of the 64x4 blocks, the last one partial each way) and 130x70
(several full blocks).  k_tex_fill has no other size-dependent path, and the layer table takes one route to the kernel
(the state's device buffer) whatever n is."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import tex_ref
from arap_flow_amd import capi, opt, pipeline

pytestmark = pytest.mark.gpu
F = np.float32
SIZES = {"70x9": (70, 9), "130x70": (130, 70)}
KINDS = range(len(tex_ref.KINDS))
SEEDS = (0, 0xffffffff, 0x9e3779b9)
PALETTES = (((250, 10, 30), (20, 200, 90), (5, 5, 120)), ((0, 0, 0), (255, 255, 255), (128, 64, 200)),
            ((90, 160, 33), (91, 20, 240), (255, 0, 17)))


def layer(kind, slot, size):
    """a description with a rotated map whose texture coordinates are negative over part of the frame (slot 0: over all
    of it), cells of `size` pixels (bricks: 2.5 cells wide), the seed and the palette of the slot"""
    rot = (0.4, -1.1, 2.5)[slot]
    co, si = math.cos(rot), math.sin(rot)
    su = size * 2.5 if kind == tex_ref.BRICK else size
    m = (co / su, si / su, (-40.25, -0.5, 1.75)[slot], -si / size, co / size, (-33.0, 0.125, -2.5)[slot])
    p0, p1 = {tex_ref.BRICK: (0.11, 0.45), tex_ref.WAVE: (0.7, float(slot % 2))}.get(kind, (0.0, 0.0))
    f32 = lambda v: float(F(v))
    return pipeline.TexLayer(kind, SEEDS[slot], tuple(f32(v) for v in m), f32(p0), f32(p1), *PALETTES[slot])


def layers_for(kind, n, size=5.0):
    """n layers, the first of `kind`, the others of the kinds after it"""
    return [layer((kind + l) % len(tex_ref.KINDS), l, size + l) for l in range(n)]


@pytest.fixture(scope="module")
def cases():
    """per size: a random frame, three overlapping masks (a pixel may belong to none, one, two or all three) and three
    smooth flows"""
    out = {}
    for name, (W, H) in SIZES.items():
        rng = np.random.default_rng(W)
        ys, xs = np.mgrid[0:H, 0:W]
        ell = lambda cx, cy, rx, ry: np.where(((xs - cx) / rx) ** 2 + ((ys - cy) / ry) ** 2 <= 1, 0, 255).astype(np.uint8)
        masks = np.stack([ell(0.35 * W, 0.5 * H, 0.3 * W, 0.45 * H), ell(0.55 * W, 0.4 * H, 0.25 * W, 0.35 * H),
                          ell(0.7 * W, 0.6 * H, 0.22 * W, 0.38 * H)])
        obj = masks == 0
        assert (obj.sum(0) == 0).any() and (obj.sum(0) == 3).any() and (obj[0] & ~obj[1] & ~obj[2]).any()
        flows = np.stack([np.stack([1.5 + 0.02 * ys + l, -1.0 + 0.01 * xs - l], -1) for l in range(3)]).astype(F)
        c = dict(W=W, H=H, rgb=rng.integers(0, 256, (H, W, 3)).astype(np.uint8), masks=masks, flows=flows)
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        out[name] = c
    return out


def same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    assert got.tobytes() == want.tobytes(), "%d bytes differ" % int((got != want).sum())


@pytest.mark.parametrize("kind", KINDS, ids=tex_ref.KINDS)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("size", list(SIZES))
def test_texture_equals_twin(gpu_state, cases, size, n, kind):
    c = cases[size]
    layers = layers_for(kind, n)
    got = opt.texture(gpu_state, c["rgb"], c["masks"][:n], layers)
    want = tex_ref.texture(c["rgb"], c["masks"][:n], layers)
    same(got, want)
    assert len(np.unique(got[c["masks"][n - 1] == 0], axis=0)) >= 2         # (the top layer shows a pattern)


@pytest.mark.parametrize("size", list(SIZES))
def test_null_masks_fill_every_pixel(gpu_state, cases, size):
    c = cases[size]
    for kind in KINDS:
        layers = layers_for(kind, 2)                                        # (layer 1 is never shown)
        got = opt.texture(gpu_state, c["rgb"], None, layers)
        same(got, tex_ref.colour(layers[0], c["W"], c["H"]))
        same(got, tex_ref.texture(c["rgb"], None, layers))


def test_pixels_outside_every_layer_keep_the_input(gpu_state, cases):
    c = cases["130x70"]
    got = opt.texture(gpu_state, c["rgb"], c["masks"], layers_for(2, 3))
    none = (c["masks"] != 0).all(0)
    assert none.any() and np.array_equal(got[none], c["rgb"][none])
    assert not np.array_equal(got[~none], c["rgb"][~none])


def test_a_layer_does_not_depend_on_the_others(gpu_state, cases):
    """changing layer 2's seed leaves layer 1's pixels (and layer 0's) as they were, and changes layer 2's own"""
    c = cases["130x70"]
    a = layers_for(2, 3)
    b = a[:2] + [a[2]._replace(seed=12345)]
    ga, gb = opt.texture(gpu_state, c["rgb"], c["masks"], a), opt.texture(gpu_state, c["rgb"], c["masks"], b)
    own = tex_ref.owner(c["masks"])
    assert np.array_equal(ga[own != 2], gb[own != 2]) and (own == 1).any()
    assert not np.array_equal(ga[own == 2], gb[own == 2])


def test_two_runs_give_identical_bytes(gpu_state, cases):
    c = cases["70x9"]
    layers = layers_for(3, 3)
    same(opt.texture(gpu_state, c["rgb"], c["masks"], layers), opt.texture(gpu_state, c["rgb"], c["masks"], layers))


def test_bad_arguments_return_minus_one_and_write_nothing(gpu_state, cases):
    c = cases["70x9"]
    W, H, n = c["W"], c["H"], 3
    lib, st = gpu_state.lib, gpu_state.handle
    rgb = torch.from_numpy(np.array(c["rgb"])).cuda()
    masks = torch.from_numpy(np.array(c["masks"])).cuda()
    out = torch.full((H, W, 3), 0xAB, dtype=torch.uint8, device="cuda")
    good = layers_for(0, n)
    table = opt.tex_table(good)
    torch.cuda.synchronize()
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(state=st, w=W, h=H, count=n, r=p(rgb), m=p(masks), t=table, o=p(out)):
        return lib.ArapFlow_Texture(state, w, h, count, r, m, t, o)

    def bad_layer(**change):
        return opt.tex_table(good[:1] + [good[1]._replace(**change)] + good[2:])
    nan, inf = float("nan"), float("inf")
    m_nan, m_inf = list(good[1].m), list(good[1].m)
    m_nan[4], m_inf[2] = nan, -inf
    bad = dict(null_state=call(state=None), null_rgb=call(r=None), null_layers=call(t=None), null_out=call(o=None),
               n_zero=call(count=0), n_256=call(count=256), w_zero=call(w=0), h_zero=call(h=0),
               too_large=call(w=65536, h=32768), too_large_2=call(w=1 << 31, h=1),
               kind=call(t=bad_layer(kind=len(tex_ref.KINDS))), kind_max=call(t=bad_layer(kind=0xffffffff)),
               map_nan=call(t=bad_layer(m=m_nan)), map_inf=call(t=bad_layer(m=m_inf)), p0_nan=call(t=bad_layer(p0=nan)),
               p1_inf=call(t=bad_layer(p1=inf)), out_is_rgb=call(o=p(rgb)), out_is_masks=call(o=p(masks)),
               out_in_rgb=call(o=C.c_void_p(rgb.data_ptr() + 3 * W * H - 1)),
               out_before_masks=call(o=C.c_void_p(masks.data_ptr() - 3 * W * H + 1)))
    torch.cuda.synchronize()
    assert bad == {k: -1 for k in bad}
    assert bool((out == 0xAB).all()) and np.array_equal(rgb.cpu().numpy(), c["rgb"])
    assert np.array_equal(masks.cpu().numpy(), c["masks"])
    assert call() == 0                                                      # the same call with nothing wrong
    torch.cuda.synchronize()
    same(out.cpu().numpy(), tex_ref.texture(c["rgb"], c["masks"], good))
    with pytest.raises(ValueError):
        opt.texture(gpu_state, c["rgb"], c["masks"], [good[0]._replace(p0=nan)] + good[1:])


@pytest.mark.parametrize("size", list(SIZES))
def test_retexture_pair_is_texture_then_the_layered_warp(gpu_state, cases, size):
    c = cases[size]
    layers = layers_for(1, 3)
    rgb1, rgb2, mask2 = opt.retexture_pair(gpu_state, c["rgb"], c["masks"], c["flows"], layers)
    same(rgb1, tex_ref.texture(c["rgb"], c["masks"], layers))
    org = opt.warp_layers(gpu_state, c["rgb"], c["masks"], c["flows"], occ=False)
    same(mask2, org["warped_mask"])                                         # same flows, same geometry
    assert (mask2 != 0).any()
    same(rgb2, opt.warp_layers(gpu_state, rgb1, c["masks"], c["flows"], occ=False)["warped_rgb"])
    assert not np.array_equal(rgb2, org["warped_rgb"])


def test_retexture_pair_of_one_layer_is_warp_image(gpu_state, cases):
    c = cases["130x70"]
    layers = layers_for(4, 1)
    rgb1, rgb2, mask2 = opt.retexture_pair(gpu_state, c["rgb"], c["masks"][:1], c["flows"][:1], layers)
    wrgb, wmask = opt.warp_image(gpu_state, rgb1, c["masks"][0], c["flows"][0])
    same(rgb2, wrgb)
    same(mask2, wmask)
