"""CPU-only: training batches (DESIGN.md "Training batches") around the kernel.  The numpy twin tests/aug_ref.py against
plain numpy slicing on the five exact cases of the definition, and its properties (used and unused bad taps, the
motion-boundary guard, the eraser rectangles); ArapFlow_AugmentTables (host only) through ctypes: the neutral table, the
inverse, the tone table against numpy's statement, every refusal; the new names.  The twin's flow under a general map against
a closed form that does not share its formula (tests/aug_cases.py)."""
import ctypes as C
import os.path as osp

import numpy as np
import pytest

import aug_cases
import aug_ref

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
F = np.float32
ID = (1, 0, 0, 0, 1, 0)


def sample(T1=ID, T2=ID, gain1=(1, 1, 1), gamma1=1.0, gain2=(1, 1, 1), gamma2=1.0, erase=(), fill=(0, 0, 0)):
    from arap_flow_amd import opt
    return opt.AugSample(T1, T2, gain1, gamma1, gain2, gamma2, erase, fill)


def pair(W, H, seed=0, B=1):
    """frames of random bytes, a flow on the 2^-6 lattice with a few NaN / inf / 1e9 pixels, a random skip"""
    rng = np.random.default_rng(seed)
    rgb1, rgb2 = (rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8) for _ in range(2))
    flow = (rng.integers(-640, 641, (B, H, W, 2)) / 64.0).astype(F)
    for k, v in enumerate((np.nan, np.inf, -np.inf, 1e9)):
        flow[:, (k * 3 + 1) % H, (k * 5 + 2) % W, k % 2] = v
    skip = np.where(rng.random((B, H, W)) < 0.1, rng.integers(1, 256, (B, H, W)), 0).astype(np.uint8)
    return rgb1, rgb2, flow, skip


def planar(a):
    return np.moveaxis(a, -1, 1).astype(F)


def bad_of(flow, skip):
    return (skip != 0) | ~np.isfinite(flow).all(-1)


# ---- the consequences of the definition, against numpy slicing ----------------------------------------------------------
@pytest.mark.parametrize("size", [(70, 9), (1, 1), (5, 4)], ids=lambda s: "%dx%d" % s)
def test_identity_returns_the_inputs(size):
    W, H = size
    rgb1, rgb2, flow, skip = pair(W, H, seed=1, B=2)
    r = aug_ref.augment(rgb1, rgb2, flow, [sample()] * 2, (W, H), skip=skip)
    assert np.array_equal(r["img1"], planar(rgb1)) and np.array_equal(r["img2"], planar(rgb2))
    bad = bad_of(flow, skip)
    assert np.array_equal(r["valid"], np.where(bad, 0, 255))
    assert np.array_equal(r["flow"], np.where(bad[:, None], F(0), planar(flow)))
    assert np.isfinite(r["flow"]).all()


def test_integer_translation_gives_the_cropped_slices():
    W, H, w, h, tx, ty = 70, 9, 48, 5, 13, 3
    rgb1, rgb2, flow, skip = pair(W, H, seed=2)
    T = (1, 0, tx, 0, 1, ty)
    r = aug_ref.augment(rgb1, rgb2, flow, [sample(T, T)], (w, h), skip=skip)
    crop = lambda a: a[:, ty:ty + h, tx:tx + w]
    assert np.array_equal(r["img1"], planar(crop(rgb1))) and np.array_equal(r["img2"], planar(crop(rgb2)))
    bad = crop(bad_of(flow, skip))
    assert np.array_equal(r["valid"], np.where(bad, 0, 255))
    assert np.array_equal(r["flow"], np.where(bad[:, None], F(0), planar(crop(flow))))


def test_mirror_gives_the_mirrored_frames_and_flow():
    W, H = 70, 9
    rgb1, rgb2, flow, skip = pair(W, H, seed=3)
    T = (-1, 0, W - 1, 0, 1, 0)
    r = aug_ref.augment(rgb1, rgb2, flow, [sample(T, T)], (W, H), skip=skip)
    assert np.array_equal(r["img1"], planar(rgb1[:, :, ::-1])) and np.array_equal(r["img2"], planar(rgb2[:, :, ::-1]))
    bad = bad_of(flow, skip)[:, :, ::-1]
    want = planar(flow[:, :, ::-1] * np.asarray([-1, 1], F))
    assert np.array_equal(r["valid"], np.where(bad, 0, 255))
    assert np.array_equal(r["flow"], np.where(bad[:, None], F(0), want))


def test_scale_two_gives_every_second_pixel_and_half_the_flow():
    W, H = 71, 9
    rgb1, rgb2, flow, skip = pair(W, H, seed=4)
    T = (2, 0, 0, 0, 2, 0)
    r = aug_ref.augment(rgb1, rgb2, flow, [sample(T, T)], (36, 5), skip=skip)
    half = lambda a: a[:, ::2, ::2]
    assert np.array_equal(r["img1"], planar(half(rgb1))) and np.array_equal(r["img2"], planar(half(rgb2)))
    bad = half(bad_of(flow, skip))
    assert np.array_equal(r["valid"], np.where(bad, 0, 255))
    assert np.array_equal(r["flow"], np.where(bad[:, None], F(0), planar(half(flow) * F(0.5))))


def test_translated_second_frame_shifts_the_flow():
    W, H = 70, 9
    rgb1, rgb2, flow, skip = pair(W, H, seed=5)
    r = aug_ref.augment(rgb1, rgb2, flow, [sample(ID, (1, 0, 2, 0, 1, 1))], (W - 2, H - 1), skip=skip)
    assert np.array_equal(r["img1"], planar(rgb1[:, :H - 1, :W - 2])) and np.array_equal(r["img2"], planar(rgb2[:, 1:, 2:]))
    bad = bad_of(flow, skip)[:, :H - 1, :W - 2]
    want = planar(flow[:, :H - 1, :W - 2] - np.asarray([2, 1], F))
    assert np.array_equal(r["flow"], np.where(bad[:, None], F(0), want))


# ---- properties of the twin ---------------------------------------------------------------------------------------------
def smooth(W, H):
    ys, xs = np.mgrid[0:H, 0:W]
    return (np.stack([xs + 2 * ys, 3 * ys - xs], -1) / 64.0).astype(F)[None]


def test_an_unused_bad_tap_does_not_invalidate_and_a_used_one_does():
    W, H = 12, 6
    flow = smooth(W, H)
    flow[0, 2, 3, 1] = np.nan
    zeros = np.zeros((1, H, W, 3), np.uint8)
    v = aug_ref.augment(zeros, zeros, flow, [sample()], (W, H), want=("valid",))["valid"][0]
    assert v[2, 3] == 0 and v.sum() == 255 * (W * H - 1)                    # fx = fy = 0: the neighbours never read (3, 2)
    v = aug_ref.augment(zeros, zeros, flow, [sample((1, 0, 0.5, 0, 1, 0))], (W - 1, H), want=("valid",))["valid"][0]
    assert v[2, 2] == 0 and v[2, 3] == 0 and v.sum() == 255 * ((W - 1) * H - 2)      # x = 2 reads (2, 3), x = 3 reads (3, 4)
    v = aug_ref.augment(zeros, zeros, flow, [sample((1, 0, 0.5, 0, 1, 0.25))], (W - 1, H - 1), want=("valid",))["valid"][0]
    assert [(y, x) for y, x in zip(*np.nonzero(v == 0))] == [(1, 2), (1, 3), (2, 2), (2, 3)]
    skip = np.zeros((1, H, W), np.uint8)
    skip[0, 4, 7] = 1
    flow = smooth(W, H)
    v = aug_ref.augment(zeros, zeros, flow, [sample((1, 0, 0, 0, 1, 0.5))], (W, H - 1), skip=skip, want=("valid",))["valid"][0]
    assert [(y, x) for y, x in zip(*np.nonzero(v == 0))] == [(3, 7), (4, 7)]


def test_spread_against_tau_at_a_planted_step():
    W, H = 12, 4
    flow = np.zeros((1, H, W, 2), F)
    flow[0, :, 5:, 0] = 4.0
    zeros = np.zeros((1, H, W, 3), np.uint8)
    s = sample((1, 0, 0.5, 0, 1, 0))
    for tau, ok in ((3.9, False), (4.0, True), (float("inf"), True), (0.0, False)):
        r = aug_ref.augment(zeros, zeros, flow, [s], (W - 1, H), tau=tau, want=("flow", "valid"))
        assert (r["valid"][0][:, 4] == (255 if ok else 0)).all(), tau
        assert (np.delete(r["valid"][0], 4, axis=1) == 255).all()
        # the mix of 0 and 4 belongs to neither surface; where it counts: q1 - x = 0.5 (frame 2 is not shifted), u.x = 2
        assert (r["flow"][0][0][:, 4] == (2.5 if ok else 0.0)).all()


def test_rectangles_overwrite_the_second_image_only_and_are_clipped():
    W, H = 20, 8
    rgb1, rgb2, flow, skip = pair(W, H, seed=6)
    rects = ((-5, -5, 3, 2), (W - 2, H - 1, W + 10, H + 10), (30, 30, 40, 40), (6, 3, 6, 5))     # the last one is empty
    plain = aug_ref.augment(rgb1, rgb2, flow, [sample()], (W, H), skip=skip)
    r = aug_ref.augment(rgb1, rgb2, flow, [sample(erase=rects, fill=(-1.5, 300, 0.25))], (W, H), skip=skip)
    m = np.zeros((H, W), bool)
    m[:2, :3] = True
    m[H - 1:, W - 2:] = True
    want = np.where(m[None], np.asarray([-1.5, 300, 0.25], F)[:, None, None], plain["img2"][0])
    assert np.array_equal(r["img2"][0], want)
    for k in ("img1", "flow", "valid"):
        assert np.array_equal(r[k], plain[k])


# ---- the flow under a general map, against a closed form ----------------------------------------------------------------
def test_flow_of_an_affine_field_is_the_closed_form():
    """u(q) = G q + g on a dyadic lattice, no skip, tau = inf, under transforms()[5] and 20 draws of AUG_DEFAULT: the
    twin's flow equals inv(T2)(T1 x + u(T1 x)) - x, evaluated in float64, within the bound aug_cases.affine_bound derives
    operation by operation, and four misreadings of the definition miss it by more than ten bounds (affine_check).
    Largest error / bound over the 21 cases: 0.570."""
    W, H, w, h = aug_cases.AFFINE_SIZES
    flow = aug_cases.affine_flow(W, H)[None]
    zeros = np.zeros((1, H, W, 3), np.uint8)
    cases = aug_cases.affine_cases()
    assert len(cases) == 21
    worst = 0.0
    for name, T1, T2 in cases:
        r = aug_ref.augment(zeros, zeros, flow, [sample(T1, T2)], (w, h), tau=float("inf"), want=("flow", "valid"))
        worst = max(worst, aug_cases.affine_check(name, r["flow"][0], r["valid"][0] != 0, T1, T2, W, H))
    print("affine flow, twin: largest error / bound %.3f" % worst)


# ---- ArapFlow_AugmentTables: the library against the Python statement ---------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from arap_flow_amd import build, capi
    build.build()
    return capi.load()


def test_neutral_table_is_the_identity(lib):
    from arap_flow_amd import opt
    P2, lut = opt.augment_tables(opt.AUG_NEUTRAL, lib=lib)
    assert P2.tolist() == [1, 0, 0, 0, 1, 0]
    assert np.array_equal(lut, np.broadcast_to(np.arange(256, dtype=F), (2, 3, 256)))
    _, lut = opt.augment_tables(opt.AUG_NEUTRAL, scale=(1 / 64, 0.5, 2), bias=(-1, 0, 3), lib=lib)
    assert np.array_equal(lut[1], np.arange(256, dtype=F) * np.asarray([[1 / 64], [0.5], [2]], F) + np.asarray([[-1], [0], [3]], F))


def test_inverse_is_the_float64_inverse_rounded_once(lib):
    from arap_flow_amd import opt
    rng = np.random.default_rng(7)
    maps = [(2, 1, 4, 0, 0.5, -8), (-1, 0, 69, 0, 1, 0), (0, -4, 3, 0.25, 0, 1)]
    maps += [tuple(rng.normal(0, 2, 6).astype(F).tolist()) for _ in range(50)]
    for T2 in maps:
        P2, _ = opt.augment_tables(sample(T2=T2), lib=lib)
        M = np.eye(3)
        M[:2] = np.asarray(T2, F).astype(np.float64).reshape(2, 3)
        inv = np.linalg.inv(M)[:2].reshape(6)
        # the crafted maps invert exactly; a random one may sit one double rounding away from numpy's LU
        assert np.allclose(P2, inv, rtol=2.0 ** -22, atol=0) and np.array_equal(P2, aug_ref.tables(sample(T2=T2))[0]), T2
    assert opt.augment_tables(sample(T2=maps[0]), lib=lib)[0].tolist() == [0.5, -1, -10, 0, 2, 16]
    assert opt.augment_tables(sample(T2=maps[1]), lib=lib)[0].tolist() == [-1, 0, 69, 0, 1, 0]
    assert opt.augment_tables(sample(T2=maps[2]), lib=lib)[0].tolist() == [0, 4, -4, -0.25, 0, 0.75]


@pytest.mark.parametrize("gamma", [1.0, 0.45, 2.2])
def test_tone_table_within_one_ulp_of_numpy(lib, gamma):
    from arap_flow_amd import opt
    gain1, gain2, scale, bias = (1.0, 0.5, 1.5), (1.25, 1.0, 0.8), (1 / 58.4, 1 / 57.1, 1 / 57.4), (-2.1, -2.0, -1.8)
    s = sample(gain1=gain1, gamma1=gamma, gain2=gain2, gamma2=1 / gamma)
    _, lut = opt.augment_tables(s, scale=scale, bias=bias, lib=lib)
    i = np.arange(256) / 255.0
    for k, (gain, g) in enumerate(((gain1, gamma), (gain2, 1 / gamma))):
        for c in range(3):
            t = np.float64(F(gain[c])) * np.power(i, np.float64(F(g)))
            want = (255.0 * np.clip(t, 0.0, 1.0)) * np.float64(F(scale[c])) + np.float64(F(bias[c]))
            assert (np.abs(lut[k, c].astype(np.float64) - want) <= np.spacing(np.abs(want).astype(F))).all()
        assert (np.diff(lut[k], axis=1) >= 0).all()
    assert lut[0, 2, 255] == F(255.0 * np.float64(F(scale[2])) + np.float64(F(bias[2])))         # gain 1.5 clips at 1


BAD_SAMPLES = [dict(T1=(1, 0, float("nan"), 0, 1, 0)), dict(T1=(float("inf"), 0, 0, 0, 1, 0)), dict(T2=(1, 0, 0, 0, 1, float("nan"))),
               dict(T2=(1, 0, 0, float("-inf"), 1, 0)), dict(T2=(0, 0, 0, 0, 0, 0)), dict(T2=(1, 2, 5, 2, 4, 7)),
               dict(gain1=(1, 0, 1)), dict(gain1=(1, 1, -1)), dict(gain1=(float("inf"), 1, 1)), dict(gain1=(1, float("nan"), 1)),
               dict(gain2=(0, 1, 1)), dict(gain2=(1, 1, float("nan"))), dict(gamma1=0.0), dict(gamma1=-1.0), dict(gamma1=float("inf")),
               dict(gamma1=float("nan")), dict(gamma2=0.0), dict(gamma2=float("nan")), dict(gamma2=float("inf"))]


def test_tables_refusals(lib):
    from arap_flow_amd import opt
    for kw in BAD_SAMPLES:
        with pytest.raises(ValueError):
            opt.augment_tables(sample(**kw), lib=lib)
        with pytest.raises(ValueError):
            aug_ref.tables(sample(**kw))
    opt.augment_tables(sample(T1=(0, 0, 0, 0, 0, 0), T2=(1e-20, 0, 0, 0, 1e-20, 0)), lib=lib)    # det(T1) is not asked; a tiny det is one
    q = opt.aug_sample(sample())
    one, P2, lut = (C.c_float * 3)(1, 1, 1), (C.c_float * 6)(), (C.c_float * 1536)()
    assert lib.ArapFlow_AugmentTables(C.byref(q), one, one, P2, lut) == 0
    assert lib.ArapFlow_AugmentTables(None, one, one, P2, lut) == -1
    assert lib.ArapFlow_AugmentTables(C.byref(q), None, one, P2, lut) == -1
    assert lib.ArapFlow_AugmentTables(C.byref(q), one, None, P2, lut) == -1
    assert lib.ArapFlow_AugmentTables(C.byref(q), one, one, None, lut) == -1
    assert lib.ArapFlow_AugmentTables(C.byref(q), one, one, P2, None) == -1
    with pytest.raises(ValueError):
        opt.aug_sample(sample(erase=[(0, 0, 1, 1)] * 5))


def test_new_entry_points_exported():
    from arap_flow_amd import build, capi, opt
    lib = C.CDLL(build.build())
    for name in ("ArapFlow_AugmentTables", "ArapFlow_AugmentPairs"):
        assert hasattr(lib, name), name
        assert name in [s[0] for s in capi.SYMBOLS]
    assert C.sizeof(capi.AugSample) == 160 and len(opt.AugSample._fields) == 8
    assert (capi.AUG_MAX_BATCH, capi.AUG_MAX_ERASE) == (64, 4)
    header = open(osp.join(ROOT, "include", "arap_opt.h")).read()
    assert "#define ARAPFLOW_AUG_MAX_BATCH 64\n" in header and "#define ARAPFLOW_AUG_MAX_ERASE 4\n" in header
    for name in ("augment_pairs", "augment_tables", "aug_sample"):
        assert callable(getattr(opt, name))
