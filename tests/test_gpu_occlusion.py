"""Backward flow and occlusion maps on the GPU (DESIGN.md "Backward flow and occlusion"): against an identity the
existing rasteriser computes by itself, bit for bit against the numpy restatement (tests/occ_ref.py) through the
three routes that compute them, closed forms, and the outputs leave everything else unchanged."""
import numpy as np
import pytest

import occ_ref
from arap_flow_amd import opt

pytestmark = pytest.mark.gpu

KEYS = ("backward_flow", "occlusion_bwd", "occlusion")


@pytest.mark.parametrize("W,H,amp", [(70, 50, 3.0), (200, 150, 2.0), (256, 256, 6.0)])
def test_backward_flow_matches_interpolated_coordinates(gpu_state, W, H, amp):
    """rgb = (x, y, 0): the rasteriser's colour interpolation is the source point s itself, so trunc(q + B) is the
    warped colour wherever s - q is exact (Sterbenz: q = 0 or q/2 <= s <= 2q), and B = 0 where nothing is drawn"""
    _, mask, fl = occ_ref.folded_case(W, H, amp)
    ys, xs = np.mgrid[0:H, 0:W]
    rgb = np.stack([xs, ys, np.zeros_like(xs)], -1).astype(np.uint8)
    r = opt.warp_image_ex(gpu_state, rgb, mask, fl)
    cov = r["warped_mask"] == 255
    assert (r["backward_flow"][~cov] == 0).all()
    checked = 0
    for d, q in ((0, xs), (1, ys)):
        lo = r["warped_rgb"][..., d].astype(np.float64)            # s in [lo, lo + 1)
        sel = cov & ((q == 0) | ((q / 2 <= lo) & (lo + 1 <= 2 * q)))
        s = q.astype(np.float32) + r["backward_flow"][..., d]
        assert np.array_equal(np.trunc(s[sel]), lo[sel])
        checked += sel.sum()
    assert checked > 1.8 * cov.sum()
    assert np.array_equal(r["occlusion_bwd"] == 255, ~cov & (mask == 0))


@pytest.mark.parametrize("W,H,amp", [(70, 50, 3.0), (129, 65, 8.0), (2, 2, 0.5), (1, 5, 1.0), (854, 480, 2.0)])
def test_warp_ex_equals_restatement(gpu_state, W, H, amp):
    rgb, mask, fl = occ_ref.folded_case(W, H, amp)
    r = opt.warp_image_ex(gpu_state, rgb, mask, fl)
    ref = occ_ref.warp_ref(rgb, mask, occ_ref.field_from_flow(fl))
    for k in ("warped_rgb", "warped_mask") + KEYS:
        assert np.array_equal(r[k], ref[k]), k
    w_rgb, w_msk = opt.warp_image(gpu_state, rgb, mask, fl)                 # the plain warp is unchanged
    assert np.array_equal(w_rgb, r["warped_rgb"]) and np.array_equal(w_msk, r["warped_mask"])
    one = opt.warp_image_ex(gpu_state, rgb, mask, fl, backward=False)      # each output on its own
    assert "backward_flow" not in one and np.array_equal(one["occlusion"], ref["occlusion"])


def _frames(W, H, n, seed):
    """random masks with strong random constraints: folded solved fields"""
    rng = np.random.default_rng(seed)
    out = []
    for b in range(n):
        mask = np.where(rng.random((H, W)) < 0.05, 255, 0).astype(np.uint8)
        k = max(4, W * H // 400)
        xs, ys = rng.integers(0, W, k), rng.integers(0, H, k)
        d = rng.normal(size=(k, 2)) * min(W, H) / 6
        cons = np.stack([xs, ys, xs + d[:, 0].astype(int), ys + d[:, 1].astype(int)], -1).astype(np.int32)
        rgb = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
        out.append((mask, cons, rgb))
    return out


@pytest.mark.parametrize("W,H,batch", [(70, 50, 2), (129, 65, 1), (854, 480, 2)])
def test_frame_solver_routes_equal_restatement(gpu_state, W, H, batch):
    frames = _frames(W, H, batch, W + H)
    fs = opt.FrameSolver(gpu_state, W, H, batch=batch)
    try:
        fs.set_outputs(backward=True, occlusion=True)
        for b, (mask, cons, rgb) in enumerate(frames):
            fs.set_frame(b, mask, cons, rgb=rgb, border_pins=False)
        fs.solve(batch, 2, 2, 20)
        fs.warp(batch)
        got = [fs.results(b) for b in range(batch)]
        for b, (mask, cons, rgb) in enumerate(frames):
            ref = occ_ref.warp_ref(rgb, mask, got[b]["offset"])
            for k in ("warped_rgb", "warped_mask") + KEYS:
                assert np.array_equal(got[b][k], ref[k]), (b, k)
            assert (ref["occlusion"][mask == 0] == 255).any()
        fs.solve_async(batch, 2, 2, 20, warp=True, download=True)
        fs.wait()
        for b in range(batch):
            h = fs.host_results(b)
            for k in ("flow", "warped_rgb", "warped_mask") + KEYS:
                assert np.array_equal(h[k], got[b][k]), (b, k)
    finally:
        fs.close()


def test_translation_closed_form(gpu_state):
    W, H = 120, 80
    mask = np.full((H, W), 255, np.uint8)
    mask[10:60, 20:100] = 0
    t = (31.0, -17.0)
    fl = np.zeros((H, W, 2), np.float32)
    fl[mask == 0] = t
    r = opt.warp_image_ex(gpu_state, None, mask, fl)
    cov = r["warped_mask"] == 255
    assert cov.sum() > 0
    assert (r["backward_flow"][cov] == (-t[0], -t[1])).all() and (r["backward_flow"][~cov] == 0).all()
    ys, xs = np.mgrid[0:H, 0:W]
    out = (xs + t[0] > W - 1) | (ys + t[1] < 0)
    assert np.array_equal(r["occlusion"] == 255, np.where(mask == 0, out, cov))
    assert np.array_equal(r["occlusion_bwd"] == 255, (mask == 0) & ~cov)


def test_mirror_fold_closed_form(gpu_state):
    """the right half of a strip mirrored over its left half at column c: later triangles lie further right in a row,
    so exactly the left-half vertices under the folded half are occluded, and the vacated right half is revealed"""
    W, H = 64, 24
    y0, y1, x0, x1, c = 5, 15, 10, 50, 36
    mask = np.full((H, W), 255, np.uint8)
    mask[y0:y1 + 1, x0:x1 + 1] = 0
    ys, xs = np.mgrid[0:H, 0:W]
    fl = np.zeros((H, W, 2), np.float32)
    right = (mask == 0) & (xs > c)
    fl[..., 0] = np.where(right, 2 * c - 2 * xs, 0).astype(np.float32)
    r = opt.warp_image_ex(gpu_state, None, mask, fl)
    strip = mask == 0
    want = strip & (xs >= 2 * c - x1) & (xs <= c - 1)
    assert np.array_equal(r["occlusion"] == 255, want)
    assert np.array_equal(r["occlusion_bwd"] == 255, strip & (xs > c))
    assert np.array_equal(r["warped_mask"] == 255, strip & (xs <= c))


def test_mirror_fold_closed_form_above_2_24_vertices(gpu_state):
    """test_mirror_fold_closed_form with the strip in the last rows of a 4096 x 4104 grid: N = 2^24 + 32768 and every
    object vertex has an index >= 2^24.  The single-layer query carries a vertex's index at full width; cut to the 24
    bits of the layered query's, its flags would land 4096 rows higher, in rows 1..6.  The whole image is compared."""
    W, H = 4096, 4104
    y0, y1, x0, x1, c = 4097, 4102, 10, 50, 36
    assert W * H == (1 << 24) + 32768 and y0 * W + x0 >= 1 << 24
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    strip = (ys >= y0) & (ys <= y1) & (xs >= x0) & (xs <= x1)
    assert np.flatnonzero(strip).min() >= 1 << 24
    mask = np.where(strip, 0, 255).astype(np.uint8)
    fl = np.zeros((H, W, 2), np.float32)
    fl[..., 0] = np.where(strip & (xs > c), 2 * c - 2 * xs, 0)
    r = opt.warp_image_ex(gpu_state, None, mask, fl)
    want = strip & (xs >= 2 * c - x1) & (xs <= c - 1)
    assert want.sum() == 6 * (c - (2 * c - x1))
    assert np.array_equal(r["occlusion"] == 255, want)
    assert np.array_equal(r["occlusion_bwd"] == 255, strip & (xs > c))
    assert np.array_equal(r["warped_mask"] == 255, strip & (xs <= c))


def test_outputs_change_nothing_else_and_repeat_bit_identical(gpu_state):
    W, H, batch = 160, 96, 2
    frames = _frames(W, H, batch, 7)
    runs = []
    for outputs in (False, True, True):
        fs = opt.FrameSolver(gpu_state, W, H, batch=batch)
        try:
            if outputs:
                fs.set_outputs(backward=True, occlusion=True)
            for b, (mask, cons, rgb) in enumerate(frames):
                fs.set_frame(b, mask, cons, rgb=rgb)
            l0 = fs.stats()["resident_launches"]
            fs.solve(batch, 2, 3, 40)
            fs.warp(batch)
            res = [fs.results(b) for b in range(batch)]
            runs.append((res, fs.stats()["resident_launches"] - l0))
        finally:
            fs.close()
    (off, n0), (on, n1), (again, n2) = runs
    assert n0 == n1 == n2
    for b in range(batch):
        for k in ("flow", "warped_rgb", "warped_mask", "offset", "angle"):
            assert np.array_equal(off[b][k], on[b][k]), k
        assert off[b]["cost"] == on[b]["cost"]
        assert not any(k in off[b] for k in KEYS)
        for k in KEYS:
            assert np.array_equal(on[b][k], again[b][k]), k
