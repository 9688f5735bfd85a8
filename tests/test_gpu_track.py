"""Point tracks on the GPU (DESIGN.md "Point tracks"): opt.track_points byte for byte against the numpy restatement
(tests/track_ref.py), against the layered step at the integer pixels, a closed form, the block edge in P, one and the
largest number of states, and the argument checks.  Every comparison is exact."""
import functools

import numpy as np
import pytest

import layers_step_ref as sref
import occ_layers_ref as lref
import track_ref as tref
from arap_flow_amd import capi, opt
from test_track_host import _rectangles, check_rectangles

pytestmark = pytest.mark.gpu
F = np.float32


def _same(a, b):
    """exact, NaN payloads included"""
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def _case(W, H, n, seed, overlap):
    """masks, the two states as flows, the case's point set and the restatement's answer, computed once"""
    _, masks, fa, fb = sref.two_state_layers(W, H, n, seed, overlap=overlap)
    flows = np.stack([fa, fb])
    pts = tref.case_points(W, H, seed)
    ref = tref.track_ref(masks, np.stack([lref.fields_from_flows(f) for f in flows]), pts)
    return masks, flows, pts, ref


def _check(r, ref):
    assert r["pos"].dtype == np.float32 and r["occ"].dtype == np.uint8
    assert np.array_equal(r["pos"].view(np.uint32), ref["pos"].view(np.uint32))         # raw bytes, NaNs included
    assert np.array_equal(r["occ"], ref["occ"])


@pytest.mark.parametrize("W,H,n,seed,overlap", sref.MULTI + sref.SINGLE)
def test_equals_restatement_and_repeats(gpu_state, W, H, n, seed, overlap):
    masks, flows, pts, ref = _case(W, H, n, seed, overlap)
    assert len(pts) > W * H and np.isnan(pts).any()              # the bins are sized by P, not N
    r = opt.track_points(gpu_state, masks, flows, pts)
    assert r["pos"].shape == (2, len(pts), 2) and r["occ"].shape == (2, len(pts))
    _check(r, ref)
    again = opt.track_points(gpu_state, masks, flows, pts)       # two runs, identical bytes
    assert _same(r["pos"], again["pos"]) and _same(r["occ"], again["occ"])


@pytest.mark.parametrize("P", [1, 255, 256, 257])
def test_block_edge_in_the_number_of_points(gpu_state, P):
    masks, flows, pts, ref = _case(*sref.MULTI[3])
    assert masks.shape[1:] == (50, 70)
    k = 70 * 50 + 60 + np.arange(P)                              # sub-pixel points, the first 15 on the quarter lattice
    r = opt.track_points(gpu_state, masks, flows, pts[k])
    _check(r, dict(pos=ref["pos"][:, k], occ=ref["occ"][:, k]))  # a point's answer does not depend on the others


@pytest.mark.parametrize("T,case", [(1, sref.MULTI[0]), (capi.MAX_SNAPSHOTS + 1, sref.MULTI[3])])
def test_one_state_and_the_most_states(gpu_state, T, case):
    masks, flows, pts, _ = _case(*case)
    states = np.stack([flows[0] * F(s / T) for s in range(1, T + 1)]).astype(F)
    ref = tref.track_ref(masks, np.stack([lref.fields_from_flows(f) for f in states]), pts)
    assert (ref["occ"] == 255).any() and (ref["occ"] == 0).any()
    r = opt.track_points(gpu_state, masks, states, pts)
    assert r["pos"].shape == (T, len(pts), 2)
    _check(r, ref)


@pytest.mark.parametrize("W,H,n,seed,overlap", sref.MULTI[2:5])
def test_integer_pixels_equal_the_layered_step_from_rest(gpu_state, W, H, n, seed, overlap):
    masks, flows, _, _ = _case(W, H, n, seed, overlap)
    q = tref.pixel_points(W, H)
    r = opt.track_points(gpu_state, masks, flows, q)
    for s in range(2):
        step = opt.warp_layers_step(gpu_state, None, masks, np.zeros_like(flows[s]), flows[s])
        covered = step["warped_mask"].ravel() != 0
        assert covered.any() and (~covered).any()
        assert np.array_equal(r["occ"][s], step["occlusion_step"].ravel())
        with np.errstate(invalid="ignore", over="ignore"):
            mine = (r["pos"][s] - q)[covered]                    # step_of: d - (float)q, one operation
        assert _same(mine, step["step"].reshape(-1, 2)[covered])
        assert _same(r["pos"][s][~covered], q[~covered])


def test_upper_rectangle_moves_over_resting_lower_one(gpu_state):
    masks, flows, pts, upper, rest, want = _rectangles()
    check_rectangles(opt.track_points(gpu_state, masks, flows, pts), pts, upper, rest, want)


def test_leaves_later_layered_results_unchanged(gpu_state):
    rgb, lm, fa, fb = sref.two_state_layers(129, 65, 5, 1, overlap=True)

    def others():
        a = opt.warp_layers_step(gpu_state, rgb, lm, fa, fb)
        b = opt.warp_layers(gpu_state, rgb, lm, fa, bwd=True, occ_bwd=True, occ=True)
        return [a[k] for k in sorted(a)] + [b[k] for k in sorted(b)]

    before = others()
    masks, flows, pts, _ = _case(*sref.MULTI[4])
    opt.track_points(gpu_state, masks, flows, pts)
    after = others()
    assert len(before) == len(after) == 9
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()


def test_bad_arguments(gpu_state):
    masks, flows, pts, _ = _case(*sref.MULTI[0])
    cap = capi.MAX_SNAPSHOTS + 1
    with pytest.raises(ValueError):
        opt.track_points(gpu_state, masks[:0], flows[:, :0], pts)                        # n = 0
    with pytest.raises(ValueError):
        opt.track_points(gpu_state, np.repeat(masks, 86, 0), np.repeat(flows, 86, 1), pts)   # n = 258
    with pytest.raises(ValueError):
        opt.track_points(gpu_state, masks, flows[:0], pts)                               # T = 0
    with pytest.raises(ValueError):
        opt.track_points(gpu_state, masks, np.repeat(flows, 5, 0), pts)                  # T = 10
    with pytest.raises(ValueError):
        opt.track_points(gpu_state, masks, flows, pts[:0])                               # P = 0
    with pytest.raises(ValueError):
        opt.track_points(gpu_state, masks, flows, pts.ravel())
    with pytest.raises(ValueError):
        opt.track_points(gpu_state, masks, flows[:, :, :, :-1], pts)
    lib, h = gpu_state.lib, gpu_state.handle
    import torch
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    f = lib.ArapFlow_TrackPoints
    assert f(h, 10, 8, 0, p, 2, p, 4, p, p, p, p) == -1              # n = 0
    assert f(h, 10, 8, 256, p, 2, p, 4, p, p, p, p) == -1            # n = 256
    assert f(h, 10, 8, 2, p, 0, p, 4, p, p, p, p) == -1              # T = 0
    assert f(h, 10, 8, 2, p, cap + 1, p, 4, p, p, p, p) == -1        # T above the cap
    assert f(h, 10, 8, 2, p, 2, p, 0, p, p, p, p) == -1              # P = 0
    assert f(h, 10, 8, 2, p, 2, p, (1 << 24) + 1, p, p, p, p) == -1  # P above the payload's 24 bits
    assert f(h, 10, 8, 2, None, 2, p, 4, p, p, p, p) == -1           # no masks
    assert f(h, 10, 8, 2, p, 2, None, 4, p, p, p, p) == -1           # no flows
    assert f(h, 10, 8, 2, p, 2, p, 4, None, p, p, p) == -1           # no points
    assert f(h, 10, 8, 2, p, 2, p, 4, p, None, None, p) == -1        # both outputs NULL
    assert f(h, 10, 8, 2, p, 2, p, 4, p, p, p, None) == -1           # no scratch
    assert f(None, 10, 8, 2, p, 2, p, 4, p, p, p, p) == -1
    assert f(h, 0, 8, 2, p, 2, p, 4, p, p, p, p) == -1
    assert f(h, 65536, 32768, 1, p, 1, p, 4, p, p, p, p) == -1       # N = 2^31
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0                                       # nothing ran
    size = lib.ArapFlow_TrackPointsScratchBytes
    N, P = 854 * 480, 4096
    assert size(854, 480, 4, P) >= 4 * (4 * (N + 1) + 37 * P) + 32 * P
    assert size(854, 480, 4, P) < size(854, 480, 4, N) and size(854, 480, 0, P) == 0 and size(854, 480, cap + 1, P) == 0


def test_either_output_alone(gpu_state):
    """out_pos or out_occ may be NULL: the other one keeps its bytes"""
    import torch
    masks, flows, pts, ref = _case(*sref.MULTI[0])
    n, H, W = masks.shape
    T, P = 2, len(pts)
    dm, df, dp = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (masks, flows, pts))
    lib = gpu_state.lib
    scratch = torch.empty(int(lib.ArapFlow_TrackPointsScratchBytes(W, H, T, P)), dtype=torch.uint8, device="cuda")
    pos = torch.empty(T, P, 2, dtype=torch.float32, device="cuda")
    occ = torch.empty(T, P, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    args = (gpu_state.handle, W, H, n, dm.data_ptr(), T, df.data_ptr(), P, dp.data_ptr())
    assert lib.ArapFlow_TrackPoints(*args, pos.data_ptr(), None, scratch.data_ptr()) == 0
    assert lib.ArapFlow_TrackPoints(*args, None, occ.data_ptr(), scratch.data_ptr()) == 0
    torch.cuda.synchronize()
    _check(dict(pos=pos.cpu().numpy(), occ=occ.cpu().numpy()), ref)
