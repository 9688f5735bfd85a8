"""Backward flow and occlusion maps (DESIGN.md "Backward flow and occlusion"), no GPU: the numpy restatement of
tests/occ_ref.py against the committed C oracle's rasteriser and against the sequential statement of the
definitions, and the library's new entry points."""
import ctypes

import numpy as np
import pytest

import occ_ref


@pytest.mark.parametrize("W,H,amp", [(70, 50, 3.0), (129, 65, 8.0), (64, 4, 1.0), (2, 2, 0.5), (1, 5, 1.0), (854, 480, 2.0)])
def test_restatement_warp_equals_oracle(oracle, W, H, amp):
    rgb, mask, fl = occ_ref.folded_case(W, H, amp)
    r = occ_ref.warp_ref(rgb, mask, occ_ref.field_from_flow(fl))
    o_rgb, o_msk = oracle.warp(rgb, mask, fl)
    assert np.array_equal(r["warped_mask"], o_msk) and np.array_equal(r["warped_rgb"], o_rgb)


def test_restatement_warp_offset_equals_oracle(oracle):
    W, H = 90, 60
    rgb, mask, fl = occ_ref.folded_case(W, H, 4.0, seed=11)
    field = occ_ref.field_from_flow(fl) + np.float32(0.25)
    r = occ_ref.warp_ref(rgb, mask, field)
    o_rgb, o_msk = oracle.warp_offset(rgb, mask, field)
    assert np.array_equal(r["warped_mask"], o_msk) and np.array_equal(r["warped_rgb"], o_rgb)


@pytest.mark.parametrize("W,H,amp,seed", [(6, 5, 1.0, 1), (9, 7, 2.0, 2), (2, 2, 0.5, 3), (1, 5, 1.0, 4), (8, 8, 3.0, 5),
                                          (10, 6, 0.7, 6)])
def test_restatement_equals_sequential_definitions(W, H, amp, seed):
    rgb, mask, fl = occ_ref.folded_case(W, H, amp, seed)
    field = occ_ref.field_from_flow(fl)
    if W * H > 20:                               # out-of-frame and NaN warp positions
        field[1, 1] = (np.float32(-3.5), np.float32(2.0))
        field[2, 3] = (np.float32(np.nan), np.float32(1.0))
    a, b = occ_ref.warp_ref(rgb, mask, field), occ_ref.warp_brute(rgb, mask, field)
    for k in ("warped_rgb", "warped_mask", "backward_flow", "occlusion_bwd", "occlusion"):
        assert np.array_equal(a[k], b[k]), k


def test_restatement_translation_and_fold():
    """closed forms: an integer translation occludes nothing in frame; a mirror fold occludes the overlapped half"""
    W, H = 40, 20
    mask = np.full((H, W), 255, np.uint8)
    mask[4:15, 6:30] = 0
    fl = np.zeros((H, W, 2), np.float32)
    fl[mask == 0] = (13.0, -2.0)
    r = occ_ref.warp_ref(None, mask, occ_ref.field_from_flow(fl))
    cov = r["warped_mask"] == 255
    assert (r["backward_flow"][cov] == (-13.0, 2.0)).all() and (r["backward_flow"][~cov] == 0).all()
    ys, xs = np.mgrid[0:H, 0:W]
    out = (xs + 13 > W - 1) | (ys - 2 < 0)
    want = np.where(mask == 0, out, cov)
    assert np.array_equal(r["occlusion"] == 255, want)


def test_new_entry_points_exported():
    from arap_flow_amd import build, capi
    lib = ctypes.CDLL(build.build())
    for name in ("ArapFlow_SolverSetOutputs", "ArapFlow_SolverGetExtraResults", "ArapFlow_SolverHostExtraResults",
                 "ArapFlow_WarpEx", "ArapFlow_WarpExScratchBytes"):
        assert hasattr(lib, name), name
        assert name in {s[0] for s in capi.SYMBOLS}
    lib.ArapFlow_WarpExScratchBytes.restype = ctypes.c_uint64
    lib.ArapFlow_WarpExScratchBytes.argtypes = [ctypes.c_uint, ctypes.c_uint]
    N = 854 * 480
    assert lib.ArapFlow_WarpExScratchBytes(854, 480) >= 8 * N + 4 * (N + 1) + 4 * N + 16 * N + 112
