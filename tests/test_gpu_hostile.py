"""Hostile fields on the GPU (DESIGN.md "Hostile fields"): every route of the warp family -- opt.warp_image /
warp_image_ex, warp_step, warp_layers, warp_layers_step, track_points, warp_diag -- on the families of
tests/hostile_fields.py, bit for bit against the numpy restatements (RGB and mask also against the C oracle).  Float
outputs have their NaNs in the same places and equal bits everywhere else.  Every route also makes each call twice
(identical bytes: no output may depend on the rank an atomicAdd hands a vertex) and follows each hostile call with a
benign one on the same state, which must equal its own restatement (no residue in keys, cell counts, accumulators).
Every family's `exercised` condition and the definedness guard are asserted before the GPU is looked at."""
import functools

import numpy as np
import pytest

import diag_ref as dr
import hostile_fields as hf
import layers_step_ref as sref
import mid_ref
import occ_layers_ref as lref
import occ_ref
import track_ref as tref
from arap_flow_amd import opt

pytestmark = pytest.mark.gpu


def _same(got, ref, keys):
    for k in keys:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, k
        ok = hf.same_float(got[k], ref[k]) if ref[k].dtype == np.float32 else np.array_equal(got[k], ref[k])
        assert ok, k


def _bytes_equal(a, b, keys):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k


def _does_its_job(W, H, name, **kw):
    assert hf.exercised(name, hf.case(W, H, name, "random", **kw)), name
    for mask_name in hf.MASKS:
        assert hf.defined(hf.case(W, H, name, mask_name, **kw)), (name, mask_name)


# ---- the benign call after every hostile one: the input and its restatement, computed once ------------------------------
@functools.lru_cache(maxsize=None)
def _benign(route):
    with np.errstate(all="ignore"):
        if route == "warp":
            rgb, mask, fl = occ_ref.folded_case(70, 50, 3.0)
            return (rgb, mask, fl), occ_ref.warp_ref(rgb, mask, occ_ref.field_from_flow(fl))
        if route == "step":
            rgb, mask, fa, fb = mid_ref.two_state_case(16, 16, 256, "folded")
            a, b = occ_ref.field_from_flow(fa), occ_ref.field_from_flow(fb)
            return (rgb, mask, fa, fb), dict(step=mid_ref.step_ref(mask, a, b), **{
                k: occ_ref.warp_ref(rgb, mask, a)[k] for k in ("warped_rgb", "warped_mask")})
        if route == "layers":
            rgb, masks, flows = lref.layered_case(10, 8, 3, 2)
            return (rgb, masks, flows), lref.layers_ref(rgb, masks, lref.fields_from_flows(flows))
        if route == "layers_step":
            rgb, masks, fa, fb = sref.two_state_layers(10, 8, 3, 3)
            return (rgb, masks, fa, fb), sref.layers_step_ref(masks, lref.fields_from_flows(fa), lref.fields_from_flows(fb))
        if route == "track":
            _, masks, fa, fb = sref.two_state_layers(10, 8, 3, 3)
            flows, pts = np.stack([fa, fb]), tref.case_points(10, 8, 3)
            return (masks, flows, pts), tref.track_ref(masks, np.stack([lref.fields_from_flows(f) for f in flows]), pts)
        if route == "diag":
            mask, fl = dr.masks()["random"], dr.fields()["noise_a"]
            return (mask, fl), dr.diag(mask, dr.flow_pos(fl))
    raise KeyError(route)


def _warp_all(state, rgb, mask, flow):
    return opt.warp_image_ex(state, rgb, mask, flow)


# ---- route 1: the single-layer warp -------------------------------------------------------------------------------------
def _check_warp(state, oracle, c):
    r = _warp_all(state, c["rgb"], c["mask"], c["flow"])
    _same(r, c["ref"], hf.KEYS)
    o_rgb, o_msk = oracle.warp(c["rgb"], c["mask"], c["flow"])
    assert np.array_equal(r["warped_rgb"], o_rgb) and np.array_equal(r["warped_mask"], o_msk)
    _bytes_equal(r, _warp_all(state, c["rgb"], c["mask"], c["flow"]), hf.KEYS)
    w_rgb, w_msk = opt.warp_image(state, c["rgb"], c["mask"], c["flow"])
    assert np.array_equal(w_rgb, o_rgb) and np.array_equal(w_msk, o_msk)
    args, ref = _benign("warp")
    _same(_warp_all(state, *args), ref, hf.KEYS)


@pytest.mark.parametrize("W,H,name", hf.CASES)
def test_warp_image(gpu_state, oracle, W, H, name):
    _does_its_job(W, H, name)
    for mask_name in hf.MASKS:
        _check_warp(gpu_state, oracle, hf.case(W, H, name, mask_name))


@pytest.mark.parametrize("W,H", hf.SCAN_SHAPES)
def test_warp_image_scan_carries(gpu_state, oracle, W, H):
    """N = 4095, 4096, 4097 with nearly every vertex in the first four cells: the start of every later cell is a carry
    of about N, and the vertices on the last cell are found only if it is right"""
    _does_its_job(W, H, "fewpoints", scan=True)
    c = hf.case(W, H, "fewpoints", "random", scan=True)
    assert hf.scan_exercised(c)
    _check_warp(gpu_state, oracle, c)


# ---- route 2: the step between two states ---------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,name", hf.CASES)
def test_warp_step(gpu_state, W, H, name):
    _does_its_job(W, H, name)
    keys = ("warped_rgb", "warped_mask", "step")
    for mask_name in hf.MASKS:
        rgb = hf.case(W, H, name, mask_name)["rgb"]
        for tag, mask, fa, fb in hf.step_inputs(W, H, name, mask_name):
            with np.errstate(all="ignore"):
                A, B = hf.fields_of(fa), hf.fields_of(fb)
                w = occ_ref.warp_ref(rgb, mask, A)
                ref = dict(step=mid_ref.step_ref(mask, A, B), warped_rgb=w["warped_rgb"], warped_mask=w["warped_mask"])
            r = opt.warp_step(gpu_state, rgb, mask, fa, fb)
            _same(r, ref, keys)
            _bytes_equal(r, opt.warp_step(gpu_state, rgb, mask, fa, fb), keys)
            args, bref = _benign("step")
            _same(opt.warp_step(gpu_state, *args), bref, keys)


# ---- route 3: the layered warp ------------------------------------------------------------------------------------------
def _layers_all(state, rgb, masks, flows):
    return opt.warp_layers(state, rgb, masks, flows, bwd=True, occ_bwd=True, occ=True)


@pytest.mark.parametrize("tag", ["below", "above", "between"])
@pytest.mark.parametrize("W,H,name", hf.CASES)
def test_warp_layers(gpu_state, W, H, name, tag):
    _does_its_job(W, H, name)
    for mask_name in hf.MASKS:
        rgb = hf.case(W, H, name, mask_name)["rgb"]
        masks, flows = {t: (m, f) for t, m, f in hf.layer_inputs(W, H, name, mask_name)}[tag]
        assert len(masks) == (3 if tag == "between" else 2)
        with np.errstate(all="ignore"):
            ref = lref.layers_ref(rgb, masks, hf.fields_of(flows))
        r = _layers_all(gpu_state, rgb, masks, flows)
        _same(r, ref, hf.KEYS)
        _bytes_equal(r, _layers_all(gpu_state, rgb, masks, flows), hf.KEYS)
        args, bref = _benign("layers")
        _same(_layers_all(gpu_state, *args), bref, hf.KEYS)


# ---- route 4: the layered step ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b", "both"])
@pytest.mark.parametrize("W,H,name", hf.CASES)
def test_warp_layers_step(gpu_state, W, H, name, tag):
    _does_its_job(W, H, name)
    keys = ("warped_mask", "step", "occlusion_step")
    for mask_name in hf.MASKS:
        rgb = hf.case(W, H, name, mask_name)["rgb"]
        masks, fa, fb = {t: (m, a, b) for t, m, a, b in hf.layers_step_inputs(W, H, name, mask_name)}[tag]
        with np.errstate(all="ignore"):
            ref = sref.layers_step_ref(masks, hf.fields_of(fa), hf.fields_of(fb))
            ref["warped_rgb"] = lref.layers_ref(rgb, masks, hf.fields_of(fa))["warped_rgb"]
        r = opt.warp_layers_step(gpu_state, rgb, masks, fa, fb)
        _same(r, ref, keys + ("warped_rgb",))
        _bytes_equal(r, opt.warp_layers_step(gpu_state, rgb, masks, fa, fb), keys + ("warped_rgb",))
        args, bref = _benign("layers_step")
        _same(opt.warp_layers_step(gpu_state, *args), bref, keys)


# ---- route 5: point tracks ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,name", hf.CASES)
def test_track_points(gpu_state, W, H, name):
    _does_its_job(W, H, name)
    for mask_name in hf.MASKS:
        masks, flows, pts = hf.track_inputs(W, H, name, mask_name)
        assert len(pts) > W * H and (pts != np.floor(pts)).any() and len(flows) == 2
        with np.errstate(all="ignore"):
            ref = tref.track_ref(masks, hf.fields_of(flows), pts)
        r = opt.track_points(gpu_state, masks, flows, pts)
        _same(r, ref, ("pos", "occ"))
        _bytes_equal(r, opt.track_points(gpu_state, masks, flows, pts), ("pos", "occ"))
        args, bref = _benign("track")
        _same(opt.track_points(gpu_state, *args), bref, ("pos", "occ"))


# ---- route 6: fold diagnostics ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,name", hf.CASES)
def test_warp_diag(gpu_state, W, H, name):
    """none of the families is among diag_ref.fields(); every count, flag and extremum bit for bit"""
    _does_its_job(W, H, name)
    for mask_name in hf.MASKS:
        c = hf.case(W, H, name, mask_name)
        want = dr.diag(c["mask"], dr.flow_pos(c["flow"]))
        r = opt.warp_diag(gpu_state, c["mask"], c["flow"])
        assert dr.stats_bytes(r["stats"]) == dr.stats_bytes(want[0]), (mask_name, r["stats"], want[0])
        assert np.array_equal(r["fold"], want[1])
        again = opt.warp_diag(gpu_state, c["mask"], c["flow"])
        assert dr.stats_bytes(again["stats"]) == dr.stats_bytes(r["stats"]) and again["fold"].tobytes() == r["fold"].tobytes()
        (mask, fl), bref = _benign("diag")
        b = opt.warp_diag(gpu_state, mask, fl)
        assert dr.stats_bytes(b["stats"]) == dr.stats_bytes(bref[0]) and np.array_equal(b["fold"], bref[1])
