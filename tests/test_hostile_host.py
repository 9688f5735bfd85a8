"""Hostile fields (DESIGN.md "Hostile fields"), no GPU: on the families of tests/hostile_fields.py every vectorised
restatement of the warp family against its sequential `*_brute` twin, and the single-layer restatement's RGB and mask
against the committed C oracle, the reference's own statement sequence.  Every family's `exercised` condition and the
definedness guard are asserted on each input first."""
import numpy as np
import pytest

import hostile_fields as hf
import layers_step_ref as sref
import mid_ref
import occ_layers_ref as lref
import occ_ref
import track_ref as tref

W0, H0 = hf.SHAPES[0]


def _same(a, b, keys):
    """u8 outputs equal, float outputs bit for bit but for a NaN's sign and payload"""
    for k in keys:
        ok = hf.same_float(a[k], b[k]) if a[k].dtype == np.float32 else np.array_equal(a[k], b[k])
        assert ok, k


def _does_its_job(W, H, name, **kw):
    """asserted before any comparison: the condition of the family on the random mask, the guard on both masks"""
    assert hf.exercised(name, hf.case(W, H, name, "random", **kw)), name
    for mask_name in hf.MASKS:
        assert hf.defined(hf.case(W, H, name, mask_name, **kw)), (name, mask_name)


def test_families_are_deterministic_flows_with_exact_positions():
    a, b = hf.flows(W0, H0, 0), hf.flows(W0, H0, 0)
    fields = hf.families(W0, H0, 0)
    assert tuple(a) == hf.NAMES == tuple(fields)
    g = hf.grid(W0, H0)
    for name in hf.NAMES:
        assert a[name].tobytes() == b[name].tobytes()
        with np.errstate(all="ignore"):
            assert hf.same_float(fields[name], g + a[name])                  # field = (float)x + flow, one addition
    assert (hf.flows(W0, H0, 1)["int"] != a["int"]).any()
    strip = hf.masks(W0, H0, 0)["strip"]
    assert (occ_ref.own_max_tri(strip)[strip == 0] == -1).all() and (strip == 0).sum() == W0
    edges = a["edges"]
    assert np.signbit(edges[edges == 0]).any() and not np.signbit(fields["edges"][fields["edges"] == 0]).any()


@pytest.mark.parametrize("name", hf.NAMES)
def test_restatements_equal_sequential_definitions(name):
    _does_its_job(W0, H0, name)
    for mask_name in hf.MASKS:
        c = hf.case(W0, H0, name, mask_name)
        with np.errstate(all="ignore"):
            _same(c["ref"], occ_ref.warp_brute(c["rgb"], c["mask"], c["field"]), hf.KEYS)
            for tag, mask, fa, fb in hf.step_inputs(W0, H0, name, mask_name):
                A, B = hf.fields_of(fa), hf.fields_of(fb)
                assert hf.same_float(mid_ref.step_ref(mask, A, B), mid_ref.step_brute(mask, A, B)), (mask_name, tag)
            for tag, masks, flows in hf.layer_inputs(W0, H0, name, mask_name):
                fields = hf.fields_of(flows)
                _same(lref.layers_ref(c["rgb"], masks, fields), lref.layers_brute(c["rgb"], masks, fields), hf.KEYS)
            for tag, masks, fa, fb in hf.layers_step_inputs(W0, H0, name, mask_name):
                A, B = hf.fields_of(fa), hf.fields_of(fb)
                _same(sref.layers_step_ref(masks, A, B), sref.layers_step_brute(masks, A, B),
                      ("step", "occlusion_step", "warped_mask"))
            masks, flows, pts = hf.track_inputs(W0, H0, name, mask_name)
            fields = hf.fields_of(flows)
            _same(tref.track_ref(masks, fields, pts), tref.track_brute(masks, fields, pts), ("pos", "occ"))


@pytest.mark.parametrize("W,H,name", hf.CASES)
def test_restatement_warp_equals_oracle(oracle, W, H, name):
    _does_its_job(W, H, name)
    for mask_name in hf.MASKS:
        c = hf.case(W, H, name, mask_name)
        o_rgb, o_msk = oracle.warp_offset(c["rgb"], c["mask"], c["field"])
        assert np.array_equal(c["ref"]["warped_rgb"], o_rgb) and np.array_equal(c["ref"]["warped_mask"], o_msk)
        f_rgb, f_msk = oracle.warp(c["rgb"], c["mask"], c["flow"])                 # the flow form places the same field
        assert np.array_equal(f_rgb, o_rgb) and np.array_equal(f_msk, o_msk)


@pytest.mark.parametrize("W,H", hf.SCAN_SHAPES)
def test_scan_shapes_carry_about_n_into_the_later_cells(oracle, W, H):
    _does_its_job(W, H, "fewpoints", scan=True)
    c = hf.case(W, H, "fewpoints", "random", scan=True)
    assert hf.scan_exercised(c)
    o_rgb, o_msk = oracle.warp_offset(c["rgb"], c["mask"], c["field"])
    assert np.array_equal(c["ref"]["warped_rgb"], o_rgb) and np.array_equal(c["ref"]["warped_mask"], o_msk)
