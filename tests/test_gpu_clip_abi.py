"""GPU: ArapFlow_AugmentClips called the way a C caller does, with the machinery of tests/abi_cases.py and
tests/abi_pool.py by import: every buffer carved out of one guarded pool at the alignment the header allows and no more
(frames, skip and occ at odd addresses, flows, pos and tracks at 4 mod 8), outputs full of 0xA5; all outputs and the
smallest legal set; the call repeated on the dirty pool; a refused call; and, with the state on a side stream, late inputs
behind a delay and three calls in flight whose frame tables differ (tests/test_gpu_abi_buffers.py and
tests/test_gpu_abi_streams.py state the treatment; their functions are called, not restated)."""
import functools

import numpy as np
import pytest
import torch

import abi_cases
import clip_ref
import test_gpu_abi_buffers as buffers
import test_gpu_abi_streams as streams
import test_gpu_clip as t
from abi_cases import Built, Call, Row
from abi_pool import Pool
from arap_flow_amd import capi, opt

pytestmark = pytest.mark.gpu
NAME = "AugmentClips"
# source, B, T, P, crop: a crop no multiple of four wide and a tile plus one pixel each way; one exact tile (the 16-byte
# stores, where the planes are aligned for them); w = 4 and one row from a wide source; P above and below a block
SHAPES = {"70x9-B3-T3-P65-65x17": (70, 9, 3, 3, 65, 65, 17), "70x9-B3-T3-P257-64x16": (70, 9, 3, 3, 257, 64, 16),
          "300x5-B1-T2-P1-4x1": (300, 5, 1, 2, 1, 4, 1)}
side_state = streams.side_state


@functools.lru_cache(maxsize=None)
def augment_clips(shape, variant=0):
    """variant 0: the case; 1: the decoy (other frames, flows, points); 2: the case under other frame descriptions"""
    W, H, B, T, P, w, h = SHAPES[shape]
    links = t.links_of(T, "next") + ((0, T - 1),)
    L = len(links)
    frames, flows, skip, pos, occ = t.make_clip(W, H, B, T, L, P, seed=W + B + (500 if variant == 1 else 0))
    if variant == 1:                                     # (the builder's flows do not depend on the seed)
        flows = flows * np.float32(0.5)
    samples = t.samples_of(W, H, w, h, B, T, first=3 if variant == 2 else 1)
    twin = clip_ref.augment(frames, samples, (w, h), links=links, flows=flows, skip=skip, pos=pos, occ=occ, tables=opt.clip_tables,
                            scale=t.SCALE, bias=t.BIAS, tau=1.0)
    table = (capi.ClipFrame * (B * T))(*[opt.clip_frame(f) for s in samples for f in s])
    link_table = (abi_cases.C.c_int32 * (2 * L))(*[v for l in links for v in l])
    call = Call.from_descriptor(abi_cases.host_state().lib, NAME, (W, H, w, h, B, T, L, P),
                                [(frames, np.uint8), (link_table, None), (flows, np.float32), (skip, np.uint8), (pos, np.float32),
                                 (occ, np.uint8), (table, None), (opt._f3(t.SCALE, "scale"), None), (opt._f3(t.BIAS, "bias"), None), (1.0, None)],
                                [("video", (B, T, 3, h, w), torch.float32), ("flows", (B, L, 2, h, w), torch.float32),
                                 ("valid", (B, L, h, w), torch.uint8), ("tracks", (B, T, P, 2), torch.float32),
                                 ("vis", (B, T, P), torch.uint8)])
    # in2: flows, in4: pos -- float data a C caller may hold at any multiple of four
    return Built(call.with_aligns({"in2": 4, "in4": 4, "tracks": 4, "flows": 4}), twin)


FIRST = next(iter(SHAPES))
ROW = Row(NAME, {s: functools.partial(augment_clips, s) for s in SHAPES}, ("vis",), ("size", {5: capi.CLIP_MAX_FRAMES + 1}),
          lambda: augment_clips(FIRST, 1), third=lambda: augment_clips(FIRST, 2), vec=True)
abi_cases.BY_NAME.setdefault(NAME, ROW)                 # (looked up by the functions called below; the tables of cases are not touched)


def test_the_decoy_differs_on_every_output():
    case, decoy = ROW.build(ROW.first), ROW.decoy()
    assert set(abi_cases.differ(case.twin, decoy.twin)) == set(case.call.outputs()) == set(opt.CLIP_OUTPUTS)
    aligns = {b.name: b.align for b in case.call.bufs()}
    assert aligns == dict(in0=1, in2=4, in3=1, in4=4, in5=1, video=4, flows=4, valid=1, tracks=4, vis=1)


@pytest.mark.parametrize("aligns", ["min", "vec"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_guards_twin_and_repeat(gpu_state, shape, aligns):
    b = ROW.build(shape)
    if aligns == "vec":
        b = Built(b.call.with_aligns({"*": 16}), b.twin)
    else:
        pool = Pool()
        b.call.carve(pool)
        pool.allocate()
        assert pool.ptr("in4") % 8 == 4 and pool.ptr("tracks") % 8 == 4 and pool.ptr("in0") % 2 == 1
    buffers.run(gpu_state, b)
    for only in (("vis",), ("valid",), ("video", "tracks")):
        buffers.run(gpu_state, b, only=set(only))


def test_a_refused_call_touches_nothing(gpu_state):
    buffers.test_a_refused_call_touches_nothing(gpu_state, NAME)


def test_late_inputs(side_state):
    streams.test_late_inputs(side_state, NAME)


def test_three_calls_in_flight(side_state):
    streams.test_two_calls_in_flight(side_state, NAME)
