"""GPU: the moving background over a sequence of frames (ArapFlow_BackgroundSeq, DESIGN.md "Moving background over
in-between frames") through the C ABI against the numpy twin tests/bg_seq_ref.py, fed with the library's own point maps.

Shapes (bg_seq_ref.SIZES): a 67x9 frame over an 80x23 picture with 4 frames (W no multiple of 64, H no multiple of 4, one
partial block each way; a first, two middle and a last frame) and a 130x70 frame over a 150x90 picture with 10 frames
(several blocks each way; the argument table at its full size).  The kernel has no other size-dependent path.
tests/test_bg_seq_host.py asserts what each link of these cases covers."""
import ctypes as C

import numpy as np
import pytest
import torch

import bg_ref
import bg_seq_ref
from arap_flow_amd import opt

pytestmark = pytest.mark.gpu
F = np.float32
PAD = 12                   # entries of every pointer array handed to the raw call: more than the largest nframes refused


@pytest.fixture(scope="module")
def cases():
    """per size: the seeded sequence, its camera, the library's point maps and the twin's outputs (computed once)"""
    out = {}
    for name in bg_seq_ref.SIZES:
        c = bg_seq_ref.sized_case(name)
        c["Gs"] = [opt.background_maps(c["maps"][f], c["maps"][f + 1])[0] for f in range(c["m"] - 1)]
        c["twin"] = twin(c, c["maps"], c["Gs"])
        out[name] = c
    return out


def twin(c, maps, Gs=None, m=None):
    m = m or len(maps)
    Gs = Gs if Gs is not None else [opt.background_maps(maps[f], maps[f + 1])[0] for f in range(m - 1)]
    with np.errstate(all="ignore"):
        return bg_seq_ref.background_seq(c["bg"], maps[:m], Gs, c["mask_red"], c["covers"][:m], c["rgbs"][:m],
                                         c["flows"][:m - 1], c["occs"][:m - 1])


def run(state, c, maps, want=None, m=None):
    m = m or len(maps)
    return opt.background_seq(state, c["bg"], maps[:m], c["mask_red"], c["covers"][:m], c["rgbs"][:m], c["flows"][:m - 1],
                              c["occs"][:m - 1], want=want)


def assert_same(got, want, only=None):
    """every entry of `want` (or those `only` = {name: flags} selects) bit for bit; every other entry is None"""
    assert set(got) == set(want) == set(opt.BG_SEQ_OUTPUTS)
    for k in want:
        assert len(got[k]) == len(want[k]), k
        for f, (a, b) in enumerate(zip(got[k], want[k])):
            if only is not None and not only.get(k, [False] * len(want[k]))[f]:
                assert a is None, (k, f)
                continue
            assert a.dtype == b.dtype and a.shape == b.shape, (k, f)
            assert a.tobytes() == b.tobytes(), "%s[%d]: %d differ" % (k, f, int((a != b).sum()))


@pytest.mark.parametrize("size", list(bg_seq_ref.SIZES))
def test_sequence_equals_twin(gpu_state, cases, size):
    c = cases[size]
    got = run(gpu_state, c, c["maps"])
    assert_same(got, c["twin"])
    assert len(got["out_rgb"]) == c["m"] and len(got["flow_full"]) == len(got["occ_full"]) == c["m"] - 1
    for f in range(c["m"] - 1):
        bgpix = c["mask_red"] != 0 if f == 0 else c["covers"][f] == 0
        assert np.abs(got["flow_full"][f][bgpix]).max() > 0 and (got["occ_full"][f][bgpix] == 255).any()
        assert (got["occ_full"][f][bgpix] == 0).any()


def test_two_frames_are_the_pair_pass(gpu_state, cases):
    """identity I1: with two frames the call gives ArapFlow_Background's out_rgb1, flow_full, occ_full and out_rgb2"""
    for size in bg_seq_ref.SIZES:
        c = cases[size]
        maps = np.stack([c["maps"][0], c["maps"][-1]])
        got = run(gpu_state, c, maps, m=2)
        pair = opt.background(gpu_state, c["bg"], maps[0], maps[1], c["rgbs"][0], c["mask_red"], c["rgbs"][1], c["covers"][1],
                              c["flows"][0], occ=c["occs"][0])
        assert_same(got, dict(out_rgb=[pair["out_rgb1"], pair["out_rgb2"]], flow_full=[pair["flow_full"]],
                              occ_full=[pair["occ_full"]]))
        # and a still camera is the static background: the object-side maps as they are
        still = run(gpu_state, c, np.stack([maps[0]] * 3), m=3)
        for f in range(2):
            assert still["flow_full"][f].tobytes() == c["flows"][f].tobytes()
            bgpix = c["mask_red"] != 0 if f == 0 else c["covers"][f] == 0
            assert np.array_equal(still["occ_full"][f][bgpix] == 255, (c["covers"][f + 1] != 0)[bgpix])


def test_null_outputs(gpu_state, cases):
    c = cases["67x9"]
    m = c["m"]
    yes, no = [True] * m, [False] * m
    only_mid = [f != 2 for f in range(m)]
    combos = dict(no_rgb=dict(flow_full=yes[:-1], occ_full=yes[:-1]),
                  no_occ=dict(out_rgb=yes, flow_full=yes[:-1]),
                  a_middle_frame_null=dict(out_rgb=only_mid, flow_full=only_mid[:-1], occ_full=only_mid[:-1]),
                  only_the_last_rgb=dict(out_rgb=no[:-1] + [True]),
                  only_the_first_occ=dict(occ_full=[True] + no[:-2]),
                  one_flow_in_the_middle=dict(out_rgb=no, flow_full=[False, True, False], occ_full=no[:-1]))
    for name, want in combos.items():
        assert_same(run(gpu_state, c, c["maps"], want=want), c["twin"], only=want)
    # an input that is not needed may be missing: no rgb at all, no occlusion at all
    got = opt.background_seq(gpu_state, c["bg"], c["maps"], c["mask_red"], c["covers"], None, c["flows"])
    assert_same(got, c["twin"], only=dict(flow_full=yes[:-1]))


def test_samples_outside_the_picture(gpu_state, cases):
    c = cases["67x9"]
    maps = bg_seq_ref.camera(c["maps"][0], c["m"], c["W"], c["H"], deg=0.0, scale=3.0, shift=(0.0, 0.0))
    got = run(gpu_state, c, maps)
    assert_same(got, twin(c, maps))
    bh, bw = c["bg"].shape[:2]
    for f in (1, 2, 3):
        sx, sy = bg_ref.apply_map(maps[f], c["W"], c["H"])
        assert ((sx > bw - 1) | (sy > bh - 1) | (sx < 0) | (sy < 0)).any()
    sx, sy = bg_ref.apply_map(maps[3], c["W"], c["H"])
    assert ((sx > bw - 1) | (sy > bh - 1) | (sx < 0) | (sy < 0)).mean() > 0.5       # most samples of the last frame are clamped
    assert all(np.isfinite(fl).all() for fl in got["flow_full"])


def test_nan_target_counts_as_outside(gpu_state, cases):
    """a camera of subnormal scale is finite and invertible in double, so ArapFlow_BackgroundMaps takes it, but the point
    map to it overflows float: its linear part is infinite, and infinity times the coordinate 0 is a NaN"""
    c = cases["67x9"]
    tiny = np.array([1e-40, 0, 3, 0, 1e-40, 4], F)
    assert tiny[0] > 0
    maps = np.stack([c["maps"][0], c["maps"][0], tiny])
    G = opt.background_maps(maps[1], maps[2])[0]
    assert np.isinf(G[0]) and np.isinf(G[4])
    got = run(gpu_state, c, maps, m=3)
    want = twin(c, maps, m=3)
    bgpix = c["covers"][1] == 0
    nan = np.isnan(want["flow_full"][1]).any(-1)
    assert (nan & bgpix).any() and not (nan & ~bgpix).any()
    assert (got["occ_full"][1][bgpix] == 255).all()                                 # NaN or infinite: outside, hidden
    for k in ("out_rgb", "occ_full"):
        for a, b in zip(got[k], want[k]):
            assert a.tobytes() == b.tobytes(), k
    assert got["flow_full"][0].tobytes() == want["flow_full"][0].tobytes()
    a, b = got["flow_full"][1], want["flow_full"][1]
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(b)], b[~np.isnan(b)])    # (a NaN's sign is free)


# ---- the raw call: device buffers, pointer arrays, prefilled outputs ----------------------------------------------------
def raw_call(state, c, maps=None, nframes=None, want=None, drop=(), dims=None, bg_size=None, handle="state"):
    """ArapFlow_BackgroundSeq on device tensors -> (return code, inputs on the device, outputs prefilled with 0xA5).
    `want`: {name: flags}, default everything; `drop`: names ("bg", "mask_red") or (list name, index) set to NULL."""
    m = c["m"]
    maps = np.ascontiguousarray(c["maps"] if maps is None else maps, F)
    W, H = dims or (c["W"], c["H"])
    dev = lambda a: None if a is None else torch.from_numpy(np.array(a)).cuda()
    d = dict(bg=dev(c["bg"]), mask_red=dev(c["mask_red"]), covers=[dev(a) for a in c["covers"]], rgbs=[dev(a) for a in c["rgbs"]],
             flows=[dev(a) for a in c["flows"]], occs=[dev(a) for a in c["occs"]])
    shape = dict(out_rgb=(c["H"], c["W"], 3), flow_full=(c["H"], c["W"], 8), occ_full=(c["H"], c["W"]))
    count = dict(out_rgb=m, flow_full=m - 1, occ_full=m - 1)
    want = want if want is not None else {k: [True] * count[k] for k in count}
    outs = {k: [torch.full(shape[k], 0xA5, dtype=torch.uint8, device="cuda") if w else None for w in want.get(k, [False] * count[k])]
            for k in count}
    gone = lambda name, f=None: name in drop if f is None else (name, f) in drop
    p = lambda t: None if t is None else t.data_ptr()
    arr = lambda name, ts: (C.c_void_p * PAD)(*([None if gone(name, f) else p(t) for f, t in enumerate(ts)] + [None] * (PAD - len(ts))))
    mp = np.zeros((PAD, 6), F)
    mp[:len(maps)] = maps
    bw, bh = bg_size or (c["bg"].shape[1], c["bg"].shape[0])
    torch.cuda.synchronize()
    rc = state.lib.ArapFlow_BackgroundSeq(
        state.handle if handle == "state" else None, W, H, None if gone("bg") else C.c_void_p(p(d["bg"])), bw, bh,
        m if nframes is None else nframes, mp.ctypes.data_as(C.POINTER(C.c_float)),
        None if gone("mask_red") else C.c_void_p(p(d["mask_red"])), arr("covers", d["covers"]), arr("rgbs", d["rgbs"]),
        arr("flows", d["flows"]), arr("occs", d["occs"]), arr("out_rgb", outs["out_rgb"]), arr("flow_full", outs["flow_full"]),
        arr("occ_full", outs["occ_full"]))
    torch.cuda.synchronize()
    return rc, d, outs


def test_bad_arguments_launch_nothing(gpu_state, cases):
    c = cases["67x9"]
    m = c["m"]
    none = {k: [False] * n for k, n in (("out_rgb", m), ("flow_full", m - 1), ("occ_full", m - 1))}
    sing, nan, inf = [1, 2, 0, 2, 4, 0], [np.nan, 0, 0, 0, 1, 0], [1, 0, 0, 0, 1, np.inf]
    with_map = lambda f, M: np.concatenate([c["maps"][:f], np.asarray([M], F), c["maps"][f + 1:]])
    bad = [dict(handle=None), dict(drop=("bg",)), dict(drop=("mask_red",))]
    bad += [dict(drop=(("covers", f),)) for f in range(1, m)]                       # a cover of a later frame
    bad += [dict(nframes=n) for n in (0, 1, 11, 12)]
    bad += [dict(dims=(0, c["H"])), dict(dims=(c["W"], 0)), dict(bg_size=(0, 23)), dict(bg_size=(80, 0))]
    bad += [dict(dims=(1 << 16, 1 << 15))]                                          # W * H = 2^31
    bad += [dict(drop=(("rgbs", f),)) for f in range(m)]                            # an output whose input is missing
    bad += [dict(drop=(("flows", f),)) for f in range(m - 1)] + [dict(drop=(("occs", f),)) for f in range(m - 1)]
    bad += [dict(want=none)]                                                        # no output at all
    bad += [dict(maps=with_map(f, M)) for f in (0, 2, m - 1) for M in (sing, nan, inf)]    # a pair of maps refused
    for kw in bad:
        rc, _, outs = raw_call(gpu_state, c, **kw)
        assert rc == -1, kw
        for k, ts in outs.items():
            for t in ts:
                assert t is None or bool((t == 0xA5).all()), (kw, k)                # nothing ran
    # what is allowed to be missing: cover 0, and the inputs of outputs not asked for
    rc, _, outs = raw_call(gpu_state, c, drop=(("covers", 0), ("rgbs", 1), ("occs", 2)),
                           want=dict(out_rgb=[True, False, True, True], flow_full=[True] * 3, occ_full=[True, True, False]))
    assert rc == 0
    assert outs["out_rgb"][0].cpu().numpy().tobytes() == c["twin"]["out_rgb"][0].tobytes()
    # through the Python wrapper a refused call is a ValueError
    with pytest.raises(ValueError):
        opt.background_seq(gpu_state, c["bg"], c["maps"], c["mask_red"], c["covers"], c["rgbs"], c["flows"],
                           want=dict(occ_full=[True] * (m - 1)))
    with pytest.raises(ValueError):
        opt.background_seq(gpu_state, c["bg"], with_map(1, sing), c["mask_red"], c["covers"], c["rgbs"], c["flows"])


def test_inputs_unchanged_and_repeatable(gpu_state, cases):
    c = cases["130x70"]
    rc, dev, a = raw_call(gpu_state, c)
    assert rc == 0
    assert np.array_equal(dev["bg"].cpu().numpy(), c["bg"]) and np.array_equal(dev["mask_red"].cpu().numpy(), c["mask_red"])
    for k in ("covers", "rgbs", "flows", "occs"):
        for t, src in zip(dev[k], c[k]):
            assert (t is None and src is None) or np.array_equal(t.cpu().numpy(), src), k
    rc, _, b = raw_call(gpu_state, c)
    assert rc == 0
    for k in opt.BG_SEQ_OUTPUTS:
        for f, (x, y) in enumerate(zip(a[k], b[k])):
            assert torch.equal(x, y), (k, f)
            assert x.cpu().numpy().tobytes() == c["twin"][k][f].tobytes(), (k, f)
