"""GPU: ArapFlow_FrameScore / opt.frame_score (DESIGN.md "Frame scoring") byte for byte, table and map, against the numpy
twin tests/fscore_ref.py: at the shapes the kernel branches on (no window, one window, one dimension too small, the edges
of its 64 x 32 tiles in pixels, anchors and staged rows, pairs misaligned for its wide loads, more pairs than grid rows,
many blocks), with every combination of planes it has a path for, on crafted frames and planes at every edge of the
definition, with sums beyond 32 bits; the call's own clearing of the table, its determinism and its refusals."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import fscore_ref
from arap_flow_amd import opt, pipeline

pytestmark = pytest.mark.gpu
F = np.float32
ONE = fscore_ref.ONE
FIELD = {k: i for i, k in enumerate(pipeline.FSCORE_FIELDS)}
ROW = {k: i for i, k in enumerate(pipeline.FSCORE_ROWS)}
KEYS = ("occ", "dist", "skip", "obj")
TH = 32                                     # the kernel's strip height: a block owns 64 x 32 pixels and stages 71 x 39


@functools.lru_cache(maxsize=None)
def case(W, H, n, seed=0):
    """random frames whose estimate is exact in places, close in others and far in the rest, with planes on every value
    the definition tests; read-only"""
    rng = np.random.default_rng([W, H, n, seed])
    ref = rng.integers(0, 256, (n, H, W, 3)).astype(np.uint8)
    ref[:, : H // 2] = (ref[:, : H // 2] // 8 + np.linspace(0, 200, W).astype(np.uint8)[None, None, :, None]).astype(np.uint8)     # a smooth part
    amp = rng.choice(np.array([0, 0, 3, 40, 255]), size=(n, H, W, 1))
    est = np.clip(ref.astype(np.int64) + rng.integers(-1, 2, ref.shape) * amp, 0, 255).astype(np.uint8)
    occ = rng.choice(np.array([0, 0, 1, 255], np.uint8), size=(n, H, W))
    dist = rng.choice(np.array([0, 50, 99, 100, 2000, 3599, 3600, 10000, 19599, 19600, 40000, 65535], np.uint16), size=(n, H, W))
    skip = rng.choice(np.array([0, 0, 0, 0, 0, 0, 0, 2, 255], np.uint8), size=(n, H, W))
    obj = rng.choice(np.array([0, 0, 7, 255], np.uint8), size=(n, H, W))
    out = dict(ref=ref, est=est, occ=occ, dist=dist, skip=skip, obj=obj)
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def want(W, H, n, planes):
    c = case(W, H, n)
    return fscore_ref.fscore_ref(c["ref"], c["est"], **{k: c[k] for k in planes})


def same(got, ref, ssim=True):
    assert got["table"].dtype == np.uint64 and got["table"].shape == ref["table"].shape
    assert np.array_equal(got["table"], ref["table"]), (got["table"] != ref["table"]).nonzero()
    if ssim:
        assert got["ssim"].dtype == F and got["ssim"].shape == ref["ssim"].shape
        assert np.array_equal(got["ssim"].view(np.uint32), ref["ssim"].view(np.uint32)), (got["ssim"] != ref["ssim"]).nonzero()


PLANES = [(), ("occ",), ("dist",), ("skip",), ("obj",), KEYS]
SHAPES = [(5, 3, 1), (8, 8, 1), (7, 20, 1), (20, 7, 1), (71, 11, 1), (72, 11, 1), (68, 36, 1), (69, 37, 1),
          (20, TH + 6, 1), (20, TH + 8, 1), (71, 9, 3)]


@pytest.mark.parametrize("planes", PLANES, ids=lambda p: "+".join(p) or "none")
@pytest.mark.parametrize("W,H,n", SHAPES)
def test_table_and_map_equal_the_twin(gpu_state, W, H, n, planes):
    """5x3: no window; 8x8: one; 7x20, 20x7: one dimension too small; 71x11, 72x11: exactly 64 window columns and one more
    (the second tile of 7 and 8 pixels holds the anchors 64..66 and 64..67); 68x36, 69x37: the last anchor is the last pixel
    of the first tile in x and y, then the first of the next; 20x38, 20x40: one row less and one more than the 39 a block
    stages; 71x9x3: W * H * 3 is odd, pairs 1 and 2 start off every 16-byte chunk"""
    c = case(W, H, n)
    ref = want(W, H, n, planes)
    same(opt.frame_score(gpu_state, c["ref"], c["est"], ssim=True, **{k: c[k] for k in planes}), ref)
    same(opt.frame_score(gpu_state, c["ref"], c["est"], **{k: c[k] for k in planes}), ref, ssim=False)     # without the map
    t = ref["table"]
    assert t[:, ROW["all"], FIELD["count"]].min() > 0
    assert (t[:, 0, FIELD["windows"]] + t[:, 8, 1] == max(W - 7, 0) * max(H - 7, 0)).all()
    if planes == KEYS and W * H > 600:
        s = t.sum(axis=0)
        assert (s[:8, FIELD["count"]] > 0).all() and (s[:8, FIELD["windows"]] > 0).all() and (s[8, :2] > 0).all()
        assert s[0, FIELD["ssim_worst"]] > 0 and s[0, FIELD["sse"]] > 0


@pytest.mark.parametrize("planes", [PLANES[0], PLANES[-1]], ids=["none", "all"])
@pytest.mark.parametrize("W,H,n", [(854, 480, 2), (9, 8, 65540)])
def test_many_blocks_and_many_pairs(gpu_state, W, H, n, planes):
    """854x480x2: 210 blocks a pair meet in the table's atomics; 9x8x65540: more pairs than grid rows, two windows each"""
    c = case(W, H, n)
    same(opt.frame_score(gpu_state, c["ref"], c["est"], ssim=True, **{k: c[k] for k in planes}), want(W, H, n, planes))


def test_a_single_pair_without_the_leading_axis(gpu_state):
    c = case(71, 9, 3)
    got = opt.frame_score(gpu_state, c["ref"][1], c["est"][1], occ=c["occ"][1], ssim=True)
    same(got, fscore_ref.fscore_ref(c["ref"][1], c["est"][1], occ=c["occ"][1]))
    assert got["table"].shape == (1, 9, 7) and got["ssim"].shape == (1, 9, 71)
    assert "ssim" not in opt.frame_score(gpu_state, c["ref"][1], c["est"][1])
    with pytest.raises(ValueError):
        opt.frame_score(gpu_state, c["ref"], c["est"][:2])
    with pytest.raises(ValueError):
        opt.frame_score(gpu_state, c["ref"], c["est"], obj=c["obj"][:2])
    with pytest.raises(ValueError):
        opt.frame_score(gpu_state, c["ref"][..., :2], c["est"][..., :2])


# ---- crafted content -------------------------------------------------------------------------------------------------------
def test_identical_frames_with_every_plane(gpu_state):
    c = case(72, 41, 2)
    planes = {k: c[k] for k in KEYS}
    got = opt.frame_score(gpu_state, c["ref"], c["ref"], ssim=True, **planes)
    same(got, fscore_ref.fscore_ref(c["ref"], c["ref"], **planes))
    t = got["table"]
    assert not t[:, :8, [1, 2, 3, 6]].any() and (t[:, :8, 5] == t[:, :8, 4] * ONE).all() and (t[:, :8, 4] > 0).all()
    assert set(np.unique(got["ssim"])) == {-2.0, 1.0}


def test_constant_frames_0_against_255(gpu_state):
    z = np.zeros((1, 40, 70, 3), np.uint8)
    got = opt.frame_score(gpu_state, z, z + np.uint8(255), ssim=True)
    same(got, fscore_ref.fscore_ref(z, z + np.uint8(255)))
    N, Wn = 40 * 70, 33 * 63
    assert list(got["table"][0, 0]) == [N, N * 195075, N * 765, 255, Wn, Wn * 1048578, ONE - 1048578]


def test_checker_against_its_inverse(gpu_state):
    ck = ((np.indices((37, 69)).sum(axis=0) & 1) * 255).astype(np.uint8)[None, ..., None].repeat(3, axis=-1)
    got = opt.frame_score(gpu_state, ck, 255 - ck, ssim=True)
    ref = fscore_ref.fscore_ref(ck, 255 - ck)
    same(got, ref)
    s = got["ssim"][0, 3:33, 3:65]
    assert (s < -0.99).all() and (s > -1).all() and (got["ssim"] != -2).sum() == s.size
    assert got["table"][0, 0, FIELD["ssim_worst"]] == ONE - int(ref["q"].min()) > 2085000


@pytest.mark.parametrize("x,y,windows", [(30, 20, 64), (0, 0, 1), (68, 36, 1), (66, 2, 3 * 3), (3, 34, 4 * 3), (64, 32, 5 * 5)])
def test_one_pixel_differs(gpu_state, x, y, windows):
    """exactly the windows containing the pixel, 64 away from the border and fewer near it, are below 2^21; (64, 32) is
    the first pixel of the fourth tile, its windows anchored in all four"""
    W, H = 69, 37
    c = case(W, H, 1)
    ref, est = c["ref"].copy(), c["ref"].copy()
    ref[0, y, x], est[0, y, x] = 0, 255
    got = opt.frame_score(gpu_state, ref, est, ssim=True)
    tw = fscore_ref.fscore_ref(ref, est)
    same(got, tw)
    assert (tw["q"] < ONE).sum() == windows and ((got["ssim"] != 1) & (got["ssim"] != -2)).sum() == windows
    below = np.argwhere((got["ssim"][0] < 1) & (got["ssim"][0] != -2)) - 3                       # top-left corners
    assert len(below) == windows and (below[:, 0] <= y).all() and (below[:, 0] + 7 >= y).all() and \
        (below[:, 1] <= x).all() and (below[:, 1] + 7 >= x).all()
    assert list(got["table"][0, 0, :4]) == [W * H, 195075, 765, 255]


def test_planes_on_every_threshold(gpu_state):
    """dist 99 / 100 / 3599 / 3600 / 19599 / 19600 / 65535 and occ, skip, obj 0 / 1 / 255 on every pixel in turn, so on
    anchors and on border pixels, across two tiles: the rows' counts are those of the definition's words"""
    W, H = 70, 13
    c = case(W, H, 1)
    i = np.arange(W * H).reshape(1, H, W)
    dist = np.array([99, 100, 3599, 3600, 19599, 19600, 65535], np.uint16)[i % 7]
    three = np.array([0, 1, 255], np.uint8)
    occ, obj = three[i % 3], three[(i // 3) % 3]
    skip = np.where(i % 5 == 4, three[(i // 5) % 3], 0).astype(np.uint8)
    got = opt.frame_score(gpu_state, c["ref"], c["est"], occ=occ, dist=dist, skip=skip, obj=obj, ssim=True)
    same(got, fscore_ref.fscore_ref(c["ref"], c["est"], occ=occ, dist=dist, skip=skip, obj=obj))
    t = got["table"][0]
    keep = skip == 0
    anchors = np.zeros((1, H, W), bool)
    anchors[:, 3:H - 4, 3:W - 4] = True
    for row, m in (("all", keep), ("noc", keep & (i % 3 == 0)), ("occ", keep & (i % 3 != 0)), ("d0-10", keep & (i % 7 == 0)),
                   ("d10-60", keep & np.isin(i % 7, (1, 2))), ("d60-140", keep & np.isin(i % 7, (3, 4))),
                   ("obj", keep & ((i // 3) % 3 == 0)), ("bg", keep & ((i // 3) % 3 != 0))):
        assert (t[ROW[row], 0], t[ROW[row], 4]) == (m.sum(), (m & anchors).sum()), row
    assert (t[8, 0], t[8, 1]) == ((~keep).sum(), (~keep & anchors).sum()) and t[8, 1] > 0
    assert ((got["ssim"] == -2) == ~(anchors & keep)).all()


@pytest.mark.parametrize("what", ["sse", "ssim_sum"])
def test_sums_beyond_32_bits(gpu_state, what):
    W, H = 854, 480
    N, Wn = W * H, (W - 7) * (H - 7)
    a = np.zeros((H, W, 3), np.uint8)
    if what == "sse":
        t = opt.frame_score(gpu_state, a, a + np.uint8(255))["table"][0]
        assert N * 195075 > 1 << 32 and list(t[0]) == [N, N * 195075, N * 765, 255, Wn, Wn * 1048578, ONE - 1048578]
    else:
        a = case(W, H, 2)["ref"][0]
        t = opt.frame_score(gpu_state, a, a)["table"][0]
        assert Wn * ONE > 1 << 32 and list(t[0]) == [N, 0, 0, 0, Wn, Wn * ONE, 0]
    assert not t[1:].any()


# ---- the call itself: clearing, determinism, refusals ------------------------------------------------------------------------
def raw(state, W, H, n, ref, est, occ, dist, skip, obj, table, ssim):
    """ArapFlow_FrameScore on device pointers: tensors, integers (addresses) or None"""
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr() if isinstance(t, torch.Tensor) else int(t))
    rc = state.lib.ArapFlow_FrameScore(state.handle, W, H, n, *[p(t) for t in (ref, est, occ, dist, skip, obj, table, ssim)])
    torch.cuda.synchronize()
    return rc


def dev(c, keys=("ref", "est") + KEYS):
    return [torch.from_numpy(c[k].view(np.int16) if k == "dist" else np.ascontiguousarray(c[k])).cuda() for k in keys]


def test_two_calls_identical_and_the_table_cleared(gpu_state):
    W, H, n = 71, 9, 3
    bufs = dev(case(W, H, n))
    ref = want(W, H, n, KEYS)
    tables = []
    for fill in (-1, 0x5a5a5a5a5a5a5a5a):
        table = torch.full((n, 9, 7), fill, dtype=torch.int64, device="cuda")
        assert raw(gpu_state, W, H, n, *bufs, table, None) == 0
        tables.append(table.cpu().numpy().view(np.uint64))
    assert tables[0].tobytes() == tables[1].tobytes() == ref["table"].tobytes()


def test_buffers_off_the_wide_loads_alignment(gpu_state):
    """frames and byte planes that start 1 byte, dist 2 and the map 4 bytes into their allocations: the one-pixel path,
    same bytes"""
    W, H, n = 71, 9, 3
    c = case(W, H, n)
    ref = want(W, H, n, KEYS)
    off = lambda a, lead: torch.from_numpy(np.concatenate([np.zeros(lead, a.dtype), a.reshape(-1)])).cuda()
    fr, es = off(c["ref"], 1), off(c["est"], 1)
    occ, dist, skip, obj = off(c["occ"], 1), off(c["dist"].view(np.int16), 1), off(c["skip"], 1), off(c["obj"], 1)
    table = torch.full((n, 9, 7), -1, dtype=torch.int64, device="cuda")
    ssim = torch.full((n * H * W + 1,), 7.0, dtype=torch.float32, device="cuda")
    assert raw(gpu_state, W, H, n, fr.data_ptr() + 1, es.data_ptr() + 1, occ.data_ptr() + 1, dist.data_ptr() + 2, skip.data_ptr() + 1,
               obj.data_ptr() + 1, table, ssim.data_ptr() + 4) == 0
    assert np.array_equal(table.cpu().numpy().view(np.uint64), ref["table"])
    s = ssim.cpu().numpy()
    assert s[0] == 7.0 and np.array_equal(s[1:].view(np.uint32), ref["ssim"].reshape(-1).view(np.uint32))


def test_refusals_leave_everything_untouched(gpu_state):
    W, H, n = 20, 12, 1
    c = case(W, H, n)
    fr, es = dev(c, ("ref", "est"))
    sentinel = lambda: torch.full((n, 9, 7), 0x0123456789abcdef, dtype=torch.int64, device="cuda")
    table = sentinel()
    ssim = torch.full((n, H, W), 7.0, dtype=torch.float32, device="cuda")
    untouched = lambda: (np.array_equal(table.cpu().numpy(), sentinel().cpu().numpy()) and (ssim.cpu().numpy() == 7.0).all() and
                         np.array_equal(fr.cpu().numpy(), c["ref"]) and np.array_equal(es.cpu().numpy(), c["est"]))
    none = (None, None, None, None)
    assert raw(gpu_state, W, H, n, fr, es, *none, es.data_ptr() + 64, None) == -1 and untouched()                  # table inside est
    assert raw(gpu_state, W, H, n, fr, es, *none, es.data_ptr() + W * H * 3 - 1, None) == -1 and untouched()       # on its last byte
    assert raw(gpu_state, W, H, n, fr, es, *none, table, fr.data_ptr() + 16) == -1 and untouched()                 # the map inside ref
    assert raw(gpu_state, W, H, n, fr, es, *none, table, table) == -1 and untouched()                              # the map on the table
    assert raw(gpu_state, W, H, n, fr, es, None, None, None, ssim, table, ssim) == -1 and untouched()              # the map on a plane
    assert raw(gpu_state, 1 << 16, 1 << 15, 1, fr, es, *none, table, None) == -1 and untouched()                   # n * W * H = 2^31
    assert raw(gpu_state, 1 << 15, 1 << 15, 2, fr, es, *none, table, None) == -1 and untouched()
    for bad in ((0, H, n), (W, 0, n), (W, H, 0)):
        assert raw(gpu_state, *bad, fr, es, *none, table, ssim) == -1 and untouched()
    assert raw(gpu_state, W, H, n, None, es, *none, table, ssim) == -1 and untouched()
    assert raw(gpu_state, W, H, n, fr, None, *none, table, ssim) == -1 and untouched()
    assert raw(gpu_state, W, H, n, fr, es, *none, None, ssim) == -1 and untouched()
    assert raw(gpu_state, W, H, n, fr, es, *none, table, ssim) == 0                             # and the same buffers are fine
    ref = want(W, H, n, ())
    assert np.array_equal(table.cpu().numpy().view(np.uint64), ref["table"])
    assert np.array_equal(ssim.cpu().numpy().view(np.uint32), ref["ssim"].view(np.uint32))


def test_kernel_timing_sees_one_launch_per_call(gpu_state):
    c = case(20, 12, 1)
    gpu_state.set_kernel_timing(True)
    try:
        opt.frame_score(gpu_state, c["ref"], c["est"])
        opt.frame_score(gpu_state, c["ref"], c["est"], occ=c["occ"], ssim=True)
        ms, launches = gpu_state.kernel_time("k_frame_score")
    finally:
        gpu_state.set_kernel_timing(False)
    assert launches == 2 and ms > 0
