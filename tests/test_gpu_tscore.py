"""GPU: ArapFlow_TrackScore / opt.track_score (DESIGN.md "Track scoring") byte for byte against the numpy twin
tests/tscore_ref.py: at the point counts the kernel branches on (less than a wave, a wave edge, a block edge, a block that
takes one, two and three chunks), at the frame counts from the smallest to the largest, on a crafted set at every edge of the
definition under a dyadic and a non-dyadic scale, with sums beyond 32 bits; the call's own clearing of the table, its
determinism, the additivity of tables, its refusals."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import tscore_ref as R
from arap_flow_amd import opt

pytestmark = pytest.mark.gpu
F = np.float32


@functools.lru_cache(maxsize=None)
def case(nf, P, seed=0):
    c = R.random_case(nf, P, seed)
    for a in c:
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def want(nf, P, scale=(1, 1)):
    return R.track_score_ref(*case(nf, P), scale)


def same(got, ref):
    assert got.dtype == np.uint64 and got.shape == ref.shape
    assert np.array_equal(got, ref), (got != ref).nonzero()


@pytest.mark.parametrize("P", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_wave_and_block_edges(gpu_state, P):
    """a single lane, one lane short of a wave, a full wave, one lane into the next, the same around a block, four blocks"""
    same(opt.track_score(gpu_state, *case(5, P)), want(5, P))
    if P >= 255:
        assert (want(5, P)[1:].sum(axis=0) > 0).all() and (want(5, P)[0, 0, :2] > 0).all()


@pytest.mark.parametrize("nf", [2, 3, 10, 64])
def test_frame_counts(gpu_state, nf):
    """F = 2: one scored frame and no `reappeared` class; F = 64: the whole LDS table"""
    scale = R.TAPVID_854x480
    same(opt.track_score(gpu_state, *case(nf, 300), scale=scale), want(nf, 300, scale))
    assert want(nf, 300, scale)[-1, 0, 0] > 0


@pytest.mark.parametrize("nf,P", [(2, 256 * 256), (3, 256 * 256 + 1), (3, 256 * 256 + 1023), (2, 256 * 1024), (3, 256 * 1024 + 1),
                                  (2, 2048 * 256 + 300)])
def test_large_blocks_and_several_chunks_a_block(gpu_state, nf, P):
    """65536 points: the most for 256-point chunks, 256 blocks; one more: 1024-point chunks, the last block a chunk of one
    point; 66559: its sixteenth wave one lane short; 256 chunks of 1024: the most blocks that take one chunk each; one point
    more: two chunks a block and the hidden-before bits of two chunks over two scored frames; 513 chunks: three a block"""
    same(opt.track_score(gpu_state, *case(nf, P)), want(nf, P))


@pytest.mark.parametrize("scale", [(1, 1), R.TAPVID_854x480], ids=["unit", "tapvid"])
def test_crafted_set(gpu_state, scale):
    """e2 exactly on every threshold and one ulp below, NaN and inf estimates, every gv / ev combination, hidden-then-visible
    ground truth, invalid queries (tests/test_tscore_host.py reads the set against the definition's words)"""
    c = R.crafted_case(scale)
    same(opt.track_score(gpu_state, *c, scale=scale), R.track_score_ref(*c, scale))


def test_sums_beyond_32_bits(gpu_state):
    """1024 points whose estimate is NaN in every frame: every point-frame is capped"""
    P, nf = 1024, 3
    gt_pos, est_pos = np.zeros((nf, P, 2), F), np.full((nf, P, 2), np.nan, F)
    occ = np.zeros((nf, P), np.uint8)
    t = opt.track_score(gpu_state, gt_pos, occ, est_pos, occ)
    assert (P << 24) >= 1 << 32
    row = [P] * 4 + [0] * 10 + [P << 24, 1 << 24]
    ref = np.zeros((nf, 3, 16), np.uint64)
    ref[0, 0, 0] = P
    ref[1:, 0] = ref[1:, 1] = row
    same(t, ref)
    same(t, R.track_score_ref(gt_pos, occ, est_pos, occ))


def raw(state, nf, P, gt_pos, gt_occ, est_pos, est_occ, sx, sy, table):
    """ArapFlow_TrackScore on device pointers: tensors, integers (addresses) or None"""
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr() if isinstance(t, torch.Tensor) else int(t))
    rc = state.lib.ArapFlow_TrackScore(state.handle, nf, P, *[p(t) for t in (gt_pos, gt_occ, est_pos, est_occ)], sx, sy, p(table))
    torch.cuda.synchronize()
    return rc


def dev(c):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in c]


def test_two_calls_identical_and_the_table_cleared(gpu_state):
    nf, P = 10, 1000
    bufs = dev(case(nf, P))
    tables = []
    for fill in (-1, 0x5a5a5a5a5a5a5a5a):
        table = torch.full((nf, 3, 16), fill, dtype=torch.int64, device="cuda")
        assert raw(gpu_state, nf, P, *bufs, 1.0, 1.0, table) == 0
        tables.append(table.cpu().numpy().view(np.uint64))
    assert tables[0].tobytes() == tables[1].tobytes() == want(nf, P).tobytes()


def test_tables_of_two_halves_add_up(gpu_state):
    """the additivity identity on the device: the points split 389 / 611, every field summed but max, which is the maximum"""
    c = case(10, 1000)
    a = opt.track_score(gpu_state, *[x[:, :389] for x in c])
    b = opt.track_score(gpu_state, *[x[:, 389:] for x in c])
    both = a + b
    both[:, :, R.MAX] = np.maximum(a[:, :, R.MAX], b[:, :, R.MAX])
    same(both, opt.track_score(gpu_state, *c))


def test_refusals_leave_the_table_untouched(gpu_state):
    nf, P = 3, 257
    c = case(nf, P)
    gp, go, ep, eo = dev(c)
    sentinel = lambda: torch.full((nf, 3, 16), 0x0123456789abcdef, dtype=torch.int64, device="cuda")
    table = sentinel()
    untouched = lambda: (np.array_equal(table.cpu().numpy(), sentinel().cpu().numpy()) and
                         np.array_equal(ep.cpu().numpy().view(np.uint32), c[2].view(np.uint32)) and
                         np.array_equal(go.cpu().numpy(), c[1]))
    call = lambda *a, **k: raw(gpu_state, *a, **k)
    for k in range(4):                                          # a null buffer
        bufs = [gp, go, ep, eo]
        bufs[k] = None
        assert call(nf, P, *bufs, 1.0, 1.0, table) == -1 and untouched()
    assert call(nf, P, gp, go, ep, eo, 1.0, 1.0, None) == -1 and untouched()
    for bad_p in (0, (1 << 24) + 1):
        assert call(nf, bad_p, gp, go, ep, eo, 1.0, 1.0, table) == -1 and untouched()
    for bad_f in (0, 1, 65):
        assert call(bad_f, P, gp, go, ep, eo, 1.0, 1.0, table) == -1 and untouched()
    for s in (0.0, -1.0, float("nan"), float("inf")):
        assert call(nf, P, gp, go, ep, eo, s, 1.0, table) == -1 and untouched()
        assert call(nf, P, gp, go, ep, eo, 1.0, s, table) == -1 and untouched()
    assert call(nf, P, gp, go, ep, eo, 1.0, 1.0, ep.data_ptr() + 64) == -1 and untouched()                  # the table inside est_pos
    assert call(nf, P, gp, go, ep, eo, 1.0, 1.0, gp.data_ptr() + nf * P * 8 - 8) == -1 and untouched()      # on gt_pos' last bytes
    assert call(nf, P, gp, go, ep, eo, 1.0, 1.0, go.data_ptr() + 8) == -1 and untouched()
    assert call(nf, P, gp, table, ep, eo, 1.0, 1.0, table) == -1 and untouched()                            # gt_occ on the table
    assert call(nf, P, gp, go, ep, eo, 1.0, 1.0, table) == 0                                                # and the same buffers are fine
    assert np.array_equal(table.cpu().numpy().view(np.uint64), want(nf, P))


def test_kernel_timing_sees_the_launch(gpu_state):
    gpu_state.set_kernel_timing(True)
    try:
        opt.track_score(gpu_state, *case(5, 64))
        opt.track_score(gpu_state, *case(5, 65))
        ms, launches = gpu_state.kernel_time("k_track_score")
    finally:
        gpu_state.set_kernel_timing(False)
    assert launches == 2 and ms > 0


def test_python_shape_checks(gpu_state):
    gp, go, ep, eo = case(5, 64)
    with pytest.raises(ValueError):
        opt.track_score(gpu_state, gp, go, ep[:4], eo)
    with pytest.raises(ValueError):
        opt.track_score(gpu_state, gp, go[:, :63], ep, eo)
    with pytest.raises(ValueError):
        opt.track_score(gpu_state, gp, go, ep, eo, scale=(0, 1))
