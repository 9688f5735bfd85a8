"""GPU: opt.augment_pairs (ArapFlow_AugmentPairs, DESIGN.md "Training batches") against the numpy twin tests/aug_ref.py,
equal as numbers (-0 may be +0) and free of NaN, at the shapes the kernel branches on: a block is a 64 x 16 tile and a
lane four pixels of a row, stored with 16-byte stores when the crop's width is a multiple of four and the bases are
aligned; B up to 64 and a table that grows under calls in flight; both tap instantiations; inputs off their natural
alignment; side streams: the call returns while its stream is busy, and two calls in flight on two streams share no
table; the flow of an affine field against its closed form (tests/aug_cases.py)."""
import ctypes as C
import itertools
import time

import numpy as np
import pytest
import torch

import aug_cases
import aug_ref
from aug_cases import transforms
from arap_flow_amd import capi, opt

pytestmark = pytest.mark.gpu
F = np.float32
ID = (1, 0, 0, 0, 1, 0)
# one exact tile, a tile plus one pixel each way, w < 4, w % 4 != 0, w % 4 == 0 with one row, three tiles in a row
CROPS = [(1, 1), (3, 2), (4, 1), (64, 16), (65, 17), (70, 9), (130, 3)]
SOURCES = [(1, 1), (2, 2), (70, 9), (300, 5)]
SCALE, BIAS = (1 / 58.395, 1 / 57.12, 1 / 57.375), (-2.1179, -2.0357, -1.8044)


def lib_tables(s, scale, bias):
    return opt.augment_tables(s, scale, bias)


def make_pair(W, H, B, seed):
    """random frames; a flow on the 2^-6 lattice, smooth with one planted step of six pixels, a few NaN / inf / 1e9
    pixels; a random skip"""
    rng = np.random.default_rng(seed)
    rgb1, rgb2 = (rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8) for _ in range(2))
    ys, xs = np.mgrid[0:H, 0:W]
    flow = np.empty((B, H, W, 2), F)
    for b in range(B):
        fx = np.round((0.03 * xs + 0.05 * ys + b) * 64) / 64 + np.where(xs > W // 2, 6.0, 0.0)
        fy = np.round((0.04 * ys - 0.02 * xs - b) * 64) / 64
        flow[b] = np.stack([fx, fy], -1)
    for k, v in enumerate((np.nan, np.inf, -np.inf, 1e9, -1e9)):
        flow[:, (k * 3 + 1) % H, (k * 7 + 2) % W, k % 2] = v
    skip = np.where(rng.random((B, H, W)) < 0.05, rng.integers(1, 256, (B, H, W)), 0).astype(np.uint8)
    return rgb1, rgb2, flow, skip


def same(got, want):
    assert set(got) == set(want)
    for k in want:
        g = got[k].cpu().numpy()
        assert g.shape == want[k].shape and g.dtype == want[k].dtype, k
        assert not np.isnan(g).any(), k
        assert np.array_equal(g, want[k]), (k, int((g != want[k]).sum()))


@pytest.fixture(scope="module")
def pairs():
    return {(W, H, B): make_pair(W, H, B, seed=W + B) for (W, H), B in itertools.product(SOURCES, (1, 3))}


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("source", SOURCES, ids=lambda s: "%dx%d" % s)
def test_augment_equals_twin(gpu_state, pairs, source, B):
    """every crop of CROPS under every transform, a different one per sample"""
    W, H = source
    rgb1, rgb2, flow, skip = pairs[W, H, B]
    dev = [torch.from_numpy(a).cuda() for a in (rgb1, rgb2, flow, skip)]
    for w, h in CROPS:
        ts = transforms(W, H, w, h)
        for first in range(0, len(ts), B):
            samples = [ts[(first + i) % len(ts)] for i in range(B)]
            kw = dict(scale=SCALE, bias=BIAS, tau=1.0)
            want = aug_ref.augment(rgb1, rgb2, flow, samples, (w, h), skip=skip, tables=lib_tables, **kw)
            same(opt.augment_pairs(gpu_state, dev[0], dev[1], dev[2], samples, (w, h), skip=dev[3], **kw), want)


@pytest.mark.parametrize("inputs", ["numpy", "device"])
def test_augment_equals_twin_on_a_side_stream(gpu_state, pairs, inputs):
    """70x9, B = 3, every crop under every transform, with the state on a side stream that is torch's current stream"""
    W, H, B = 70, 9, 3
    host = pairs[W, H, B]
    side = torch.cuda.Stream()
    try:
        gpu_state.set_stream(side)
        with torch.cuda.stream(side):
            ins = [torch.from_numpy(a).cuda() for a in host] if inputs == "device" else host
            for w, h in CROPS:
                ts = transforms(W, H, w, h)
                for first in range(0, len(ts), B):
                    samples = [ts[(first + i) % len(ts)] for i in range(B)]
                    kw = dict(scale=SCALE, bias=BIAS, tau=1.0)
                    want = aug_ref.augment(*host[:3], samples, (w, h), skip=host[3], tables=lib_tables, **kw)
                    got = opt.augment_pairs(gpu_state, ins[0], ins[1], ins[2], samples, (w, h), skip=ins[3], **kw)
                    side.synchronize()
                    same(got, want)
    finally:
        gpu_state.set_stream(None)


# ---- batch sizes up to the limit, and a table that grows while calls are in flight ----------------------------------------
def cycled(W, H, w, h, B, first=0):
    ts = transforms(W, H, w, h)
    return [ts[(first + i) % len(ts)] for i in range(B)]


@pytest.fixture(scope="module")
def big():
    """{B: (inputs, samples, the twin's outputs)} for 70x9 -> 65x9, the seven transforms cycled over the samples"""
    W, H, w, h = 70, 9, 65, 9
    out = {}
    for B in (1, 3, 33, 64):
        ins = make_pair(W, H, B, seed=100 + B)
        samples = cycled(W, H, w, h, B, first=B)
        out[B] = (ins, samples, aug_ref.augment(*ins[:3], samples, (w, h), skip=ins[3], tables=lib_tables, scale=SCALE, bias=BIAS))
    return out


@pytest.mark.parametrize("B", [33, 64])
def test_large_batches(gpu_state, big, B):
    ins, samples, want = big[B]
    same(opt.augment_pairs(gpu_state, *ins[:3], samples, (65, 9), skip=ins[3], scale=SCALE, bias=BIAS), want)


def test_table_grows_under_calls_in_flight(big):
    """a fresh state: B = 1, then 64, then 3, with nothing waited for in between"""
    st = opt.State()
    try:
        dev = {B: [torch.from_numpy(a).cuda() for a in big[B][0]] for B in (1, 64, 3)}
        torch.cuda.synchronize()
        got = {B: opt.augment_pairs(st, *dev[B][:3], big[B][1], (65, 9), skip=dev[B][3], scale=SCALE, bias=BIAS) for B in (1, 64, 3)}
        torch.cuda.synchronize()
        for B in (1, 64, 3):
            same(got[B], big[B][2])
    finally:
        st.close()


# ---- both instantiations of the taps ------------------------------------------------------------------------------------
def test_byte_taps_equal_dword_taps(gpu_state, pairs, monkeypatch):
    """ARAPOPT_AUG_BYTES=1 selects k_augment<false> at any size (a state reads it when it is made)"""
    monkeypatch.setenv("ARAPOPT_AUG_BYTES", "1")
    st = opt.State()
    try:
        for W, H in SOURCES:
            rgb1, rgb2, flow, skip = pairs[W, H, 3]
            samples = transforms(W, H, 65, 17)[4:7]
            kw = dict(skip=skip, scale=SCALE, bias=BIAS)
            want = aug_ref.augment(rgb1, rgb2, flow, samples, (65, 17), tables=lib_tables, **kw)
            a = opt.augment_pairs(st, rgb1, rgb2, flow, samples, (65, 17), **kw)
            b = opt.augment_pairs(gpu_state, rgb1, rgb2, flow, samples, (65, 17), **kw)
            same(a, want)
            same(b, want)
            assert all(a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes() for k in want), (W, H)
    finally:
        st.close()


# ---- inputs off their natural alignment ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(70, 9, 65, 9), (2, 2, 4, 1)], ids=lambda s: "%dx%d-%dx%d" % s)
def test_misaligned_inputs(gpu_state, pairs, shape):
    """each input one element into a larger allocation: the frames and skip at odd addresses (the dword taps straddle
    dwords), the flow at 4 mod 8 (its two-float loads are not 8-byte aligned)"""
    W, H, w, h = shape
    host = pairs[W, H, 3]
    dev = []
    for a in host:
        t = torch.from_numpy(a)
        room = torch.zeros(t.numel() + 1, dtype=t.dtype, device="cuda")
        room[1:] = t.reshape(-1).cuda()
        dev.append(room[1:].view(t.shape))
    assert dev[0].data_ptr() % 2 == 1 and dev[1].data_ptr() % 2 == 1 and dev[3].data_ptr() % 2 == 1 and dev[2].data_ptr() % 8 == 4
    assert all(t.is_contiguous() for t in dev)
    samples = transforms(W, H, w, h)[4:7]
    want = aug_ref.augment(*host[:3], samples, (w, h), skip=host[3], tables=lib_tables, scale=SCALE, bias=BIAS)
    same(opt.augment_pairs(gpu_state, *dev[:3], samples, (w, h), skip=dev[3], scale=SCALE, bias=BIAS), want)
    samples = transforms(W, H, w, h)[:3]
    want = aug_ref.augment(*host[:3], samples, (w, h), skip=host[3], tables=lib_tables)
    same(opt.augment_pairs(gpu_state, *dev[:3], samples, (w, h), skip=dev[3]), want)


# ---- streams ------------------------------------------------------------------------------------------------------------
def host_time_of_a_call(call, sync):
    """seconds, the median of five calls that each begin on an idle stream"""
    ts = []
    for _ in range(5):
        sync()
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    sync()
    return sorted(ts)[2]


@pytest.mark.parametrize("B", [3, 64])
def test_call_returns_while_the_stream_is_busy(gpu_state, big, B):
    """device work of D = min(0.4 s, 300 host times of the call) is queued on the state's stream, then the call is made:
    when it has returned that work has not finished, i.e. the call waited for nothing on its stream -- not for its
    table either, 19 KB of pageable host memory at B = 3 and 394 KB at B = 64, which the runtime stages itself"""
    size = (65, 9)
    host, samples, want = big[B]
    side = torch.cuda.Stream()
    try:
        gpu_state.set_stream(side)
        with torch.cuda.stream(side):
            dev = [torch.from_numpy(a).cuda() for a in host]
            call = lambda: opt.augment_pairs(gpu_state, *dev[:3], samples, size, skip=dev[3], scale=SCALE, bias=BIAS)
            call()                                                         # (first use: the table is allocated)
            t_call = host_time_of_a_call(call, side.synchronize)
            work = aug_cases.BusyWork(side)
            begin, busy = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            begin.record()
            work.queue(min(0.4, 300 * t_call))
            busy.record()
            t0 = time.perf_counter()
            got = call()
            t_busy_call = time.perf_counter() - t0
            returned_first = not busy.query()
            side.synchronize()
            D = begin.elapsed_time(busy) / 1e3
        print("augment_pairs, B = %d, on a busy stream: D %.1f ms, host time of the call idle %.0f us, busy %.0f us, returned first: %s"
              % (B, D * 1e3, t_call * 1e6, t_busy_call * 1e6, returned_first))
        assert D <= 0.5
        assert returned_first
        same(got, want)
    finally:
        gpu_state.set_stream(None)


def test_two_streams_do_not_share_a_table(gpu_state, pairs):
    """call 1 on stream a behind 0.1 s of work, call 2 with other samples on stream b at once: each equals its twin.  The
    state has one table, and the library does not order two streams: here call 2's table and kernel run at once, call 1's
    table is written behind the work on a and read by the kernel that follows it there.  What could go wrong is a copy
    that lands between another stream's copy and its kernel, a window of microseconds that no test can hold open; a
    caller who moves a state between streams closes it (data.AugmentLoader does, tests/test_gpu_data.py)."""
    W, H, B, size = 70, 9, 3, (65, 9)
    host = pairs[W, H, B]
    ts = transforms(W, H, *size)
    S1, S2 = ts[4:7], ts[1:4]
    kw = dict(scale=SCALE, bias=BIAS)
    want1 = aug_ref.augment(*host[:3], S1, size, skip=host[3], tables=lib_tables, **kw)
    want2 = aug_ref.augment(*host[:3], S2, size, skip=host[3], tables=lib_tables, **kw)
    assert all(not np.array_equal(want1[k], want2[k]) for k in want1)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    try:
        dev = [torch.from_numpy(x).cuda() for x in host]
        opt.augment_pairs(gpu_state, *dev[:3], S2, size, skip=dev[3], **kw)      # (first use: the tables are allocated)
        torch.cuda.synchronize()
        work = aug_cases.BusyWork(a)
        busy = torch.cuda.Event()
        with torch.cuda.stream(a):
            work.queue(0.1)
            busy.record()
            gpu_state.set_stream(a)
            got1 = opt.augment_pairs(gpu_state, *dev[:3], S1, size, skip=dev[3], **kw)
        with torch.cuda.stream(b):
            gpu_state.set_stream(b)
            got2 = opt.augment_pairs(gpu_state, *dev[:3], S2, size, skip=dev[3], **kw)
        in_flight = not busy.query()
        a.synchronize()
        b.synchronize()
        assert in_flight                                                       # call 1 had not run when call 2 was made
        same(got2, want2)
        same(got1, want1)
    finally:
        gpu_state.set_stream(None)


# ---- the flow under a general map, against a closed form ----------------------------------------------------------------
def test_flow_of_an_affine_field_is_the_closed_form(gpu_state):
    """as tests/test_aug_host.py states it for the twin, here for the kernel: 21 cases in batches of seven, within the bound
    aug_cases.affine_bound derives.  Largest error / bound on the MI355X: see DESIGN.md "Training batches"."""
    W, H, w, h = aug_cases.AFFINE_SIZES
    cases = aug_cases.affine_cases()
    flow = aug_cases.affine_flow(W, H)
    worst = 0.0
    for first in range(0, len(cases), 7):
        part = cases[first:first + 7]
        samples = [opt.AUG_NEUTRAL._replace(T1=T1, T2=T2) for _, T1, T2 in part]
        got = opt.augment_pairs(gpu_state, None, None, np.stack([flow] * len(part)), samples, (w, h), tau=float("inf"), want=("flow", "valid"))
        out, valid = got["flow"].cpu().numpy(), got["valid"].cpu().numpy() != 0
        for i, (name, T1, T2) in enumerate(part):
            worst = max(worst, aug_cases.affine_check(name, out[i], valid[i], T1, T2, W, H))
    print("affine flow, kernel: largest error / bound %.3f" % worst)


def crafted():
    W, H, w, h = 70, 9, 48, 8
    rgb1, rgb2, flow, skip = make_pair(W, H, 1, seed=11)
    s = transforms(W, H, w, h)[5]
    return rgb1, rgb2, flow, skip, s, (w, h)


def test_crafted_case_is_not_vacuous(gpu_state):
    """70x9 -> 48x8 under a rotation of 0.2 rad and a scale of 1.3: asserted on the twin, at least a quarter of the pixels
    are valid and every reason for invalidity occurs; then the device equals the twin"""
    rgb1, rgb2, flow, skip, s, size = crafted()
    want = aug_ref.augment(rgb1, rgb2, flow, [s], size, skip=skip, tables=lib_tables, reasons=True)
    why = want.pop("reasons")[0]
    valid = want["valid"][0] != 0
    assert valid.mean() >= 0.25, valid.mean()
    for k in ("outside", "bad", "spread", "erased"):
        assert why[k].any(), k
    assert (why["spread"] & ~why["outside"] & ~why["bad"]).any()           # a pixel only the guard rejects
    assert (why["erased"] & valid).any() and (want["img2"][0][:, why["erased"]] == np.asarray(s.fill, F)[:, None]).all()
    same(opt.augment_pairs(gpu_state, rgb1, rgb2, flow, [s], size, skip=skip), want)


def test_every_subset_of_outputs(gpu_state, pairs):
    W, H, B = 70, 9, 3
    rgb1, rgb2, flow, skip = pairs[W, H, B]
    w, h = 65, 9
    samples = transforms(W, H, w, h)[4:7]
    full = aug_ref.augment(rgb1, rgb2, flow, samples, (w, h), skip=skip, tables=lib_tables)
    for n in range(1, 5):
        for want in itertools.combinations(opt.AUG_OUTPUTS, n):
            need_flow = "flow" in want or "valid" in want
            got = opt.augment_pairs(gpu_state, rgb1 if "img1" in want else None, rgb2 if "img2" in want else None,
                                    flow if need_flow else None, samples, (w, h), skip=skip if need_flow else None, want=want)
            same(got, {k: full[k] for k in want})


@pytest.mark.parametrize("size", [(64, 8), (70, 9)], ids=lambda s: "%dx%d" % s)
def test_null_skip_infinite_tau_and_four_rectangles(gpu_state, pairs, size):
    W, H, B = 70, 9, 3
    rgb1, rgb2, flow, skip = pairs[W, H, B]
    samples = transforms(W, H, *size)[3:6]
    for kw in (dict(skip=None), dict(skip=skip, tau=float("inf")), dict(skip=None, tau=0.0), dict(skip=skip, tau=5.5)):
        want = aug_ref.augment(rgb1, rgb2, flow, samples, size, tables=lib_tables, **kw)
        same(opt.augment_pairs(gpu_state, rgb1, rgb2, flow, samples, size, **kw), want)
    with_skip = aug_ref.augment(rgb1, rgb2, flow, samples, size, skip=skip, tau=float("inf"), want=("valid",))["valid"]
    without = aug_ref.augment(rgb1, rgb2, flow, samples, size, tau=float("inf"), want=("valid",))["valid"]
    assert (with_skip != without).any() and (with_skip <= without).all()


def offset_tensors(B, w, h, shift):
    """caller-owned outputs whose bases lie `shift` elements behind an aligned allocation"""
    form = {"img1": ((B, 3, h, w), torch.float32), "img2": ((B, 3, h, w), torch.float32), "flow": ((B, 2, h, w), torch.float32),
            "valid": ((B, h, w), torch.uint8)}
    out = {}
    for k, (shape, dt) in form.items():
        n = int(np.prod(shape))
        out[k] = torch.zeros(n + shift, dtype=dt, device="cuda")[shift:].view(shape)
    return out


@pytest.mark.parametrize("size", [(64, 16), (68, 5)], ids=lambda s: "%dx%d" % s)
def test_misaligned_outputs_and_two_runs(gpu_state, pairs, size):
    """w % 4 == 0, so only the bases decide between the 16-byte stores and the scalar ones"""
    W, H, B = 70, 9, 3
    rgb1, rgb2, flow, skip = pairs[W, H, B]
    samples = transforms(W, H, *size)[4:7]
    want = aug_ref.augment(rgb1, rgb2, flow, samples, size, skip=skip, tables=lib_tables)
    runs = []
    for shift in (0, 1, 0):
        out = offset_tensors(B, *size, shift)
        assert all(t.data_ptr() % 16 == (0 if shift == 0 else t.element_size()) for t in out.values())
        got = opt.augment_pairs(gpu_state, rgb1, rgb2, flow, samples, size, skip=skip, out=out)
        assert all(got[k].data_ptr() == out[k].data_ptr() for k in out)
        same(got, want)
        runs.append({k: t.cpu().numpy().tobytes() for k, t in got.items()})
    assert runs[0] == runs[1] == runs[2]
    only_valid = offset_tensors(B, *size, 0)
    only_valid["valid"] = torch.zeros(B * size[0] * size[1] + 1, dtype=torch.uint8, device="cuda")[1:].view(B, size[1], size[0])
    same(opt.augment_pairs(gpu_state, rgb1, rgb2, flow, samples, size, skip=skip, out=only_valid), want)


def test_bad_arguments_return_minus_one_and_write_nothing(gpu_state, pairs):
    W, H, B = 70, 9, 3
    w, h = 48, 8
    rgb1, rgb2, flow, skip = (torch.from_numpy(a).cuda() for a in pairs[W, H, B])
    good = transforms(W, H, w, h)[4:7]
    out = offset_tensors(B, w, h, 0)
    for t in out.values():
        t.fill_(7)
    lib, st = gpu_state.lib, gpu_state.handle

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == 7).all()) for t in out.values())

    def raw(st=st, dims=(W, H, w, h, B), ins=(rgb1, rgb2, flow, skip), samples=good, scale=(1, 1, 1), bias=(0, 0, 0), tau=1.0,
            outs=tuple(out[k] for k in opt.AUG_OUTPUTS), n_erase=None):
        table = None
        if samples is not None:
            table = (capi.AugSample * len(samples))(*[opt.aug_sample(s) for s in samples])
            if n_erase is not None:
                table[1].n_erase = n_erase
        f3 = lambda v: None if v is None else (C.c_float * 3)(*v)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        return lib.ArapFlow_AugmentPairs(st, *dims, *[ptr(t) for t in ins], table, f3(scale), f3(bias), tau, *[ptr(t) for t in outs])

    assert raw(tau=float("inf")) == 0
    torch.cuda.synchronize()
    assert not any(bool((t == 7).all()) for t in out.values())
    for t in out.values():
        t.fill_(7)
    o = tuple(out[k] for k in opt.AUG_OUTPUTS)
    refused = [dict(st=None), dict(samples=None), dict(scale=None), dict(bias=None), dict(outs=(None,) * 4),
               dict(ins=(None, rgb2, flow, skip)), dict(ins=(rgb1, None, flow, skip)), dict(ins=(rgb1, rgb2, None, skip)),
               dict(ins=(rgb1, rgb2, None, skip), outs=(None, None, None, o[3])), dict(ins=(None, rgb2, flow, skip), outs=(o[0], None, None, None)),
               dict(dims=(0, H, w, h, B)), dict(dims=(W, 0, w, h, B)), dict(dims=(W, H, 0, h, B)), dict(dims=(W, H, w, 0, B)),
               dict(dims=(W, H, w, h, 0)), dict(dims=(1 << 16, 1 << 15, w, h, B)), dict(dims=(W, H, 1 << 16, 1 << 15, 1)),
               dict(dims=(W, H, 1 << 15, 1 << 14, 4)), dict(dims=(W, H, w, h, 65)), dict(tau=float("nan")), dict(tau=-1.0),
               dict(tau=-float("inf")), dict(n_erase=5), dict(n_erase=0xffffffff),
               dict(samples=[good[0], good[1]._replace(T1=(1, 0, float("nan"), 0, 1, 0)), good[2]]),
               dict(samples=[good[0], good[1], good[2]._replace(T2=(1, 2, 0, 2, 4, 0))]),
               dict(samples=[good[0]._replace(gain2=(1, 0, 1)), good[1], good[2]]),
               dict(samples=[good[0], good[1]._replace(gamma1=float("inf")), good[2]]),
               # an output over an input, an output over another output
               dict(outs=(rgb1, o[1], o[2], o[3])), dict(outs=(o[0], rgb2.view(-1)[100:], o[2], o[3])),
               dict(outs=(o[0], o[1], flow, o[3])), dict(outs=(o[0], o[1], o[2], skip.view(-1)[B * H * W - 1:])),
               dict(outs=(o[0], o[1], rgb1, o[3])), dict(outs=(o[0], o[0], o[2], o[3])),
               dict(outs=(o[0], o[1], o[0].view(-1)[B * w * h:], o[3])), dict(outs=(o[0], o[1], o[2], o[1].view(-1)[5:]))]
    for kw in refused:
        assert raw(**kw) == -1, sorted(kw)
    assert untouched()
    # an input that no asked output needs may be null or overlap anything: it is not read
    assert raw(ins=(None, None, flow, None), outs=(None, None, o[2], o[3])) == 0
    assert raw(ins=(o[3], rgb2, None, None), outs=(None, o[1], None, None)) == 0
    torch.cuda.synchronize()
    # the wrapper turns -1 into a ValueError and checks what it can before the call
    for kw in (dict(tau=float("nan")), dict(tau=-0.5), dict(want=()), dict(want=("img1", "depth")), dict(scale=(1, 1)),
               dict(out={"img1": out["img1"][:, :, :, 1:]}), dict(out={"valid": out["flow"]})):
        with pytest.raises(ValueError):
            opt.augment_pairs(gpu_state, rgb1, rgb2, flow, good, (w, h), skip=skip, **kw)
    for size in ((0, h), (w, 0)):
        with pytest.raises(ValueError):
            opt.augment_pairs(gpu_state, rgb1, rgb2, flow, good, size)
    with pytest.raises(ValueError):
        opt.augment_pairs(gpu_state, rgb1, rgb2, flow, good[:2], (w, h))
    with pytest.raises(ValueError):
        opt.augment_pairs(gpu_state, rgb1, rgb2[:, :, :-1], flow, good, (w, h))


def test_kernel_timing_sees_the_launch(gpu_state, pairs):
    W, H, B = 70, 9, 1
    rgb1, rgb2, flow, skip = pairs[W, H, B]
    gpu_state.set_kernel_timing(True)
    try:
        opt.augment_pairs(gpu_state, rgb1, rgb2, flow, [opt.AUG_NEUTRAL], (W, H), skip=skip)
        torch.cuda.synchronize()
        after = gpu_state.kernel_time("k_augment")
    finally:
        gpu_state.set_kernel_timing(False)
    assert after is not None and after[1] == 1 and after[0] > 0
