"""GPU: opt.augment_clips (ArapFlow_AugmentClips, DESIGN.md "Training clips") against the numpy twin tests/clip_ref.py,
equal as numbers and free of NaN, at the shapes the kernels branch on: a block of k_augment_clip is a 64 x 16 tile of one
frame or one link and a lane four pixels of a row, stored with 16-byte stores when the crop's width is a multiple of four
and the bases are aligned; a block of k_clip_tracks is 256 points of one frame, read and written with 8-byte accesses when
the bases allow; T = 1 (no link possible) to 16, L = 0 to 32 with repeats, the most frames a call takes; every subset of
outputs; both tap instantiations; bases off their natural alignment; a side stream; every refusal."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import clip_ref
from aug_cases import transforms
from arap_flow_amd import capi, opt

pytestmark = pytest.mark.gpu
F = np.float32
# one exact tile, a tile plus one pixel each way, w < 4, w % 4 != 0, w % 4 == 0 with one row, three tiles in a row
CROPS = [(1, 1), (3, 2), (4, 1), (64, 16), (65, 17), (70, 9), (130, 3)]
SOURCES = [(1, 1), (2, 2), (70, 9), (300, 5)]
FRAMES = [1, 2, 3, 16]
LINKS = ["none", "one", "next", "most"]
POINTS = [1, 63, 64, 65, 257]                  # below, at and above a wave; above a block
SCALE, BIAS = (1 / 58.395, 1 / 57.12, 1 / 57.375), (-2.1179, -2.0357, -1.8044)


def lib_tables(f, scale, bias):
    return opt.clip_tables(f, scale, bias)


def links_of(T, kind):
    """none: (); one: (0, T-1); next: (t, t+1); most: 32 links, forward, from-first and backward ones, with repeats"""
    if T == 1 or kind == "none":
        return ()
    if kind == "one":
        return ((0, T - 1),)
    nxt = [(t, t + 1) for t in range(T - 1)]
    if kind == "next":
        return tuple(nxt)
    pool = nxt + [(0, t) for t in range(1, T)] + [(t + 1, t) for t in range(T - 1)] + [(T - 1, 0)]
    return tuple(pool[i % len(pool)] for i in range(capi.CLIP_MAX_LINKS))


def make_clip(W, H, B, T, L, P, seed):
    """random frames; flows on the 2^-6 lattice, smooth with one planted step of six pixels, a few NaN / inf / 1e9 pixels;
    a random skip; points on the 2^-6 lattice around the source, three that no map keeps finite; a random hidden flag"""
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (B, T, H, W, 3)).astype(np.uint8)
    ys, xs = np.mgrid[0:H, 0:W]
    flows = np.empty((B, L, H, W, 2), F)
    for b, l in itertools.product(range(B), range(L)):
        fx = np.round((0.03 * xs + 0.05 * ys + b - l) * 64) / 64 + np.where(xs > W // 2, 6.0, 0.0)
        fy = np.round((0.04 * ys - 0.02 * xs - b + l) * 64) / 64
        flows[b, l] = np.stack([fx, fy], -1)
    for k, v in enumerate((np.nan, np.inf, -np.inf, 1e9, -1e9)):
        flows[:, :, (k * 3 + 1) % H, (k * 7 + 2) % W, k % 2] = v
    skip = np.where(rng.random((B, L, H, W)) < 0.05, rng.integers(1, 256, (B, L, H, W)), 0).astype(np.uint8)
    pos = (np.stack([rng.integers(-128, 64 * (W + 2), (B, T, P)), rng.integers(-128, 64 * (H + 2), (B, T, P))], -1) / 64.0).astype(F)
    for k, v in enumerate(((np.nan, 1.0), (2.0, np.inf), (3e38, -3e38))):
        pos[:, :, (5 * k + 3) % P] = v
    occ = np.where(rng.random((B, T, P)) < 0.2, rng.integers(1, 256, (B, T, P)), 0).astype(np.uint8)
    return frames, flows, skip, pos, occ


def samples_of(W, H, w, h, B, T, first=0):
    """per frame a map, a tone curve, rectangles and a fill of tests/aug_cases.py's transforms, another one per frame"""
    ts = transforms(W, H, w, h)
    out = []
    for b in range(B):
        clip = []
        for t in range(T):
            s = ts[(first + b * T + t) % len(ts)]
            clip.append(opt.ClipFrame(s.T2, s.gain2, s.gamma2, s.erase, s.fill) if (b + t) % 2 else
                        opt.ClipFrame(s.T1, s.gain1, s.gamma1, s.erase, s.fill))
        out.append(clip)
    return out


def same(got, want):
    assert set(got) == set(want)
    for k in want:
        g = got[k].cpu().numpy()
        assert g.shape == want[k].shape and g.dtype == want[k].dtype, k
        assert not np.isnan(g).any(), k
        assert np.array_equal(g, want[k]), (k, int((g != want[k]).sum()))


def run_both(st, c, samples, size, links, **kw):
    frames, flows, skip, pos, occ = c
    L = len(links)
    args = dict(links=links, flows=flows[:, :L] if L else None, skip=skip[:, :L] if L else None, pos=pos, occ=occ)
    args.update(kw)
    want = clip_ref.augment(frames, samples, size, tables=lib_tables, **args)
    same(opt.augment_clips(st, frames, samples, size, **args), want)
    return want


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("source", SOURCES, ids=lambda s: "%dx%d" % s)
def test_clips_equal_twin(gpu_state, source, B):
    """every crop of CROPS under every T of FRAMES and every link table of LINKS; the point counts rotate, so that every
    crop and every T meets every one of them"""
    W, H = source
    for ci, (w, h) in enumerate(CROPS):
        for k, (T, kind) in enumerate(itertools.product(FRAMES, LINKS)):
            links = links_of(T, kind)
            P = POINTS[(k + k // 4 + ci) % 5]
            c = make_clip(W, H, B, T, max(len(links), 1), P, seed=W + B + 10 * T)
            run_both(gpu_state, c, samples_of(W, H, w, h, B, T, first=ci + k), (w, h), links, scale=SCALE, bias=BIAS, tau=1.0)


def test_the_most_frames_a_call_takes(gpu_state):
    """B = 16, T = 16 at a 3 x 2 crop: 256 frames, the table at its largest"""
    W, H, B, T, w, h = 70, 9, 16, 16, 3, 2
    links = links_of(T, "next")
    c = make_clip(W, H, B, T, len(links), 65, seed=9)
    run_both(gpu_state, c, samples_of(W, H, w, h, B, T), (w, h), links, scale=SCALE, bias=BIAS)
    st = opt.State()                               # a fresh state: the table grows from 2 frames to 256 and is used at 6
    try:
        for b, t in ((1, 2), (16, 16), (2, 3)):
            cc = tuple(a[:b, :t] for a in c)
            run_both(st, cc, samples_of(W, H, w, h, b, t), (w, h), links_of(t, "next"))
    finally:
        st.close()


@pytest.fixture(scope="module")
def mid():
    """70x9 -> 65x9 (ragged) and 64x8 (16-byte stores): B = 3, T = 3, two links, 65 points"""
    W, H, B, T, P = 70, 9, 3, 3, 65
    links = ((0, 1), (0, 2))
    return dict(W=W, H=H, B=B, T=T, P=P, links=links, clip=make_clip(W, H, B, T, 2, P, seed=21))


def test_every_subset_of_outputs(gpu_state, mid):
    W, H, B, T = mid["W"], mid["H"], mid["B"], mid["T"]
    frames, flows, skip, pos, occ = mid["clip"]
    w, h = 65, 9
    samples = samples_of(W, H, w, h, B, T, first=4)
    full = clip_ref.augment(frames, samples, (w, h), links=mid["links"], flows=flows, skip=skip, pos=pos, occ=occ, tables=lib_tables)
    for n in range(1, 6):
        for want in itertools.combinations(opt.CLIP_OUTPUTS, n):
            need_links = "flows" in want or "valid" in want
            need_pos = "tracks" in want or "vis" in want
            got = opt.augment_clips(gpu_state, frames if "video" in want else None, samples, (w, h), links=mid["links"] if need_links else (),
                                    flows=flows if need_links else None, skip=skip if need_links else None,
                                    pos=pos if need_pos else None, occ=occ if "vis" in want else None, want=want)
            same(got, {k: full[k] for k in want})


@pytest.mark.parametrize("size", [(64, 8), (70, 9)], ids=lambda s: "%dx%d" % s)
def test_null_skip_tau_and_four_rectangles(gpu_state, mid, size):
    W, H, B, T = mid["W"], mid["H"], mid["B"], mid["T"]
    samples = samples_of(W, H, *size, B, T, first=3)
    assert any(len(f.erase) == 4 for s in samples for f in s)
    frames, flows, skip, pos, occ = mid["clip"]
    for kw in (dict(skip=None), dict(tau=float("inf")), dict(skip=None, tau=0.0), dict(tau=5.5)):
        run_both(gpu_state, mid["clip"], samples, size, mid["links"], **kw)
    a = clip_ref.augment(None, samples, size, links=mid["links"], flows=flows, skip=skip, tau=float("inf"), want=("valid",))["valid"]
    b = clip_ref.augment(None, samples, size, links=mid["links"], flows=flows, tau=float("inf"), want=("valid",))["valid"]
    assert (a != b).any() and (a <= b).all()


def shifted(a, shift=1):
    """a device copy of `a` whose base lies `shift` elements behind an aligned allocation"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    room = torch.zeros(t.numel() + shift, dtype=t.dtype, device="cuda")
    room[shift:] = t.reshape(-1).cuda()
    return room[shift:].view(t.shape)


def out_tensors(B, T, L, P, w, h, shift):
    form = {"video": ((B, T, 3, h, w), torch.float32), "flows": ((B, L, 2, h, w), torch.float32), "valid": ((B, L, h, w), torch.uint8),
            "tracks": ((B, T, P, 2), torch.float32), "vis": ((B, T, P), torch.uint8)}
    return {k: torch.zeros(int(np.prod(s)) + shift, dtype=dt, device="cuda")[shift:].view(s) for k, (s, dt) in form.items()}


@pytest.mark.parametrize("size", [(64, 16), (68, 5), (65, 9)], ids=lambda s: "%dx%d" % s)
def test_misaligned_bases_and_two_runs(gpu_state, mid, size):
    """every input and every output one element into a larger allocation: frames, skip and occ at odd addresses (the dword
    taps straddle dwords), flows, pos and tracks at 4 mod 8 (no 8-byte access), the float planes at 4 mod 16 (no 16-byte
    store although w % 4 == 0); aligned again: the same bytes"""
    W, H, B, T, P = mid["W"], mid["H"], mid["B"], mid["T"], mid["P"]
    samples = samples_of(W, H, *size, B, T, first=4)
    host = mid["clip"]
    want = clip_ref.augment(host[0], samples, size, links=mid["links"], flows=host[1], skip=host[2], pos=host[3], occ=host[4],
                            tables=lib_tables)
    runs = []
    for shift in (0, 1, 0):
        dev = [shifted(a, shift) for a in host]
        out = out_tensors(B, T, 2, P, *size, shift)
        if shift:
            assert all(t.data_ptr() % 2 == 1 for t in (dev[0], dev[2], dev[4], out["valid"], out["vis"]))
            assert all(t.data_ptr() % 8 == 4 for t in (dev[1], dev[3], out["tracks"])) and out["video"].data_ptr() % 16 == 4
        got = opt.augment_clips(gpu_state, dev[0], samples, size, links=mid["links"], flows=dev[1], skip=dev[2], pos=dev[3], occ=dev[4], out=out)
        assert all(got[k].data_ptr() == out[k].data_ptr() for k in out)
        same(got, want)
        runs.append({k: t.cpu().numpy().tobytes() for k, t in got.items()})
    assert runs[0] == runs[1] == runs[2]
    # only one side of the 8-byte rule off: pos aligned and tracks not, and the other way round
    for sp, so in ((0, 1), (1, 0)):
        out = {"tracks": out_tensors(B, T, 2, P, *size, so)["tracks"]}
        got = opt.augment_clips(gpu_state, None, samples, size, pos=shifted(host[3], sp), want=("tracks",), out=out)
        same(got, {"tracks": want["tracks"]})


def test_byte_taps_equal_dword_taps(gpu_state, monkeypatch):
    """ARAPOPT_AUG_BYTES=1 selects k_augment_clip<false> at any size (a state reads it when it is made)"""
    monkeypatch.setenv("ARAPOPT_AUG_BYTES", "1")
    st = opt.State()
    try:
        for W, H in SOURCES:
            c = make_clip(W, H, 3, 3, 2, 5, seed=W)
            samples = samples_of(W, H, 65, 17, 3, 3, first=4)
            kw = dict(links=((0, 1), (1, 2)), flows=c[1], skip=c[2], scale=SCALE, bias=BIAS)
            want = clip_ref.augment(c[0], samples, (65, 17), tables=lib_tables, **kw)
            a = opt.augment_clips(st, c[0], samples, (65, 17), **kw)
            b = opt.augment_clips(gpu_state, c[0], samples, (65, 17), **kw)
            same(a, want)
            same(b, want)
            assert all(a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes() for k in want), (W, H)
    finally:
        st.close()


@pytest.mark.parametrize("size", [(65, 17), (64, 16), (3, 2)], ids=lambda s: "%dx%d" % s)
def test_a_clip_of_two_frames_is_augment_pairs(gpu_state, size):
    """T = 2, L = 1, links = (0, 1), no rectangle on frame 0: the device's own pair call, bit for bit"""
    W, H, B = 70, 9, 7
    ts = transforms(W, H, *size)
    frames, flows, skip, _, _ = make_clip(W, H, B, 2, 1, 1, seed=31)
    dev = [torch.from_numpy(a).cuda() for a in (frames, flows, skip)]
    samples = [[opt.ClipFrame(s.T1, s.gain1, s.gamma1, (), s.fill), opt.ClipFrame(s.T2, s.gain2, s.gamma2, s.erase, s.fill)] for s in ts]
    pair = opt.augment_pairs(gpu_state, dev[0][:, 0].contiguous(), dev[0][:, 1].contiguous(), dev[1][:, 0].contiguous(), ts, size,
                             skip=dev[2][:, 0].contiguous(), scale=SCALE, bias=BIAS)
    got = opt.augment_clips(gpu_state, dev[0], samples, size, links=((0, 1),), flows=dev[1], skip=dev[2], scale=SCALE, bias=BIAS)
    assert torch.equal(got["video"][:, 0], pair["img1"]) and torch.equal(got["video"][:, 1], pair["img2"])
    assert torch.equal(got["flows"][:, 0], pair["flow"]) and torch.equal(got["valid"][:, 0], pair["valid"])
    assert bool(pair["valid"].any()) and not bool(torch.isnan(got["video"]).any())


@pytest.mark.parametrize("inputs", ["numpy", "device"])
def test_clips_equal_twin_on_a_side_stream(gpu_state, mid, inputs):
    W, H, B, T = mid["W"], mid["H"], mid["B"], mid["T"]
    host = mid["clip"]
    side = torch.cuda.Stream()
    try:
        gpu_state.set_stream(side)
        with torch.cuda.stream(side):
            ins = [torch.from_numpy(a).cuda() for a in host] if inputs == "device" else host
            for size in ((65, 9), (64, 8), (3, 2)):
                samples = samples_of(W, H, *size, B, T, first=2)
                kw = dict(links=mid["links"], scale=SCALE, bias=BIAS)
                want = clip_ref.augment(host[0], samples, size, flows=host[1], skip=host[2], pos=host[3], occ=host[4], tables=lib_tables, **kw)
                got = opt.augment_clips(gpu_state, ins[0], samples, size, flows=ins[1], skip=ins[2], pos=ins[3], occ=ins[4], **kw)
                side.synchronize()
                same(got, want)
    finally:
        gpu_state.set_stream(None)


def test_crafted_case_on_the_device(gpu_state):
    """tests/test_clip_host.py's case with every reason for a hidden point"""
    import test_clip_host
    c = test_clip_host.crafted()
    kw = dict(links=c["links"], flows=c["flows"], skip=c["skip"], pos=c["pos"], occ=c["occ"])
    want = clip_ref.augment(c["frames"], c["samples"], c["size"], tables=lib_tables, **kw)
    assert 0.3 <= (want["vis"] != 0).mean() <= 0.7
    same(opt.augment_clips(gpu_state, c["frames"], c["samples"], c["size"], **kw), want)


def test_flow_and_tracks_agree_on_the_device(gpu_state):
    """as tests/test_clip_host.py states it for the twin, here for the kernels, seven clips a call.  Largest error / bound
    on the MI355X: DESIGN.md "Training clips"."""
    import aug_cases
    import test_clip_host as t
    W, H, w, h = aug_cases.AFFINE_SIZES
    flow, cases = t.flow_track_inputs()
    worst = 0.0
    for first in range(0, len(cases), 7):
        part = cases[first:first + 7]
        samples = [[opt.CLIP_NEUTRAL._replace(T=T1), opt.CLIP_NEUTRAL._replace(T=T2)] for _, T1, T2, _ in part]
        got = opt.augment_clips(gpu_state, None, samples, (w, h), links=((0, 1),), flows=np.concatenate([flow] * len(part)),
                                pos=np.stack([p for _, _, _, p in part]), tau=float("inf"), want=("flows", "valid", "tracks"))
        out, valid, tracks = (got[k].cpu().numpy() for k in ("flows", "valid", "tracks"))
        for i, (name, T1, T2, pos) in enumerate(part):
            worst = max(worst, t.flow_track_check(name, out[i, 0], valid[i, 0] != 0, tracks[i], pos, T1, T2, w, h))
    print("flow and tracks, kernels: largest error / bound %.3f" % worst)


def test_bad_arguments_return_minus_one_and_write_nothing(gpu_state, mid):
    W, H, B, T, P = mid["W"], mid["H"], mid["B"], mid["T"], mid["P"]
    w, h, L = 48, 8, 2
    frames, flows, skip, pos, occ = (torch.from_numpy(a).cuda() for a in mid["clip"])
    good = samples_of(W, H, w, h, B, T, first=4)
    out = out_tensors(B, T, L, P, w, h, 0)
    for t in out.values():
        t.fill_(7)
    lib, st = gpu_state.lib, gpu_state.handle
    o = tuple(out[k] for k in opt.CLIP_OUTPUTS)

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == 7).all()) for t in out.values())

    def raw(st=st, dims=(W, H, w, h, B, T, L, P), ins=(frames, flows, skip, pos, occ), links=mid["links"], samples=good, scale=(1, 1, 1),
            bias=(0, 0, 0), tau=1.0, outs=o, n_erase=None):
        table = None
        if samples is not None:
            table = (capi.ClipFrame * (len(samples) * len(samples[0])))(*[opt.clip_frame(f) for s in samples for f in s])
            if n_erase is not None:
                table[4].n_erase = n_erase
        lt = None if links is None else (C.c_int32 * max(1, 2 * len(links)))(*[v for l in links for v in l])
        f3 = lambda v: None if v is None else (C.c_float * 3)(*v)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        fr, fl, sk, ps, oc = (ptr(t) for t in ins)
        return lib.ArapFlow_AugmentClips(st, *dims, fr, lt, fl, sk, ps, oc, table, f3(scale), f3(bias), tau, *[ptr(t) for t in outs])

    assert raw(tau=float("inf")) == 0
    torch.cuda.synchronize()
    assert not any(bool((t == 7).all()) for t in out.values())
    for t in out.values():
        t.fill_(7)
    N5 = (None,) * 5
    bad_frame = lambda f: [good[0], [good[1][0], f, good[1][2]], good[2]]
    refused = [dict(st=None), dict(samples=None), dict(scale=None), dict(bias=None), dict(outs=N5),
               # a null input that an asked output needs
               dict(ins=(None, flows, skip, pos, occ)), dict(ins=(frames, None, skip, pos, occ)), dict(ins=(frames, flows, skip, None, occ)),
               dict(ins=(frames, flows, skip, pos, None)), dict(ins=(frames, None, skip, pos, occ), outs=(None, None, o[2], None, None)),
               dict(ins=(frames, flows, skip, None, occ), outs=(None, None, None, o[3], None)),
               dict(ins=(frames, flows, skip, pos, None), outs=(None, None, None, None, o[4])),
               # sizes and limits
               dict(dims=(0, H, w, h, B, T, L, P)), dict(dims=(W, 0, w, h, B, T, L, P)), dict(dims=(W, H, 0, h, B, T, L, P)),
               dict(dims=(W, H, w, 0, B, T, L, P)), dict(dims=(W, H, w, h, 0, T, L, P)), dict(dims=(W, H, w, h, B, 0, L, P)),
               dict(dims=(1 << 16, 1 << 15, w, h, B, T, L, P)), dict(dims=(W, H, 1 << 16, 1 << 15, 1, 1, L, P)),
               dict(dims=(W, H, 1 << 15, 1 << 13, 2, 4, L, P)), dict(dims=(W, H, 1 << 15, 1 << 13, 4, 1, 2, P)),
               dict(dims=(W, H, w, h, 65, 1, L, P)), dict(dims=(W, H, w, h, 1, 17, L, P)), dict(dims=(W, H, w, h, 17, 16, L, P)),
               dict(dims=(W, H, w, h, B, T, 33, P)), dict(dims=(W, H, w, h, B, T, L, 1 << 28)),
               # links and points asked without any
               dict(dims=(W, H, w, h, B, T, 0, P)), dict(links=None), dict(dims=(W, H, w, h, B, T, L, 0)),
               dict(dims=(W, H, w, h, B, T, 0, P), outs=(None, None, o[2], None, None)),
               dict(dims=(W, H, w, h, B, T, L, 0), outs=(None, None, None, None, o[4])),
               # links out of range
               dict(links=((0, 1), (0, 3))), dict(links=((0, 1), (-1, 2))), dict(links=((1, 1), (0, 2))), dict(links=((0, 1), (T, 0))),
               dict(tau=float("nan")), dict(tau=-1.0), dict(tau=-float("inf")), dict(n_erase=5), dict(n_erase=0xffffffff),
               dict(samples=bad_frame(good[1][1]._replace(T=(1, 0, float("nan"), 0, 1, 0)))),
               dict(samples=bad_frame(good[1][1]._replace(T=(1, 2, 0, 2, 4, 0)))),
               dict(samples=[[good[0][0]._replace(T=(0, 0, 1, 0, 0, 1)), good[0][1], good[0][2]], good[1], good[2]]),      # det == 0 on a first frame
               dict(samples=bad_frame(good[1][1]._replace(gain=(1, 0, 1)))), dict(samples=bad_frame(good[1][1]._replace(gamma=float("inf")))),
               # an output over an input, an output over another output
               dict(outs=(frames, o[1], o[2], o[3], o[4])), dict(outs=(o[0], flows, o[2], o[3], o[4])),
               dict(outs=(o[0], o[1], skip.view(-1)[B * L * H * W - 1:], o[3], o[4])), dict(outs=(o[0], o[1], o[2], pos, o[4])),
               dict(outs=(o[0], o[1], o[2], o[3], occ.view(-1)[5:])), dict(outs=(o[0], o[1], o[2], frames, o[4])),
               dict(outs=(o[0], o[0], o[2], o[3], o[4])), dict(outs=(o[0], o[1], o[2], o[1].view(-1)[7:], o[4])),
               dict(outs=(o[0], o[1], o[2], o[3], o[2].view(-1)[B * L * w * h - 1:]))]
    for kw in refused:
        assert raw(**kw) == -1, sorted(kw)
    assert untouched()
    # an input that no asked output needs may be null or overlap anything, and its links are not looked at
    assert raw(ins=(frames, None, None, None, None), links=None, outs=(o[0], None, None, None, None)) == 0
    assert raw(ins=(o[0], flows, None, None, None), outs=(None, o[1], o[2], None, None)) == 0
    assert raw(ins=(None, None, None, pos, o[4]), links=((9, 9), (0, 0)), outs=(None, None, None, o[3], None)) == 0
    assert raw(ins=(frames, None, None, None, None), dims=(W, H, w, h, B, T, 0, 0), outs=(o[0], None, None, None, None)) == 0
    torch.cuda.synchronize()
    # the wrapper turns -1 into a ValueError and checks what it can before the call
    kw = dict(links=mid["links"], flows=flows, skip=skip, pos=pos, occ=occ)
    for bad in (dict(tau=float("nan")), dict(tau=-0.5), dict(want=()), dict(want=("video", "depth")), dict(scale=(1, 1)),
                dict(out={"video": out["video"][..., 1:]}), dict(out={"valid": out["flows"]}), dict(links=((0, 1), (0, 5))),
                dict(links=((0, 1),)), dict(links=((0, 1, 2), (0, 2))), dict(flows=flows[:, :, :-1]), dict(occ=occ[:, :, :-1])):
        with pytest.raises(ValueError):
            opt.augment_clips(gpu_state, frames, good, (w, h), **dict(kw, **bad))
    for size in ((0, h), (w, 0)):
        with pytest.raises(ValueError):
            opt.augment_clips(gpu_state, frames, good, size, **kw)
    for samples in (good[:2], [good[0], good[1], good[2][:2]], []):
        with pytest.raises(ValueError):
            opt.augment_clips(gpu_state, frames, samples, (w, h), **kw)


def test_kernel_timing_sees_both_kernels(gpu_state, mid):
    W, H, B, T = mid["W"], mid["H"], mid["B"], mid["T"]
    frames, flows, skip, pos, occ = mid["clip"]
    samples = samples_of(W, H, 48, 8, B, T)
    gpu_state.set_kernel_timing(True)
    try:
        opt.augment_clips(gpu_state, frames, samples, (48, 8), links=mid["links"], flows=flows, skip=skip, pos=pos, occ=occ)
        opt.augment_clips(gpu_state, frames, samples, (48, 8), want=("video",))
        opt.augment_clips(gpu_state, None, samples, (48, 8), pos=pos, want=("tracks",))
        torch.cuda.synchronize()
        image, tracks = gpu_state.kernel_time("k_augment_clip"), gpu_state.kernel_time("k_clip_tracks")
    finally:
        gpu_state.set_kernel_timing(False)
    assert image is not None and image[1] == 2 and image[0] > 0          # a launch whose outputs are all NULL is not made
    assert tracks is not None and tracks[1] == 2 and tracks[0] > 0
