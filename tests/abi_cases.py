"""One table of the entry points that work on caller-owned device memory (include/arap_opt.h, part 2), for the tests that
call them the way a C caller does: tests/test_abi_host.py, tests/test_gpu_abi_buffers.py, tests/test_gpu_abi_streams.py.

A row says nothing about argument order: the wrappers of arap_flow_amd/opt.py already state it once (every one of them
hands opt._warp_call a description of its call), so a row runs its wrapper against a recorder (capture) and keeps the
description as a Call: the ctypes function, its host values, its inputs as host arrays, its outputs as sizes, its scratch
size function and that function's arguments.  Call then carves those buffers out of an abi_pool.Pool instead of
torch.empty tensors, and makes the call itself.  ArapFlow_AugmentPairs, whose wrapper keeps its tensors on the device,
states its description here in the same form.

The inputs and the expected outputs come from the builders and twins the families' own tests use (tests/*_ref.py and the
case builders of tests/test_gpu_*.py); nothing is restated.

Shapes per row: the smallest at which the call's scratch parts and launch grids have a ragged edge -- W no multiple of 64
and H no multiple of 4; for calls with N + 1 cell counters, N = W * H with 4 (N + 1) an exact multiple of 256 (21x3: no
slack behind the counters), with 4 N one (64x4: the last counter starts a new 256 bytes) and neither; where another size
than the frame's sizes a part (P, T, samples, K), that size above and below the frame's.  Nothing is larger than 130x70.

Alignments: `scratch` is promised 256 bytes; where the header is silent a buffer owes its element type's alignment: 8 for
float2 data, 8 for the 64-bit tables, 4 for float planes and ArapFlow_MeshStats, 2 for the 16-bit distances, 1 for bytes.
Every kernel of these families but four reads and writes such buffers one element at a time (arap_warp.h, arap_occ.h,
arap_layers.h, arap_layers_step.h, arap_track.h, arap_bg.h, arap_tex.h, arap_blur.h, arap_light.h, arap_seg.h,
arap_tscore.h, arap_chain.h, arap_interp.h, arap_diag.h hold no wider access to a caller's buffer); the four that load or
store groups -- k_flow_score, k_frame_score, k_mscore_count, k_augment -- test the addresses first (ScoreJob::vec,
FScoreJob::vec, MScoreJob::vec, AugJob::vec) and go element by element otherwise.  Those rows are run a second time with
every buffer at 16 bytes ("vec"), which takes the group path."""
import collections
import ctypes as C
import functools
import types

import numpy as np
import torch

import aug_ref
import bg_ref
import bg_seq_ref
import diag_ref
import interp_ref
import layers_step_ref as sref
import light_ref
import mid_ref
import mscore_ref
import occ_layers_ref as lref
import occ_ref
import score_ref
import fscore_ref
import tex_ref
import track_ref as tref
import tscore_ref
from arap_flow_amd import capi, opt, pipeline
from aug_cases import transforms

F = np.float32


def fixture_body(f):
    """the function behind a pytest fixture of another test module (its case builder)"""
    return getattr(f, "__wrapped__", None) or f.__pytest_wrapped__.obj


# ---- a call's description ----------------------------------------------------------------------------------------------
Val = collections.namedtuple("Val", "value")                          # a host value, passed as it is
Buf = collections.namedtuple("Buf", "name kind data nbytes align")    # a device buffer; data: an input's host array
BufList = collections.namedtuple("BufList", "name items")             # a host array of device pointers; items: Buf or None
Scratch = collections.namedtuple("Scratch", "fn args nbytes")


def element_align(dtype, shape):
    """what a caller owes a buffer the header says nothing about: its element type's alignment"""
    dtype = np.dtype(dtype)
    if dtype == np.float32 and len(shape) >= 2 and shape[-1] == 2:
        return 8                                                       # float2
    return dtype.itemsize


def _torch_np(dt):
    return {torch.uint8: np.uint8, torch.int16: np.int16, torch.float32: np.float32, torch.int64: np.int64}[dt]


class Call:
    """ArapFlow_<name>(state, *args): what to pass, what to carve"""

    def __init__(self, name, args):
        self.name, self.args = name, args

    @classmethod
    def from_descriptor(cls, lib, name, dims, inputs, outputs, scratch=None, lead=(), **_):
        args = [Val(int(d)) for d in dims]
        for i, a in enumerate(lead):
            args.append(cls._input("lead%d" % i, *a) if isinstance(a, tuple) else Val(a))
        for i, (a, dt) in enumerate(inputs):
            args.append(Val(a) if dt is None or a is None else cls._input("in%d" % i, a, dt))
        for key, shape, tdt in outputs:
            dt = _torch_np(tdt)
            if isinstance(shape, list):
                args.append(BufList(key, [None if q is None else cls._output("%s[%d]" % (key, k), q, dt) for k, q in enumerate(shape)]))
            else:
                args.append(Val(None) if shape is None else cls._output(key, shape, dt))
        if scratch:
            fn, sdims = scratch if isinstance(scratch, tuple) else (scratch, dims)
            sdims = tuple(int(v) for v in sdims)
            args.append(Scratch("ArapFlow_" + fn, sdims, int(getattr(lib, "ArapFlow_" + fn)(*sdims))))
        return cls(name, args)

    @staticmethod
    def _input(name, a, dt):
        if isinstance(a, list):
            return BufList(name, [None if x is None else Call._input("%s[%d]" % (name, k), x, dt) for k, x in enumerate(a)])
        a = np.ascontiguousarray(a, dt)
        return Buf(name, "input", a, a.nbytes, element_align(dt, a.shape))

    @staticmethod
    def _output(name, shape, dt):
        return Buf(name, "output", None, int(np.prod(shape)) * np.dtype(dt).itemsize, element_align(dt, shape))

    def bufs(self, kind=None):
        for a in self.args:
            for b in (a.items if isinstance(a, BufList) else [a]):
                if isinstance(b, Buf) and (kind is None or b.kind == kind):
                    yield b

    def outputs(self):
        return [b.name for b in self.bufs("output")]

    @property
    def scratch(self):
        return next((a for a in self.args if isinstance(a, Scratch)), None)

    def with_aligns(self, aligns):
        """a copy whose buffers sit at aligns[name] (or aligns["*"]) where given"""
        def one(b):
            if isinstance(b, Buf):
                return b._replace(align=aligns.get(b.name, aligns.get("*", b.align)))
            if isinstance(b, BufList):
                return b._replace(items=[one(x) for x in b.items])
            return b
        return Call(self.name, [one(a) for a in self.args])

    # -- over a pool ----------------------------------------------------------------------------------------------------
    def carve(self, pool, tag="", only=None, scratch="scratch"):
        """carve the inputs, the outputs `only` names (None: all) and the scratch, which calls that name the same
        `scratch` share; exactly the bytes asked, each at its alignment and no more"""
        for b in self.bufs():
            if b.kind == "input" or only is None or b.name in only:
                pool.carve(tag + b.name, b.nbytes, b.align, b.kind)
        s = self.scratch
        if s is not None and scratch not in pool.layout.parts:
            assert s.nbytes > 0
            pool.carve(scratch, s.nbytes, 256, "scratch")

    def upload(self, pool, tag=""):
        for b in self.bufs("input"):
            pool.upload(tag + b.name, b.data)

    def invoke(self, lib, handle, pool, tag="", scratch="scratch", null=None, values=None):
        """the call: every buffer's pointer from the pool (NULL for an output that was not carved, and for the buffer
        `null` names); `values`: {position among the arguments: host value} passed instead"""
        keep, argv = [], []
        for k, a in enumerate(self.args):
            if values and k in values:
                argv.append(values[k])
            elif isinstance(a, Val):
                argv.append(a.value)
            elif isinstance(a, Buf):
                argv.append(None if a.name == null else pool.ptr(tag + a.name))
            elif isinstance(a, BufList):
                arr = (C.c_void_p * max(1, len(a.items)))(*[None if b is None or b.name == null else pool.ptr(tag + b.name) for b in a.items])
                keep.append(arr)
                argv.append(arr)
            else:
                argv.append(None if null == "scratch" else pool.ptr(scratch))
        return getattr(lib, "ArapFlow_" + self.name)(handle, *argv)

    def position(self, name):
        """where among the arguments the buffer `name` (or "scratch") is"""
        for k, a in enumerate(self.args):
            if (isinstance(a, Scratch) and name == "scratch") or (isinstance(a, Buf) and a.name == name):
                return k
        raise KeyError(name)


HOST = None


def host_state():
    """what a wrapper needs of a state to describe its call: the library (no device is touched)"""
    global HOST
    if HOST is None:
        HOST = types.SimpleNamespace(lib=capi.load(), handle=None)
    return HOST


class _Captured(Exception):
    pass


def capture(wrapper, *a, **kw):
    """the Call a wrapper of arap_flow_amd/opt.py would make"""
    rec = {}

    def recorder(state, name, dims, inputs, outputs, scratch=None, bad_args=True, lead=(), view=None):
        rec.update(name=name, dims=dims, inputs=inputs, outputs=outputs, scratch=scratch, lead=lead)
        raise _Captured()
    real = opt._warp_call
    opt._warp_call = recorder
    try:
        wrapper(host_state(), *a, **kw)
    except _Captured:
        pass
    finally:
        opt._warp_call = real
    assert rec, "%s made no call" % wrapper.__name__
    return Call.from_descriptor(host_state().lib, **rec)


# a built case: the call and {output name: the twin's array}
Built = collections.namedtuple("Built", "call twin")


def flat(twin):
    """{name: array} with a list output spread as name[k]"""
    out = {}
    for k, v in twin.items():
        if isinstance(v, list):
            out.update({"%s[%d]" % (k, i): a for i, a in enumerate(v) if a is not None})
        elif v is not None:
            out[k] = v
    return out


def differ(a, b):
    """the output names on which two twins differ"""
    a, b = flat(a), flat(b)
    return [k for k in a if k in b and np.ascontiguousarray(a[k]).tobytes() != np.ascontiguousarray(b[k]).tobytes()]


# ---- the families' cases ------------------------------------------------------------------------------------------------
# single-layer warps: 67x9 (ragged both ways, 2 x 3 blocks), 64x4 (4 N a multiple of 256), 21x3 (4 (N + 1) one), 129x65
WARP_SHAPES = {"67x9": (67, 9), "64x4": (64, 4), "21x3": (21, 3), "129x65": (129, 65)}


@functools.lru_cache(maxsize=None)
def warp_case(shape, seed=None):
    W, H = WARP_SHAPES[shape]
    rgb, mask, fl = occ_ref.folded_case(W, H, 2.0, seed=seed)
    return rgb, mask, fl, occ_ref.warp_ref(rgb, mask, occ_ref.field_from_flow(fl))


def warp(shape, seed=None):
    rgb, mask, fl, ref = warp_case(shape, seed)
    return Built(capture(opt.warp_image, rgb, mask, fl), {k: ref[k] for k in ("warped_rgb", "warped_mask")})


def warp_ex(shape, seed=None):
    rgb, mask, fl, ref = warp_case(shape, seed)
    return Built(capture(opt.warp_image_ex, rgb, mask, fl), ref)


@functools.lru_cache(maxsize=None)
def warp_step(shape, seed=None):
    W, H = WARP_SHAPES[shape]
    rgb, mask, fa, fb = mid_ref.two_state_case(W, H, W * H if seed is None else seed, "folded")
    a, b = occ_ref.field_from_flow(fa), occ_ref.field_from_flow(fb)
    ref = occ_ref.warp_ref(rgb, mask, a)
    return Built(capture(opt.warp_step, rgb, mask, fa, fb),
                 dict(warped_rgb=ref["warped_rgb"], warped_mask=ref["warped_mask"], step=mid_ref.step_ref(mask, a, b)))


def stats_struct(stats):
    """the twin's statistics as the bytes of an ArapFlow_MeshStats (reserved = 0)"""
    s = capi.MeshStats()
    for k in capi.MESH_STATS_KEYS:
        setattr(s, k, float(stats[k]) if k in diag_ref.FLOAT_KEYS else int(stats[k]))
    return np.frombuffer(bytes(s), np.uint8)


DIAG_SHAPES = {"67x9": (67, 9), "64x4": (64, 4), "130x70": (130, 70)}


@functools.lru_cache(maxsize=None)
def warp_diag(shape, seed=0, fold=True):
    """a 30 % background, a noisy flow that folds triangles, one NaN and one inf vertex"""
    W, H = DIAG_SHAPES[shape]
    rng = np.random.default_rng([W, H, seed])
    mask = np.where(rng.random((H, W)) < 0.3, 255, 0).astype(np.uint8)
    fl = rng.normal(0, 0.5, (H, W, 2)).astype(F)
    fl[H // 2, W // 3, 0], fl[1, 2 * W // 3, 1] = np.nan, np.inf
    stats, fmap = diag_ref.diag(mask, diag_ref.flow_pos(fl))
    assert stats["folded"] and stats["nonfinite"]
    twin = dict(fold=fmap, stats=stats_struct(stats)) if fold else dict(stats=stats_struct(stats))
    return Built(capture(opt.warp_diag, mask, fl, fold=fold).with_aligns({"stats": 4}), twin)


# layered calls: the shapes of tests/layers_step_ref.py -- 10x8 and 70x50 and 129x65 (ragged), 64x4 (4 N a multiple of
# 256), 5x1 (a single row: no rasterised quad) -- and 21x3 (4 (N + 1) a multiple of 256)
LAYER_SHAPES = {"10x8-n3": sref.MULTI[0], "70x50-n3": sref.MULTI[3], "129x65-n5": sref.MULTI[4], "64x4-n2": sref.MULTI[5],
                "5x1-n1": sref.SINGLE[2], "21x3-n2": (21, 3, 2, 4, True)}


@functools.lru_cache(maxsize=None)
def layer_case(shape, seed=None):
    W, H, n, s, overlap = LAYER_SHAPES[shape]
    rgb, masks, fa, fb = sref.two_state_layers(W, H, n, s if seed is None else seed, overlap=overlap)
    return rgb, masks, fa, fb


@functools.lru_cache(maxsize=None)
def warp_layers(shape, seed=None):
    rgb, masks, fa, _ = layer_case(shape, seed)
    ref = lref.layers_ref(rgb, masks, lref.fields_from_flows(fa))
    keys = ("warped_rgb", "warped_mask", "backward_flow", "occlusion_bwd", "occlusion")
    return Built(capture(opt.warp_layers, rgb, masks, fa, bwd=True, occ_bwd=True, occ=True), {k: ref[k] for k in keys})


@functools.lru_cache(maxsize=None)
def warp_layers_step(shape, seed=None):
    rgb, masks, fa, fb = layer_case(shape, seed)
    A, B = lref.fields_from_flows(fa), lref.fields_from_flows(fb)
    ref = sref.layers_step_ref(masks, A, B)
    twin = dict(warped_rgb=lref.layers_ref(rgb, masks, A)["warped_rgb"], warped_mask=ref["warped_mask"], step=ref["step"],
                occlusion_step=ref["occlusion_step"])
    return Built(capture(opt.warp_layers_step, rgb, masks, fa, fb), twin)


# tracks: P above N (the case's own point set) and below it (257 of its sub-pixel points), two states and one
TRACK_SHAPES = {"10x8-n3-P>N": ("10x8-n3", 2, None), "70x50-n3-P<N": ("70x50-n3", 2, 257), "64x4-n2-T1": ("64x4-n2", 1, None),
                "21x3-n2-P<N": ("21x3-n2", 2, 40)}


@functools.lru_cache(maxsize=None)
def track_points(shape, seed=None):
    layers, T, P = TRACK_SHAPES[shape]
    W, H, n, s, _ = LAYER_SHAPES[layers]
    _, masks, fa, fb = layer_case(layers, seed)
    flows = np.stack([fa, fb])[:T]
    pts = tref.case_points(W, H, s if seed is None else seed)
    assert len(pts) > W * H
    if P is not None:
        pts = pts[W * H + 20 + np.arange(P)]                   # sub-pixel points
        assert len(pts) < W * H
    ref = tref.track_ref(masks, np.stack([lref.fields_from_flows(f) for f in flows]), pts)
    return Built(capture(opt.track_points, masks, flows, pts), dict(pos=ref["pos"], occ=ref["occ"]))


BG_SHAPES = {"67x9": (67, 9, 80, 23, (6, 7)), "130x70": (130, 70, 150, 90, (10, 10))}      # tests/test_gpu_background.py's


@functools.lru_cache(maxsize=None)
def background(shape, seed=None):
    """the ellipse pair of tests/test_gpu_background.py, its warp from the rasteriser's twin, a rotated and scaled camera"""
    W, H, bw, bh, (left, top) = BG_SHAPES[shape]
    c = bg_ref.ellipse_case(W, H, bw, bh, seed=W if seed is None else seed)
    if seed is not None:                                 # (the builder's object and flow do not depend on the seed: move them)
        c["mask_red"] = np.roll(c["mask_red"], 5, axis=1)
        c["flow"] = (np.roll(c["flow"], 5, axis=1) * F(0.75)).astype(F)
    r = occ_ref.warp_ref(c["rgb1"], c["mask_red"], occ_ref.field_from_flow(c["flow"]))
    M1 = np.array([1, 0, left, 0, 1, top], F)
    deg = 3.0 if seed is None else -2.0
    M2 = bg_ref.compose(M1, bg_ref.similarity(deg, 1.02, (2.5, -1.25), ((W - 1) / 2.0, (H - 1) / 2.0)))
    G, Ginv = opt.background_maps(M1, M2)
    args = (c["rgb1"], c["mask_red"], r["warped_rgb"], r["warped_mask"], c["flow"], r["occlusion"], r["backward_flow"], r["occlusion_bwd"])
    twin = bg_ref.background(c["bg"], M1, M2, G, Ginv, *args)
    return Built(capture(opt.background, c["bg"], M1, M2, *args[:5], occ=args[5], bwd=args[6], occ_bwd=args[7]), twin)


@functools.lru_cache(maxsize=None)
def background_seq(shape, seed=None):
    if seed is None:
        c = bg_seq_ref.sized_case(shape)
    else:
        W, H, bw, bh, (left, top), m = bg_seq_ref.SIZES[shape]
        c = bg_seq_ref.seq_case(W, H, bw, bh, m, seed=seed)
        move = lambda a, s=1: None if a is None else np.ascontiguousarray((np.roll(a, 4, axis=1) * s).astype(a.dtype))
        c["mask_red"], c["covers"] = move(c["mask_red"]), [move(a) for a in c["covers"]]     # (they do not depend on the seed)
        c["flows"] = [move(a, F(0.75)) for a in c["flows"]]
        c["maps"] = bg_seq_ref.camera(np.array([1, 0, left, 0, 1, top], F), m, W, H, deg=-2.0)
    Gs = [opt.background_maps(c["maps"][f], c["maps"][f + 1])[0] for f in range(c["m"] - 1)]
    with np.errstate(all="ignore"):
        twin = bg_seq_ref.background_seq(c["bg"], c["maps"], Gs, c["mask_red"], c["covers"], c["rgbs"], c["flows"], c["occs"])
    return Built(capture(opt.background_seq, c["bg"], c["maps"], c["mask_red"], c["covers"], c["rgbs"], c["flows"], c["occs"]), twin)


@functools.lru_cache(maxsize=None)
def _family(module):
    """the read-only cases of a family's GPU test module"""
    return fixture_body(__import__(module).cases)()


TEX_SHAPES = {"70x9-n3": ("70x9", 3, 1), "130x70-n1": ("130x70", 1, 2)}


@functools.lru_cache(maxsize=None)
def texture(shape, variant=0):
    """variant 0: the case; 1: the decoy (another frame); 2: the case under other layer descriptions"""
    import test_gpu_tex as t
    size, n, kind = TEX_SHAPES[shape]
    c = _family("test_gpu_tex")[size]
    rgb = c["rgb"] if variant != 1 else np.ascontiguousarray(c["rgb"][::-1, ::-1])
    masks = c["masks"][:n] if variant != 1 else np.ascontiguousarray(c["masks"][:n, :, ::-1])
    layers = t.layers_for((kind + 2) % len(tex_ref.KINDS) if variant == 2 else kind, n, size=5.0 if variant != 2 else 3.0)
    return Built(capture(opt.texture, rgb, masks, layers), dict(rgb=tex_ref.texture(rgb, masks, layers)))


# samples at most and more than ARAPFLOW_BLUR_CHUNK: without and with the carried sums
BLUR_SHAPES = {"70x9-n3-S5": ("70x9-n3", 5), "70x9-n3-S9": ("70x9-n3", capi.BLUR_CHUNK + 1), "130x70-n3-S2": ("130x70-n3", 2)}


@functools.lru_cache(maxsize=None)
def blur_layers(shape, decoy=False):
    import test_gpu_blur as t
    name, S = BLUR_SHAPES[shape]
    c = _family("test_gpu_blur")[name]
    if decoy:                                            # mirrored, the other way round in time, before another picture
        flip = lambda a, axis: np.ascontiguousarray(np.flip(a, axis=axis))          # (axis: the one x runs along)
        c = dict(c, rgb=flip(c["rgb"], 1), masks=flip(c["masks"], 2), flows=flip(c["flows_a"], 2), flows_a=flip(c["flows"], 2),
                 bg=flip(c["bg"], 0))
    want = t.blur_ref.blur_ref(c["rgb"], c["masks"], c["flows"], 0.0, 1.0, S, flows_a=c["flows_a"], bg=c["bg"], Ma=c["Ma"], Mb=c["Mb"])
    call = capture(opt.blur_layers, c["rgb"], c["masks"], c["flows"], 0.0, 1.0, S, flows_a=c["flows_a"], bg=c["bg"], maps=(c["Ma"], c["Mb"]))
    return Built(call, dict(rgb=want[0], alpha=want[1]))


LIGHT_SHAPES = ("70x9", "130x70", "7x5")


@functools.lru_cache(maxsize=None)
def relight(shape, variant=0):
    """variant 0: the case; 1: the decoy (another frame and cover); 2: the case under another tone table and shadow"""
    import test_gpu_light as t
    c = _family("test_gpu_light")[shape]
    frame = pipeline.LightFrame(7, t.FIELD, 0.3, 1.0, (1.1, 0.9, 1.0), 2.2, 5, -3, 16, 256, 1.0, 0.05)
    if variant == 2:
        frame = frame._replace(gain=(0.7, 1.3, 0.9), gamma=0.45, sh_r=1, sh_dx=-2)
    rgb = c["rgb"] if variant != 1 else np.ascontiguousarray(255 - c["rgb"][::-1])
    cover = c["cover"] if variant != 1 else np.ascontiguousarray(c["cover"][:, ::-1])
    return Built(capture(opt.relight, rgb, cover, frame), dict(rgb=light_ref.relight(rgb, cover, frame)))


SEG_SHAPES = ("70x9-n3", "7x5-n1", "130x70-n1")


@functools.lru_cache(maxsize=None)
def seg_maps(shape, decoy=False):
    import seg_ref
    import test_gpu_seg as t
    c = t.Case(shape)
    if decoy:
        c.masks, c.flows, c.fold, c.nan = seg_ref.seg_case(c.W, c.H, c.n, seed=1000 + c.W)
    M1, M2 = c.cams["moving"]
    return Built(capture(opt.seg_maps, c.masks, c.flows, tau=1.0, radius=16, M1=M1, M2=M2), c.twin("moving", 1.0, 16))


SCORE_SHAPES = {"71x9x3": (71, 9, 3), "65x4x1": (65, 4, 1), "5x3x1": (5, 3, 1)}


@functools.lru_cache(maxsize=None)
def flow_score(shape, seed=0):
    import test_gpu_score as t
    c = t.case(*SCORE_SHAPES[shape], seed=seed)
    ref = score_ref.score_ref(c["gt"], c["est"], occ=c["occ"], dist=c["dist"], skip=c["skip"])
    return Built(capture(opt.flow_score, c["gt"], c["est"], occ=c["occ"], dist=c["dist"], skip=c["skip"], err=True),
                 dict(table=ref["table"], err=ref["err"]))


FSCORE_SHAPES = {"71x9x3": (71, 9, 3), "69x37x1": (69, 37, 1), "5x3x1": (5, 3, 1)}


@functools.lru_cache(maxsize=None)
def frame_score(shape, seed=0):
    import test_gpu_fscore as t
    c = t.case(*FSCORE_SHAPES[shape], seed=seed)
    planes = {k: c[k] for k in t.KEYS}
    ref = fscore_ref.fscore_ref(c["ref"], c["est"], **planes)
    return Built(capture(opt.frame_score, c["ref"], c["est"], ssim=True, **planes), dict(table=ref["table"], ssim=ref["ssim"]))


TSCORE_SHAPES = {"F5-P257": (5, 257), "F2-P63": (2, 63), "F64-P300": (64, 300)}


@functools.lru_cache(maxsize=None)
def track_score(shape, seed=0):
    c = tscore_ref.random_case(*TSCORE_SHAPES[shape], seed)
    return Built(capture(opt.track_score, *c, scale=tscore_ref.TAPVID_854x480),
                 dict(table=tscore_ref.track_score_ref(*c, tscore_ref.TAPVID_854x480)))


# P below and above N
CHAIN_SHAPES = {"33x17-L8-P257": (33, 17, 8, 257), "9x5-L2-P300": (9, 5, 2, 300), "64x8-L1-P255": (64, 8, 1, 255)}


@functools.lru_cache(maxsize=None)
def chain_flows(shape, seed=0):
    import test_gpu_chain as t
    flows, bwd, pts = t.case(*CHAIN_SHAPES[shape], seed=seed)
    pos, occ = tscore_ref.chain_ref(flows, pts, bwd)
    return Built(capture(opt.chain_flows, flows, pts, bwd=bwd), dict(pos=pos, occ=occ))


MSCORE_SHAPES = {"71x9x3": (71, 9, 3), "65x4x1": (65, 4, 1), "130x70x1": (130, 70, 1)}


@functools.lru_cache(maxsize=None)
def label_score(shape, seed=0):
    import test_gpu_mscore as t
    c = t.case(*MSCORE_SHAPES[shape], seed=seed)
    ref = mscore_ref.label_ref(c["gt"], c["est"], 3, 8, c["skip"])
    return Built(capture(opt.label_score, c["gt"], c["est"], 3, 8, skip=c["skip"]), dict(table=ref["table"]))


@functools.lru_cache(maxsize=None)
def map_score(shape, seed=0):
    import test_gpu_mscore as t
    c = t.case(*MSCORE_SHAPES[shape], seed=seed)
    ref = mscore_ref.map_ref(c["occ"], c["score"], c["skip"], (64, 128), 2)
    return Built(capture(opt.map_score, c["occ"], c["score"], skip=c["skip"], thr=(64, 128), radius=2),
                 dict(hist=ref["hist"], match=ref["match"]))


# K = 1, 3 and the most
INTERP_SHAPES = {"70x9-K1": (70, 9, (0.5,)), "300x5-K3": (300, 5, (0.25, float(F(9) / F(19)), 0.875)),
                 "13x6-K32": (13, 6, tuple(float(F(i) / F(33)) for i in range(1, 33)))}


@functools.lru_cache(maxsize=None)
def interp_frames(shape, seed=0):
    import test_gpu_interp as t
    W, H, times = INTERP_SHAPES[shape]
    A, B, fwd, bwd = t.case(W, H, seed=seed)
    out, src = interp_ref.interp_ref(A, B, fwd, times, bwd)
    return Built(capture(opt.interp_frames, A, B, fwd, times, bwd=bwd, want_src=True), dict(out=out, src=src))


# source, B, crop: a crop no multiple of four wide and a tile plus one pixel each way; one exact tile (the 16-byte stores,
# where the planes are aligned for them); w = 4 and one row from a wide source
AUG_SHAPES = {"70x9-B3-65x17": (70, 9, 3, 65, 17), "70x9-B3-64x16": (70, 9, 3, 64, 16), "300x5-B1-4x1": (300, 5, 1, 4, 1)}


@functools.lru_cache(maxsize=None)
def augment_pairs(shape, variant=0):
    """variant 0: the case; 1: the decoy (other frames); 2: the case under other samples"""
    import test_gpu_aug as t
    W, H, B, w, h = AUG_SHAPES[shape]
    rgb1, rgb2, flow, skip = t.make_pair(W, H, B, seed=W + B + (500 if variant == 1 else 0))
    if variant == 1:                                     # (the builder's flow does not depend on the seed)
        flow = flow * F(0.5)
    ts = transforms(W, H, w, h)
    first = 3 if variant == 2 else 1
    samples = [ts[(first + i) % len(ts)] for i in range(B)]
    twin = aug_ref.augment(rgb1, rgb2, flow, samples, (w, h), skip=skip, tables=opt.augment_tables, scale=t.SCALE, bias=t.BIAS, tau=1.0)
    table = (capi.AugSample * B)(*[opt.aug_sample(s) for s in samples])
    # opt.augment_pairs keeps its tensors on the device and makes the call itself: its description, in _warp_call's form
    call = Call.from_descriptor(host_state().lib, "AugmentPairs", (W, H, w, h, B),
                                [(rgb1, np.uint8), (rgb2, np.uint8), (flow, np.float32), (skip, np.uint8), (table, None),
                                 (opt._f3(t.SCALE, "scale"), None), (opt._f3(t.BIAS, "bias"), None), (1.0, None)],
                                [("img1", (B, 3, h, w), torch.float32), ("img2", (B, 3, h, w), torch.float32),
                                 ("flow", (B, 2, h, w), torch.float32), ("valid", (B, h, w), torch.uint8)])
    return Built(call.with_aligns({"flow": 4}), twin)


# ---- the table ------------------------------------------------------------------------------------------------------------
class Row:
    """one entry point.  shapes: {id: builder of the Built}; the first is the one the stream tests use.
    minimal: the smallest legal set of outputs (None: every output is required); refuse: how a refused call is made --
    ("null", buffer) passes that required pointer as NULL, ("size", {argument position: value}) a size the call (and its
    size function) refuses; decoy: the builder of a second valid input set of the smallest shape; third: of a third call
    whose host table or parameters differ from both; vec: run a second time with every buffer at 16 bytes;
    waits: the call is documented to return only when its outputs are written; nan_any: float outputs in which a NaN is
    compared as a NaN, whatever its sign and payload (every other value bit for bit)"""

    def __init__(self, name, shapes, minimal, refuse, decoy, third=None, vec=False, waits=False, nan_any=()):
        self.name, self.shapes, self.minimal, self.refuse = name, shapes, minimal, refuse
        self.decoy, self.third, self.vec, self.waits, self.nan_any = decoy, third, vec, waits, nan_any
        self.first = next(iter(shapes))

    def build(self, shape):
        return self.shapes[shape]()


def _shapes(fn, ids, *a):
    return {s: functools.partial(fn, s, *a) for s in ids}


ROWS = [
    Row("Warp", _shapes(warp, WARP_SHAPES), ("warped_mask",), ("null", "in2"), lambda: warp("67x9", 1)),
    Row("WarpEx", _shapes(warp_ex, WARP_SHAPES), ("warped_mask",), ("size", {0: 0}), lambda: warp_ex("67x9", 1)),
    Row("WarpStep", _shapes(warp_step, WARP_SHAPES), ("warped_mask", "step"), ("size", {0: 0}), lambda: warp_step("67x9", 1), waits=True),
    Row("WarpDiag", _shapes(warp_diag, DIAG_SHAPES), ("stats",), ("size", {1: 0}), lambda: warp_diag("67x9", 1),
        third=lambda: warp_diag("67x9", 2, False)),
    Row("WarpLayers", _shapes(warp_layers, LAYER_SHAPES), ("warped_mask",), ("size", {2: 0}), lambda: warp_layers("10x8-n3", 2)),
    Row("WarpLayersStep", _shapes(warp_layers_step, LAYER_SHAPES), ("occlusion_step",), ("size", {2: 256}),
        lambda: warp_layers_step("10x8-n3", 2)),
    Row("TrackPoints", _shapes(track_points, TRACK_SHAPES), ("pos",), ("size", {4: capi.MAX_SNAPSHOTS + 2}),
        lambda: track_points("10x8-n3-P>N", 2)),
    Row("Background", _shapes(background, BG_SHAPES), ("occ_full",), ("null", "lead0"), lambda: background("67x9", 5)),
    Row("BackgroundSeq", _shapes(background_seq, bg_seq_ref.SIZES), ("occ_full[0]",), ("size", {5: 1}), lambda: background_seq("67x9", 5)),
    Row("Texture", _shapes(texture, TEX_SHAPES), None, ("size", {2: 0}), lambda: texture("70x9-n3", 1), third=lambda: texture("70x9-n3", 2)),
    Row("BlurLayers", _shapes(blur_layers, BLUR_SHAPES), ("alpha",), ("size", {9: capi.MAX_BLUR_SAMPLES + 1}),
        lambda: blur_layers("70x9-n3-S5", True)),
    Row("Relight", _shapes(relight, LIGHT_SHAPES), None, ("null", "in0"), lambda: relight("70x9", 1), third=lambda: relight("70x9", 2)),
    Row("SegMaps", _shapes(seg_maps, SEG_SHAPES), ("idx1",), ("size", {2: 256}), lambda: seg_maps("70x9-n3", True)),
    Row("FlowScore", _shapes(flow_score, SCORE_SHAPES), ("table",), ("size", {2: 0}), lambda: flow_score("71x9x3", 1), vec=True),
    Row("TrackScore", _shapes(track_score, TSCORE_SHAPES), None, ("size", {0: 1}), lambda: track_score("F5-P257", 1)),
    # a point that lands on a NaN flow sample gets a NaN the arithmetic made: IEEE 754 leaves its sign and payload open, the
    # twin's numpy and the kernel choose differently, and tests/test_gpu_chain.py compares it as a NaN too
    Row("ChainFlows", _shapes(chain_flows, CHAIN_SHAPES), None, ("size", {2: 0}), lambda: chain_flows("33x17-L8-P257", 1), nan_any=("pos",)),
    Row("FrameScore", _shapes(frame_score, FSCORE_SHAPES), ("table",), ("size", {2: 0}), lambda: frame_score("71x9x3", 1), vec=True),
    Row("LabelScore", _shapes(label_score, MSCORE_SHAPES), None, ("size", {3: 256}), lambda: label_score("71x9x3", 1), vec=True),
    Row("MapScore", _shapes(map_score, MSCORE_SHAPES), None, ("size", {8: 255}), lambda: map_score("71x9x3", 1), vec=True),
    Row("InterpFrames", _shapes(interp_frames, INTERP_SHAPES), ("out",), ("size", {6: 33}), lambda: interp_frames("70x9-K1", 1)),
    Row("AugmentPairs", _shapes(augment_pairs, AUG_SHAPES), ("valid",), ("size", {4: capi.AUG_MAX_BATCH + 1}),
        lambda: augment_pairs("70x9-B3-65x17", 1), third=lambda: augment_pairs("70x9-B3-65x17", 2), vec=True),
]
BY_NAME = {r.name: r for r in ROWS}

# every case of the buffer tests: (row, shape, "min" or "vec")
CASES = [(r.name, s, "min") for r in ROWS for s in r.shapes] + [(r.name, s, "vec") for r in ROWS if r.vec for s in r.shapes]


def built(name, shape, aligns="min"):
    b = BY_NAME[name].build(shape)
    return b if aligns == "min" else Built(b.call.with_aligns({"*": 16}), b.twin)
