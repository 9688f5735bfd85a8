"""GPU: segment maps (ArapFlow_SegMaps, DESIGN.md "Segment maps") through opt.seg_maps against the numpy twin
tests/seg_ref.py, byte for byte.

Shapes: 70x9 (two block columns and three block rows of the 64x4 blocks, both partial), 130x70 (several full blocks),
7x5 (a frame smaller than any window) and 300x6 with radius 254 (the staged row window of a block spans several blocks
and runs past both frame edges) and 9x200 (the column pass cuts a column into 64 runs of rows: runs of four rows here, of
two at 130x70, of one with empty runs behind them at the flat shapes; fewer columns than a block of that pass holds).  One layer and three overlapping ones (seg_ref.seg_case: whole-pixel shifts, a fold
strictly inside layer 0, a NaN vertex in the top layer); radius 0, 1, 16, 254; tau 0, 1, 1e30; a static background, two
bit-equal cameras (must equal static) and a rotated and scaled one.  The kernels have no other size-dependent path."""
import ctypes as C

import numpy as np
import pytest
import torch

import bg_ref
import seg_ref
from arap_flow_amd import capi, opt

pytestmark = pytest.mark.gpu
F = np.float32
SIZES = {"70x9": (70, 9), "130x70": (130, 70), "7x5": (7, 5), "300x6": (300, 6), "9x200": (9, 200)}
CASES = ["%s-n%d" % (s, n) for s in SIZES for n in (1, 3)]
RADII = (0, 1, 16, 254)
TAUS = (0.0, 1.0, 1e30)
CAMERAS = ("static", "same", "moving")


class Case:
    """one frame pair, read-only, with the twin's results cached by what they depend on"""

    def __init__(self, name):
        size, n = name.split("-n")
        self.W, self.H = SIZES[size]
        self.n = int(n)
        self.masks, self.flows, self.fold, self.nan = seg_ref.seg_case(self.W, self.H, self.n, seed=self.W + self.n)
        self.masks.setflags(write=False)
        self.flows.setflags(write=False)
        c = (self.W / 2, self.H / 2)
        self.cams = dict(static=None, same=(bg_ref.similarity(2.0, 1.01, (0.5, 0.25), c),) * 2,
                         moving=(bg_ref.similarity(3.0, 1.03, (1.5, -0.75), c), bg_ref.similarity(-2.0, 0.98, (-0.5, 1.25), c)))
        self._base, self._mb, self._dist = {}, {}, {}

    def base(self, cam):
        if cam not in self._base:
            G = Ginv = None
            if self.cams[cam] is not None:
                G, Ginv = opt.background_maps(*self.cams[cam])
            self._base[cam] = seg_ref.seg_ref(self.masks, self.flows, 1.0, 1, G, Ginv)
        return self._base[cam]

    def twin(self, cam, tau, radius):
        b = self.base(cam)
        out = dict(idx1=b["idx1"], idx2=b["idx2"])
        for f, key in (("1", "F1"), ("2", "B2")):
            if (cam, tau, f) not in self._mb:
                self._mb[cam, tau, f] = seg_ref.boundaries(b[key], tau)
            mb = out["mb" + f] = self._mb[cam, tau, f]
            if (cam, tau, f) not in self._dist:
                self._dist[cam, tau, f] = seg_ref.nearest2(mb)
            out["dist" + f] = seg_ref.distances(mb, radius, self._dist[cam, tau, f])
        return out

    def gpu(self, st, cam, tau, radius, **kw):
        M1, M2 = self.cams[cam] or (None, None)
        return opt.seg_maps(st, self.masks, self.flows, tau=tau, radius=radius, M1=M1, M2=M2, **kw)


@pytest.fixture(scope="module")
def cases():
    out = {name: Case(name) for name in CASES}
    for name, c in out.items():                    # no case is vacuous: asserted on the twin's own output
        t = c.twin("static", 1.0, 1)
        fx, fy = c.fold
        if c.W >= 70:                               # (the 7 x 5 frame has no room for an interior or, with one layer, a border)
            assert len(set(t["idx1"][fy - 1:fy + 2, fx - 1:fx + 2].ravel())) == 1 and t["mb1"][fy, fx] == 255, name   # the fold: inside
            border = (t["idx1"][:, 1:] != t["idx1"][:, :-1]) & (t["mb1"][:, 1:] == 255)
            assert border.any(), name               # and object borders
            for f in "12":
                d = t["dist" + f]
                assert (d == 0).any() and (d == 1).any() and (d == seg_ref.FAR).any(), name
        if c.n == 3:
            assert len(set(t["idx2"].ravel()) - {0}) >= 2, name
        big = c.twin("static", 1e30, 1)["mb1"]
        nx, ny = c.nan
        want = np.zeros_like(big)
        for x, y in ((nx, ny), (nx - 1, ny), (nx + 1, ny), (nx, ny - 1), (nx, ny + 1)):
            if 0 <= x < c.W and 0 <= y < c.H:
                want[y, x] = 255
        assert (big == want).all(), name            # tau = 1e30: only the NaN vertex and its neighbours
    return out


def same(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert got.tobytes() == want.tobytes(), "%s: %d values differ" % (what, int((got != want).sum()))


def same_all(got, want, what=""):
    assert set(got) <= set(seg_ref.OUTPUTS)
    for k in got:
        same(got[k], want[k], "%s %s" % (what, k))


@pytest.mark.parametrize("name", CASES)
def test_twin(gpu_state, cases, name):
    """every camera, tau and radius against the twin; at 130x70 the other two taus with the static camera and two radii only"""
    c = cases[name]
    for cam in CAMERAS:
        for tau in TAUS:
            for radius in RADII:
                if c.W == 130 and tau != 1.0 and (cam != "static" or radius not in (1, 254)):
                    continue
                got = c.gpu(gpu_state, cam, tau, radius)
                assert set(got) == set(seg_ref.OUTPUTS)
                same_all(got, c.twin(cam, tau, radius), "%s %s tau=%g r=%d" % (name, cam, tau, radius))


@pytest.mark.parametrize("name", ["70x9-n3", "7x5-n1"])
def test_same_camera_is_static(gpu_state, cases, name):
    c = cases[name]
    same_all(c.gpu(gpu_state, "same", 1.0, 16), c.gpu(gpu_state, "static", 1.0, 16))
    same_all(c.twin("same", 1.0, 16), c.twin("static", 1.0, 16))


@pytest.mark.parametrize("name", ["70x9-n1", "70x9-n3", "130x70-n3"])
def test_against_the_layered_warp(gpu_state, cases, name):
    """idx2 != 0 exactly where the layered warp's mask is set, n = 1 gives labels 0 / 1, idx1 is the top-most mask"""
    c = cases[name]
    got = c.gpu(gpu_state, "static", 1.0, 1, which=("idx1", "idx2"))
    wm = opt.warp_layers(gpu_state, None, c.masks, c.flows, occ=False)["warped_mask"]
    assert ((got["idx2"] != 0) == (wm != 0)).all()
    if c.n == 1:
        assert set(got["idx2"].ravel()) <= {0, 1}
    top = np.zeros((c.H, c.W), np.uint8)
    for l in range(c.n):
        top[c.masks[l] == 0] = l + 1
    same(got["idx1"], top)


SUBSETS = [(k,) for k in seg_ref.OUTPUTS] + [("idx1", "mb1", "dist1"), ("idx2", "mb2", "dist2"), ("mb1", "dist1"), ("idx2", "dist2")]


@pytest.mark.parametrize("name", ["70x9-n3"])
def test_subsets_and_repeat(gpu_state, cases, name):
    """each output alone and every subset that drops a frame gives the bytes of the full call; so does a second run"""
    c = cases[name]
    full = c.gpu(gpu_state, "moving", 1.0, 16)
    same_all(c.gpu(gpu_state, "moving", 1.0, 16), full, "second run")
    for which in SUBSETS:
        got = c.gpu(gpu_state, "moving", 1.0, 16, which=which)
        assert set(got) == set(which)
        same_all(got, full, "+".join(which))


def test_unused_passes_are_not_launched(gpu_state, cases):
    """launch counts through the per-kernel timer: a frame-1-only call runs no rasteriser kernel, a call without dist no
    distance pass"""
    c = cases["70x9-n3"]
    st = gpu_state
    count = lambda k: (st.kernel_time(k) or (0.0, 0))[1]
    try:
        st.set_kernel_timing(True)
        c.gpu(st, "static", 1.0, 16, which=("idx1", "mb1", "dist1"))
        assert [count(k) for k in ("k_seg_index1", "k_seg_jump", "k_seg_cols", "k_seg_rows")] == [1, 1, 1, 1]
        assert [count(k) for k in ("k_layers_raster", "k_layers_keys", "k_seg_index2", "k_warp_resolve")] == [0, 0, 0, 0]
        st.set_kernel_timing(True)                  # clears the records
        c.gpu(st, "static", 1.0, 16, which=("idx2", "mb1", "mb2"))
        assert [count(k) for k in ("k_layers_raster", "k_layers_keys", "k_seg_index2", "k_seg_jump")] == [1, 1, 1, 2]
        assert [count(k) for k in ("k_seg_cols", "k_seg_rows")] == [0, 0]
        st.set_kernel_timing(True)
        c.gpu(st, "static", 1.0, 16, which=("idx2",))
        assert [count(k) for k in ("k_layers_raster", "k_layers_keys", "k_seg_index1", "k_seg_jump")] == [1, 0, 0, 0]
        st.set_kernel_timing(True)
        c.gpu(st, "static", 1.0, 16)
        assert [count(k) for k in ("k_layers_raster", "k_seg_jump", "k_seg_cols", "k_seg_rows")] == [1, 2, 2, 2]
    finally:
        st.set_kernel_timing(False)


def raw(st, c, outs, scratch, masks=None, flows=None, M1=None, M2=None, tau=1.0, radius=16, dims=None, state=True):
    """ArapFlow_SegMaps itself on device tensors; `outs`: six tensors or None, in the library's order"""
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    m = lambda q: None if q is None else (C.c_float * 6)(*[float(v) for v in q])
    W, H, n = dims or (c.W, c.H, c.n)
    torch.cuda.synchronize()
    rc = st.lib.ArapFlow_SegMaps(st.handle if state else None, W, H, n, p(masks), p(flows), m(M1), m(M2), tau, radius,
                                 *[p(t) for t in outs], p(scratch))
    torch.cuda.synchronize()
    return rc


def device_case(st, c):
    masks, flows = torch.from_numpy(c.masks.copy()).cuda(), torch.from_numpy(c.flows.copy()).cuda()
    nbytes = st.lib.ArapFlow_SegMapsScratchBytes(c.W, c.H, c.n)
    assert nbytes >= 18 * c.W * c.H
    scratch = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
    outs = [torch.full((c.H, c.W), 77, dtype=torch.int16 if k.startswith("dist") else torch.uint8, device="cuda")
            for k in seg_ref.OUTPUTS]
    return masks, flows, scratch, outs


def test_dirty_scratch_and_clean_keys(gpu_state, cases):
    """a scratch buffer full of junk gives the twin's bytes; the key image is zero afterwards and a following layered warp
    is what it was"""
    c = cases["70x9-n3"]
    st = gpu_state
    before = opt.warp_layers(st, None, c.masks, c.flows, bwd=True)
    masks, flows, scratch, outs = device_case(st, c)
    assert raw(st, c, outs, scratch, masks, flows) == 0
    want = c.twin("static", 1.0, 16)
    for k, t in zip(seg_ref.OUTPUTS, outs):
        a = t.cpu().numpy()
        same(a.view(np.uint16) if k.startswith("dist") else a, want[k], k)
    assert not scratch[:8 * c.W * c.H].any()
    after = opt.warp_layers(st, None, c.masks, c.flows, bwd=True)
    for k in ("warped_mask", "backward_flow", "occlusion"):
        same(after[k], before[k], k)


def test_bad_arguments(gpu_state, cases):
    """every refusal: -1, and the outputs keep their bytes"""
    c = cases["70x9-n3"]
    st = gpu_state
    lib = st.lib
    masks, flows, scratch, outs = device_case(st, c)
    M = [1, 0, 0, 0, 1, 0]
    nan6, sing = [float("nan")] + M[1:], [1, 2, 0, 2, 4, 0]
    big = 1 << 16
    bad = [dict(state=False), dict(masks=None), dict(flows=None), dict(scratch=None), dict(outs=[None] * 6),
           dict(dims=(c.W, c.H, 0)), dict(dims=(c.W, c.H, 256)), dict(dims=(0, c.H, c.n)), dict(dims=(c.W, 0, c.n)),
           dict(dims=(big, big // 2, 1)), dict(M1=M), dict(M2=M), dict(M1=nan6, M2=M), dict(M1=M, M2=sing),
           dict(tau=-1.0), dict(tau=float("nan")), dict(tau=float("inf")), dict(radius=255),
           dict(outs=[outs[0], outs[0]] + outs[2:]), dict(outs=[masks[0]] + outs[1:]), dict(outs=outs[:4] + [flows[0], outs[5]]),
           dict(outs=outs[:5] + [scratch[256:256 + 2 * c.W * c.H]])]
    for kw in bad:
        a = dict(masks=masks, flows=flows, scratch=scratch, outs=outs)
        a.update(kw)
        o, s = a.pop("outs"), a.pop("scratch")
        assert raw(st, c, o, s, **a) == -1, kw
    for k, t in zip(seg_ref.OUTPUTS, outs):
        assert (t == 77).all(), k
    assert (scratch == 0xA5).all() and torch.equal(masks.cpu(), torch.from_numpy(c.masks.copy()))
    for dims in ((0, 5, 1), (5, 0, 1), (5, 5, 0), (5, 5, 256), (big, big // 2, 1)):
        assert lib.ArapFlow_SegMapsScratchBytes(*dims) == 0
    with pytest.raises(ValueError):
        opt.seg_maps(st, c.masks, c.flows, radius=capi.SEG_MAX_RADIUS + 1)
    with pytest.raises(ValueError):
        opt.seg_maps(st, c.masks, c.flows, tau=-1.0)
    with pytest.raises(ValueError):
        opt.seg_maps(st, c.masks, c.flows, which=())
    with pytest.raises(ValueError):
        opt.seg_maps(st, c.masks, c.flows, M1=M)
