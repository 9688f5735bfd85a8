"""GPU: the frame solver's result groups (base, extra outputs, in-between frames, fold diagnostics) through both of
their routes, the copying getters (results / snapshot) and the pinned views of a `download` solve (host_results /
host_snapshot), at a shape where every stride of the staging is rounded and the batch is larger than the solve:
N = 3500, so that none of N, 3N, 8N is a multiple of 256, and 2 frames in a solver of 3 slots.  Slot 1 has no RGB."""
import numpy as np
import pytest

from arap_flow_amd import opt, synth

pytestmark = pytest.mark.gpu
W, H, BATCH, NFRAMES = 70, 50, 3, 2
SCHEDULE = (3, 1, 10)
HAS_RGB = (True, False)
BASE_KEYS = {"flow", "warped_rgb", "warped_mask"}
EXTRA_KEYS = {"backward_flow", "occlusion_bwd", "occlusion"}
DIAG_KEYS = {"mesh_stats", "fold"}


@pytest.fixture(scope="module")
def frames():
    fr = [synth.make_frame(W, H, seed=s, fd=3) for s in (21, 22)]
    assert all(len(f["constraints"]) > 0 for f in fr)
    return fr


@pytest.fixture(scope="module")
def solver(gpu_state, frames):
    """one solver object for the whole module: the second test runs on the buffers the first one left"""
    fs = opt.FrameSolver(gpu_state, W, H, batch=BATCH)
    for b, f in enumerate(frames):
        fs.set_frame(b, f["mask_red"], f["constraints"], rgb=f["rgb"] if HAS_RGB[b] else None)
    yield fs
    fs.close()


@pytest.fixture(scope="module")
def alone(gpu_state, frames):
    """every frame in a solver of its own on the blocking route"""
    out = []
    for b, f in enumerate(frames):
        fs = opt.FrameSolver(gpu_state, W, H, batch=1)
        fs.set_outputs(backward=True, occlusion=True)
        fs.set_frame(0, f["mask_red"], f["constraints"], rgb=f["rgb"] if HAS_RGB[b] else None)
        fs.solve(1, *SCHEDULE)
        fs.warp(1)
        out.append(fs.results(0, want_rgb=HAS_RGB[b]))
        fs.close()
    return out


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, dict):
        return set(a) == set(b) and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def _async(fs, warp=True, download=True):
    fs.solve_async(NFRAMES, *SCHEDULE, warp=warp, download=download)
    fs.wait()


def _check_snapshot(fs, b, k):
    host, copy = fs.host_snapshot(b, k), fs.snapshot(b, k, want_rgb=HAS_RGB[b])
    assert set(host) == set(copy) == {"flow", "rgb", "mask", "step"}
    for key in host:
        assert _same(host[key], copy[key]), (b, k, key)
    assert (host["rgb"] is not None) == HAS_RGB[b]
    return host


def test_host_views_equal_copies_for_every_result_group(solver, alone):
    fs = solver
    fs.set_outputs(backward=True, occlusion=True)
    fs.set_snapshots((1, 2))
    fs.set_diag(True)
    _async(fs)
    for b in range(NFRAMES):
        host, copy = fs.host_results(b), fs.results(b, want_rgb=HAS_RGB[b])
        assert set(host) == BASE_KEYS | EXTRA_KEYS | DIAG_KEYS
        for key in host:
            assert _same(host[key], copy[key]), (b, key)
        assert (host["warped_rgb"] is not None) == HAS_RGB[b]
        # not trivially equal
        assert (host["flow"] != 0).any() and (host["warped_mask"] != 0).any() and host["mesh_stats"]["triangles"] > 0
        for k in range(2):
            s = _check_snapshot(fs, b, k)
            assert (s["flow"] != 0).any() and (s["step"] != 0).any() and (s["mask"] != 0).any()
        # the slot's planes are its own: those of the frame solved alone
        for key in ("flow", "warped_mask", "backward_flow", "occlusion"):
            assert _same(host[key], alone[b][key]), (b, key)
    with pytest.raises(ValueError):
        fs.snapshot(1, 0, want_rgb=True)


def test_results_follow_the_last_warp_and_the_last_download(solver):
    fs = solver
    # occlusion only, one snapshot, diag off
    fs.set_outputs(occlusion=True)
    fs.set_snapshots((2,))
    fs.set_diag(False)
    _async(fs)
    for b in range(NFRAMES):
        host = fs.host_results(b)
        assert set(host) == BASE_KEYS | {"occlusion"}
        assert _same(host["occlusion"], fs.results(b, want_rgb=HAS_RGB[b])["occlusion"])
        _check_snapshot(fs, b, 0)
        with pytest.raises(ValueError):
            fs.host_snapshot(b, 1)
        with pytest.raises(ValueError):
            fs.snapshot(b, 1, want_rgb=HAS_RGB[b])
    # a download without a warp carries the base group alone
    _async(fs, warp=False)
    for b in range(NFRAMES):
        assert set(fs.host_results(b)) == BASE_KEYS
        with pytest.raises(ValueError):
            fs.host_snapshot(b, 0)
    # a blocking solve downloads nothing
    fs.solve(NFRAMES, *SCHEDULE)
    with pytest.raises(ValueError):
        fs.host_results(0)
    # more snapshots than the buffers were made for; the last one is ramp step numIter, i.e. the final result
    fs.set_snapshots((1, 2, 3))
    _async(fs)
    for b in range(NFRAMES):
        host, s = fs.host_results(b), _check_snapshot(fs, b, 2)
        assert _same(s["flow"], host["flow"]) and _same(s["mask"], host["warped_mask"])
        assert (s["flow"] != 0).any()
        if HAS_RGB[b]:
            assert _same(s["rgb"], host["warped_rgb"])
