"""GPU: data.ClipLoader (arap_flow_amd/data.py, DESIGN.md "Training clips") on a three-clip tree: the batches of the
kernels equal those the same loader makes on the numpy twin, they are CUDA tensors of the current device, a second epoch
differs from the first, and batch_at between the steps of an epoch gives the undisturbed bytes."""
import functools

import numpy as np
import pytest
import torch

import clip_ref
from arap_flow_amd import data, opt

pytestmark = pytest.mark.gpu
CFG = data.AUG_DEFAULT._replace(erase_size=(3, 12), erase_max=4)
TWIN = functools.partial(clip_ref.as_augment, tables=lambda f, scale, bias: opt.clip_tables(f, scale, bias))
KW = dict(batch=2, size=(48, 8), cfg=CFG, seed=4, jobs=4, scale=(1 / 58.395, 1 / 57.12, 1 / 57.375), bias=(-2.1179, -2.0357, -1.8044))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """(the clips, the bytes of the epochs 0 and 1 from a loader on the twin that nothing disturbs)"""
    root = str(tmp_path_factory.mktemp("clips"))
    clip_ref.write_clip_tree(root, 3, 70, 9, steps=(4, 9, 14), P=33)
    clips = data.ClipList(root, links=("next", "first"))
    host = data.ClipLoader(clips, None, augment=TWIN, **KW)
    want = [list(host.epoch(e)) for e in range(2)]
    host.close()
    return clips, want


def equal(got, want, where):
    assert sorted(got) == sorted(want) == ["flows", "tracks", "valid", "video", "vis"]
    for k, t in got.items():
        assert t.is_cuda and t.device.index == torch.cuda.current_device(), k
        a = t.cpu().numpy()
        assert a.shape == tuple(want[k].shape) and not np.isnan(a).any(), (where, k)
        assert np.array_equal(a, want[k].numpy()), (where, k)


def test_loader_equals_the_loader_on_the_twin(gpu_state, tree):
    clips, want = tree
    dev = data.ClipLoader(clips, gpu_state, **KW)
    try:
        epochs = []
        for e in range(2):
            got = list(dev)
            assert len(got) == len(want[e]) == 2
            for k, (g, w) in enumerate(zip(got, want[e])):
                equal(g, w, (e, k))
            assert got[0]["video"].shape == (2, 5, 3, 8, 48) and got[0]["flows"].shape == (2, 8, 2, 8, 48)
            assert got[1]["valid"].shape == (1, 8, 8, 48) and got[1]["tracks"].shape == (1, 5, 33, 2) and got[1]["vis"].shape == (1, 5, 33)
            epochs.append([{k: t.cpu().numpy().tobytes() for k, t in g.items()} for g in got])
        assert all(epochs[0][i][k] != epochs[1][i][k] for i in range(2) for k in ("video", "flows", "tracks"))
        assert any((g["vis"] != 0).any() and (g["vis"] == 0).any() and (g["valid"] != 0).any() for g in want[0])
    finally:
        gpu_state.set_stream(None)
        dev.close()


def test_batch_at_between_the_steps_of_an_epoch(gpu_state, tree):
    clips, want = tree
    dev = data.ClipLoader(clips, gpu_state, **KW)
    try:
        it = dev.epoch(0)
        for k in range(2):
            equal(next(it), want[0][k], (0, k))
            for e, j in ((1, 1), (0, 1 - k), (1, 0)):
                equal(dev.batch_at(e, j), want[e][j], (k, e, j))
        with pytest.raises(StopIteration):
            next(it)
    finally:
        gpu_state.set_stream(None)
        dev.close()
