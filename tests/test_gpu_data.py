"""GPU: data.AugmentLoader on a three-pair tree (arap_flow_amd/data.py, DESIGN.md "Training batches"): the batches of the
kernel equal those the same loader makes on the numpy twin, they are CUDA tensors of the current device, and a second
epoch differs from the first."""
import functools

import numpy as np
import pytest
import torch

import aug_ref
from arap_flow_amd import data, opt

pytestmark = pytest.mark.gpu
CFG = data.AUG_DEFAULT._replace(erase_size=(3, 12), erase_max=4)


def test_loader_equals_the_loader_on_the_twin(gpu_state, tmp_path):
    aug_ref.write_tree(str(tmp_path), 3, 70, 9)
    kw = dict(batch=2, size=(48, 8), cfg=CFG, seed=4, jobs=4, scale=(1 / 58.395, 1 / 57.12, 1 / 57.375), bias=(-2.1179, -2.0357, -1.8044))
    pairs = data.PairList(str(tmp_path))
    twin = functools.partial(aug_ref.as_augment, tables=lambda s, scale, bias: opt.augment_tables(s, scale, bias))
    dev, host = data.AugmentLoader(pairs, gpu_state, **kw), data.AugmentLoader(pairs, None, augment=twin, **kw)
    try:
        epochs = []
        for e in range(2):
            got, want = list(dev), list(host.epoch(e))
            assert len(got) == len(want) == 2
            for g, w in zip(got, want):
                assert sorted(g) == ["flow", "img1", "img2", "valid"]
                for k, t in g.items():
                    assert t.is_cuda and t.device.index == torch.cuda.current_device(), k
                    a = t.cpu().numpy()
                    assert a.shape == tuple(w[k].shape) and not np.isnan(a).any(), k
                    assert np.array_equal(a, w[k].numpy()), (e, k)
            assert got[0]["img1"].shape == (2, 3, 8, 48) and got[1]["valid"].shape == (1, 8, 48)
            epochs.append([{k: t.cpu().numpy().tobytes() for k, t in g.items()} for g in got])
        assert all(epochs[0][i][k] != epochs[1][i][k] for i in range(2) for k in ("img1", "img2", "flow"))
    finally:
        gpu_state.set_stream(None)
        dev.close()
        host.close()
