"""GPU: data.AugmentLoader (arap_flow_amd/data.py, DESIGN.md "Training batches").  On a three-pair tree: the batches of the
kernel equal those the same loader makes on the numpy twin, they are CUDA tensors of the current device, and a second
epoch differs from the first.  On an eleven-pair tree, two pairs a batch, so that every pinned buffer set is used again
and again: unaugmented batches are the files themselves, also when the stream is so busy that a set's upload is still
pending when the loader wants the set back; batches taken under two streams in turn and batch_at between the steps of
an epoch equal the loader on the twin."""
import functools

import numpy as np
import pytest
import torch

import aug_cases
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


# ---- eleven pairs, two a batch: six batches, the last one ragged ----------------------------------------------------------
W, H = 70, 9
F = np.float32
TWIN = functools.partial(aug_ref.as_augment, tables=lambda s, scale, bias: opt.augment_tables(s, scale, bias))
BLOCK = 0.05            # seconds of device work queued in front of a batch


@pytest.fixture(scope="module")
def eleven(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("eleven"))
    return root, aug_ref.write_tree(root, 11, W, H)


def the_files(made, k):
    """batch k of the unaugmented, unshuffled loader, as tests/test_data_host.py states it for one batch"""
    out = dict(img1=[], img2=[], flow=[], valid=[])
    for i in range(2 * k, min(2 * k + 2, len(made))):
        m = made[i]
        bad = ~np.isfinite(m["flow"]).all(-1) | ((m["fold"] != 0) if i % 2 == 0 else False)
        out["img1"].append(np.moveaxis(m["rgb1"][""], -1, 0).astype(F))
        out["img2"].append(np.moveaxis(m["rgb2"][""], -1, 0).astype(F))
        out["valid"].append(np.where(bad, 0, 255).astype(np.uint8))
        out["flow"].append(np.where(bad[None], F(0), np.moveaxis(m["flow"], -1, 0)))
    return {k: np.stack(v) for k, v in out.items()}


def equal(got, want, where):
    assert sorted(got) == sorted(want)
    for k in want:
        g, w = got[k].cpu().numpy(), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), (where, k)


def identity_loader(root, state):
    return data.AugmentLoader(data.PairList(root), state, batch=2, size=(W, H), cfg=data.AUG_NONE, shuffle=False, jobs=4)


def test_unaugmented_batches_are_the_files_over_two_epochs(gpu_state, eleven):
    """every buffer set is used three times an epoch, and a ragged batch is followed by a full one in the same set"""
    root, made = eleven
    ld = identity_loader(root, gpu_state)
    try:
        for e in range(2):
            got = list(ld)
            assert len(got) == 6 and got[5]["img1"].shape == (1, 3, H, W)
            for k, g in enumerate(got):
                equal(g, the_files(made, k), (e, k))
    finally:
        gpu_state.set_stream(None)
        ld.close()


def test_unaugmented_batches_are_the_files_behind_a_busy_stream(gpu_state, eleven):
    """BLOCK seconds of device work go in front of every batch, so a set's upload has not run when the loader wants the
    set for the batch after next: the loader has to wait for that upload before it decodes into the set.  At least one
    next() must return before its block has finished, or the test shows nothing."""
    root, made = eleven
    ld = identity_loader(root, gpu_state)
    side = torch.cuda.Stream()
    try:
        with torch.cuda.stream(side):
            work = aug_cases.BusyWork(side)
            got, pending = [], []
            for e in range(2):
                it = iter(ld)
                for k in range(6):
                    work.queue(BLOCK)
                    block = torch.cuda.Event()
                    block.record()
                    got.append((e, k, next(it)))
                    pending.append(not block.query())
            side.synchronize()
        print("batches returned before the work in front of them had finished: %d of %d" % (sum(pending), len(pending)))
        assert any(pending)
        for e, k, g in got:
            equal(g, the_files(made, k), (e, k))
    finally:
        gpu_state.set_stream(None)
        ld.close()


def augmenting_loaders(root, state):
    kw = dict(batch=2, size=(48, 8), cfg=CFG, seed=4, jobs=4, scale=(1 / 58.395, 1 / 57.12, 1 / 57.375), bias=(-2.1179, -2.0357, -1.8044))
    pairs = data.PairList(root)
    return data.AugmentLoader(pairs, state, **kw), data.AugmentLoader(pairs, None, augment=TWIN, **kw)


def test_batches_under_two_streams_in_turn(gpu_state, eleven):
    """even batches under stream a, behind BLOCK seconds of work each, odd ones under stream b.  The state's one sample
    table is why the loader orders the two: when an odd batch is ready on b, the batch before it has been made on a."""
    root, _ = eleven
    dev, host = augmenting_loaders(root, gpu_state)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    try:
        want = list(host.epoch(0))
        work = aug_cases.BusyWork(a)
        it, got = dev.epoch(0), []
        for k in range(6):
            with torch.cuda.stream(b if k % 2 else a):
                if k % 2 == 0:
                    work.queue(BLOCK)
                got.append(next(it))
                made = torch.cuda.Event()
                made.record()
                if k % 2:
                    made.synchronize()
                    assert before.query(), k
                before = made
        a.synchronize()
        b.synchronize()
        for k in range(6):
            equal(got[k], want[k], k)
    finally:
        gpu_state.set_stream(None)
        dev.close()
        host.close()


def test_batch_at_between_the_steps_of_an_epoch(gpu_state, eleven):
    root, _ = eleven
    dev, host = augmenting_loaders(root, gpu_state)
    try:
        want = [list(host.epoch(e)) for e in range(2)]
        it = dev.epoch(0)
        for k in range(6):
            equal(next(it), want[0][k], k)
            for e, j in ((0, (k + 2) % 6 // 2 * 2), (0, 3), (1, 4), (1, 5)):
                equal(dev.batch_at(e, j), want[e][j], (k, e, j))
    finally:
        gpu_state.set_stream(None)
        dev.close()
        host.close()
