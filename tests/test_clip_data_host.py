"""CPU-only: from a --mid K --tracks P tree to batches of clips (DESIGN.md "Training clips", arap_flow_amd/data.py).
ClipList on trees written here (tests/clip_ref.py write_clip_tree): both link kinds, missing occlusion planes, a moved
tree, a track file of another length, a missing one; draw_clip: pure, draw_sample at T = 2, invertible maps, the identity
crop without augmentation; ClipLoader on the numpy twin: the same bytes for the same (seed, epoch, k), a ragged last
batch, batch_at between the steps of an epoch, a clip of another T."""
import os
import shutil

import numpy as np
import pytest

import clip_ref
from arap_flow_amd import data, opt, trk

F = np.float32
W, H = 70, 9
STEPS = (4, 9, 14)
T = len(STEPS) + 2


def as_bytes(batch):
    return {k: np.asarray(v).tobytes() for k, v in batch.items()}


def loader(root, links=("next",), tracks=True, **kw):
    kw = dict(dict(batch=2, size=(48, 8), seed=1, jobs=4, scale=(1 / 58.395, 1 / 57.12, 1 / 57.375), bias=(-2.1179, -2.0357, -1.8044)), **kw)
    return data.ClipLoader(data.ClipList(root, links=links, tracks=tracks), None, augment=clip_ref.as_augment, **kw)


# ---- ClipList -----------------------------------------------------------------------------------------------------------------
def test_clip_list_reads_both_link_kinds(tmp_path):
    made = clip_ref.write_clip_tree(str(tmp_path), 4, W, H, steps=STEPS, P=5)
    nxt = data.ClipList(str(tmp_path))
    both = data.ClipList(str(tmp_path), links=("next", "first"))
    first = data.ClipList(str(tmp_path), links=("first",), tracks=False)
    assert len(nxt) == len(both) == len(first) == 4 and nxt.P == 5
    assert nxt[0].links == ((0, 1), (1, 2), (2, 3), (3, 4)) and first[0].links == ((0, 1), (0, 2), (0, 3), (0, 4))
    assert both[0].links == nxt[0].links + first[0].links
    for i, m in enumerate(made):
        frames, links, flows, skip, pos, occ = both.load(i)
        assert links == both[i].links and frames.dtype == np.uint8 and flows.dtype == F and skip.dtype == np.uint8
        assert np.array_equal(frames, m["frames"])
        assert flows[:4].tobytes() == m["step"].tobytes() and flows[4:].tobytes() == m["first"].tobytes()     # (one NaN: bytes)
        assert np.array_equal(pos, m["pos"]) and np.array_equal(occ, m["occ"])
        zeros = np.zeros((H, W), np.uint8)
        want = [zeros if a is None else a for a in m["occ_step"]]                         # the "next" links
        want += [want[0], zeros, zeros, zeros if m["occ_pair"] is None else m["occ_pair"]]   # (0, 1) .. (0, 4)
        assert np.array_equal(skip, np.stack(want))
        assert (skip[:4].any() and skip[7].any()) == (i % 2 == 0)                       # the odd clips have no planes at all
        f2 = first.load(i)
        assert f2[4] is None and f2[5] is None and np.array_equal(f2[3], skip[4:]) and f2[2].tobytes() == flows[4:].tobytes()


def test_a_line_without_in_between_frames_is_no_clip(tmp_path):
    clip_ref.write_clip_tree(str(tmp_path), 3, W, H, steps=STEPS)
    for f in os.listdir(tmp_path / "Mid" / "seq1"):
        os.remove(tmp_path / "Mid" / "seq1" / f)
    cl = data.ClipList(str(tmp_path), tracks=False)
    assert len(cl) == 2 and all("seq0" in c.frames[0] for c in cl.clips)


def test_a_moved_tree_is_found_by_the_last_three_components(tmp_path):
    made = clip_ref.write_clip_tree(str(tmp_path / "there"), 2, W, H, steps=STEPS, named_root="/nowhere/OUT")
    cl = data.ClipList(str(tmp_path / "there"))
    assert len(cl) == 2 and np.array_equal(cl.load(1)[0], made[1]["frames"])


def test_track_files_of_another_length_and_missing_ones(tmp_path):
    root = str(tmp_path)
    made = clip_ref.write_clip_tree(root, 3, W, H, steps=STEPS, P=6)
    name = os.path.join(root, "Tracks", "seq1", "00001.trk")
    trk.write(name, W, H, made[1]["pos"][:, :4], made[1]["occ"][:, :4])            # fewer points: the first P of every file
    cl = data.ClipList(root)
    assert cl.P == 4 and np.array_equal(cl.load(0)[4], made[0]["pos"][:, :4]) and cl.load(2)[5].shape == (T, 4)
    trk.write(name, W, H, made[1]["pos"][:T - 1], made[1]["occ"][:T - 1])          # F != T
    with pytest.raises(ValueError, match="00001.trk"):
        data.ClipList(root)
    os.remove(name)
    with pytest.raises(ValueError, match="00001.trk"):
        data.ClipList(root)
    assert len(data.ClipList(root, tracks=False)) == 3
    with pytest.raises(ValueError):
        data.ClipList(root, links=("next", "last"))
    with pytest.raises(ValueError):
        data.ClipList(root, links=())


# ---- draw_clip ------------------------------------------------------------------------------------------------------------------
def test_draw_clip_is_pure_and_is_draw_sample_for_two_frames():
    a = data.draw_clip(data.AUG_DEFAULT, 3, 2, 5, 854, 480, 512, 384, 5)
    assert a == data.draw_clip(data.AUG_DEFAULT, 3, 2, 5, 854, 480, 512, 384, 5) and len(a) == 5
    assert a != data.draw_clip(data.AUG_DEFAULT, 3, 2, 6, 854, 480, 512, 384, 5)
    assert all(isinstance(f, opt.ClipFrame) for f in a)
    rects = 0
    for i in range(200):
        s = data.draw_sample(data.AUG_DEFAULT, 7, i % 3, i, 854, 480, 512, 384)
        c = data.draw_clip(data.AUG_DEFAULT, 7, i % 3, i, 854, 480, 512, 384, 2)
        assert len(c) == 2 and c[0].erase == ()
        assert (c[0].T, c[1].T, c[0].gain, c[0].gamma, c[1].gain, c[1].gamma, c[1].erase, c[1].fill) == tuple(s), i
        # the first and the last frame do not depend on T; the frames in between have draws of their own
        c5 = data.draw_clip(data.AUG_DEFAULT, 7, i % 3, i, 854, 480, 512, 384, 5)
        assert c5[0] == c[0] and c5[4] == c[1]
        assert len({tuple(f.gain) for f in c5}) == 5
        rects += sum(len(f.erase) > 0 for f in c5[1:4])
    assert 200 < rects < 400                                        # erase_prob = 0.5, three frames, 200 clips
    assert len(data.draw_clip(data.AUG_DEFAULT, 0, 0, 0, 70, 9, 48, 8, 1)) == 1


def test_every_map_of_a_clip_is_invertible_and_the_motion_is_steady():
    for i in range(1000):
        c = data.draw_clip(data.AUG_DEFAULT, 11, 0, i, 854, 480, 512, 384, 10)
        for f in c:
            a, b, _, d, e, _ = (float(v) for v in f.T)
            assert abs(a * e - b * d) > 1e-3
            opt.clip_frame(f)
        if i < 50:
            centre = lambda f: np.asarray(f.T, np.float64).reshape(2, 3) @ [255.5, 191.5, 1]
            steps = np.diff([centre(f) for f in c], axis=0)
            assert np.abs(steps - steps.mean(0)).max() < 0.05 * (1 + np.abs(steps).max())


def test_without_augmentation_every_frame_is_the_identity_crop():
    for i in range(20):
        c = data.draw_clip(data.AUG_NONE, 0, 0, i, 854, 480, 512, 384, 6)
        assert all(f.T == c[0].T and f.erase == () and list(f.gain) == [1, 1, 1] and f.gamma == 1 for f in c)
        a, b, tx, d, e, ty = c[0].T
        assert (a, b, d, e) == (1, 0, 0, 1) and 0 <= tx <= 854 - 512 and 0 <= ty <= 480 - 384


# ---- ClipLoader on the twin --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def five(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("five"))
    clip_ref.write_clip_tree(root, 5, W, H, steps=STEPS, P=7)
    ld = loader(root)
    ref = [[as_bytes(x) for x in ld.epoch(e)] for e in range(2)]
    ld.close()
    return root, ref


def test_loader_batches_are_a_function_of_seed_epoch_and_index(five):
    root, ref = five
    ld = loader(root, jobs=1)
    assert len(ld) == 3
    e0 = [as_bytes(x) for x in ld]
    e1 = [as_bytes(x) for x in ld]
    assert e0 == ref[0] and e1 == ref[1] and e0 != e1
    assert all(len(set(x[k] for x in e0)) == 3 for k in ("video", "flows", "tracks"))
    shapes = [{k: tuple(v.shape) for k, v in x.items()} for x in ld.epoch(0)]
    assert shapes[0] == dict(video=(2, T, 3, 8, 48), flows=(2, 4, 2, 8, 48), valid=(2, 4, 8, 48), tracks=(2, T, 7, 2), vis=(2, T, 7))
    assert shapes[2]["video"] == (1, T, 3, 8, 48) and shapes[2]["vis"] == (1, T, 7)            # the ragged last batch
    assert as_bytes(ld.batch_at(1, 2)) == ref[1][2] and as_bytes(ld.batch_at(0, 1)) == ref[0][1]
    assert [as_bytes(x) for x in loader(root, seed=2).epoch(0)] != ref[0]
    ld.close()


def test_loader_feeds_the_clips_it_names(tmp_path):
    """without augmentation and shuffling a batch is the files themselves"""
    made = clip_ref.write_clip_tree(str(tmp_path), 3, W, H, steps=STEPS, P=7)
    ld = loader(str(tmp_path), links=("first",), cfg=data.AUG_NONE, size=(W, H), shuffle=False, scale=(1, 1, 1), bias=(0, 0, 0), batch=3)
    (batch,) = list(ld.epoch(0))
    for i, m in enumerate(made):
        assert np.array_equal(np.asarray(batch["video"][i]), np.moveaxis(m["frames"], -1, 1).astype(F))
        assert np.array_equal(np.asarray(batch["tracks"][i]), m["pos"])
        assert np.array_equal(np.asarray(batch["vis"][i]), np.where((m["occ"] == 0) & trk.in_frame(m["pos"], W, H), 255, 0))
        bad = ~np.isfinite(m["first"]).all(-1)
        if i % 2 == 0:
            bad[0] |= m["occ_step"][0] != 0
            bad[3] |= m["occ_pair"] != 0
        assert np.array_equal(np.asarray(batch["valid"][i]), np.where(bad, 0, 255))
        assert np.array_equal(np.asarray(batch["flows"][i]), np.where(bad[:, None], F(0), np.moveaxis(m["first"], -1, 1)))
    ld.close()


def test_batch_at_between_the_steps_of_an_epoch(five):
    root, ref = five
    ld = loader(root)
    it = ld.epoch(0)
    for k in range(3):
        assert as_bytes(next(it)) == ref[0][k], k
        for e, j in ((0, (k + 1) % 3), (1, 2), (1, 0)):
            assert as_bytes(ld.batch_at(e, j)) == ref[e][j], (k, e, j)
    with pytest.raises(StopIteration):
        next(it)
    older = ld.epoch(1)
    ld.epoch(0)
    with pytest.raises(RuntimeError, match="ClipLoader"):
        next(older)
    ld.close()


def test_a_clip_of_another_length_is_an_error_that_leaves_the_loader_usable(five, tmp_path):
    root, ref = five
    mine = str(tmp_path / "tree")
    shutil.copytree(root, mine)
    cl = data.ClipList(mine)
    victim = int(loader(mine, shuffle=False).order(0)[2])                   # clip 2: batch 1
    os.remove(cl[victim].frames[2])                                          # one in-between frame less: T = 4
    prefix = cl[victim].frames[2][:-4]
    os.remove(prefix + ".flo")
    os.remove(prefix + "_step.flo")
    short = data.ClipList(mine, tracks=False)
    assert len(short[victim].frames) == T - 1 and len(short[0].frames) == T
    ld = data.ClipLoader(short, None, 2, (48, 8), seed=1, augment=clip_ref.as_augment, shuffle=False)
    it = ld.epoch(0)
    first = as_bytes(next(it))
    with pytest.raises(ValueError):
        next(it)
    with pytest.raises(ValueError):
        ld.batch_at(0, 1)
    assert as_bytes(ld.batch_at(0, 0)) == first and set(as_bytes(ld.batch_at(0, 2))) == {"video", "flows", "valid"}
    ld.close()


def test_the_batch_limit_follows_the_number_of_frames(five):
    root, _ = five
    with pytest.raises(ValueError):
        loader(root, batch=65)
    ld = loader(root, batch=256 // T + 1)                                   # 52 clips of 5 frames: one too many
    with pytest.raises(ValueError, match="256 // T"):
        next(ld.epoch(0))
    ld.close()
    ld = loader(root, batch=256 // T)
    assert len(list(ld.epoch(0))) == 1
    ld.close()
