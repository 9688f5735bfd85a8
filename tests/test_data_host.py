"""CPU-only: from a generated tree to training batches (arap_flow_amd/data.py, DESIGN.md "Training batches").  PairList on
a tree written here: the four lists, missing planes, the OR into one skip plane, a moved tree; draw_sample: a pure function
within its configuration's ranges whose frame-2 map always inverts; AugmentLoader on the numpy twin: the same bytes for the
same (seed, epoch, k), other bytes for another epoch, the ragged last batch; who owns the loader's buffer sets: batch_at between the
steps of an epoch, two epochs at once, an abandoned epoch, a pair of another size, one and sixteen decoding threads."""
import math

import numpy as np
import pytest

import aug_ref
from arap_flow_amd import data, opt

F = np.float32
W, H = 70, 9


# ---- PairList -----------------------------------------------------------------------------------------------------------
def test_pair_list_reads_all_four_lists(tmp_path):
    made = aug_ref.write_tree(str(tmp_path), 3, W, H, variants=("", "tex", "blur", "light"), planes=())
    for v in ("", "tex", "blur", "light"):
        pl = data.PairList(str(tmp_path), variant=v)
        assert len(pl) == 3
        for i, m in enumerate(made):
            rgb1, rgb2, flow, skip = pl.load(i)
            assert np.array_equal(rgb1, m["rgb1"][v]) and np.array_equal(rgb2, m["rgb2"][v]) and skip is None
            assert flow.tobytes() == m["flow"].tobytes()                  # the twins share the pair's flow file
            assert pl[i].flow.endswith("Flow/seq%d/%05d.flo" % (i % 2, i)) and pl[i].planes == {}
    with pytest.raises(ValueError):
        data.PairList(str(tmp_path), variant="ext")
    with pytest.raises(ValueError):
        data.PairList(str(tmp_path), planes=("dist",))
    with pytest.raises(OSError):
        data.PairList(str(tmp_path / "nowhere"))


def test_planes_are_ored_where_they_exist(tmp_path):
    made = aug_ref.write_tree(str(tmp_path), 4, W, H, planes=("fold", "mask", "occ"))
    want = {"fold": lambda m: m["fold"] != 0, "mask": lambda m: m["mask"][..., 0] != 0, "occ": lambda m: m["occ"] != 0}
    for planes in (("fold",), ("mask",), ("occ",), ("fold", "occ"), ("fold", "mask", "occ")):
        pl = data.PairList(str(tmp_path), planes=planes)
        for i, m in enumerate(made):
            skip = pl.load(i)[3]
            if i % 2:                                                     # the odd pairs have no plane at all
                assert skip is None and pl[i].planes == {}
                continue
            assert sorted(pl[i].planes) == sorted(planes)
            hit = np.zeros((H, W), bool)
            for k in planes:
                hit |= want[k](m)
            assert skip.dtype == np.uint8 and np.array_equal(skip, np.where(hit, 255, 0)) and 0 < hit.sum() < hit.size
    assert data.PairList(str(tmp_path), planes=()).load(0)[3] is None


def test_a_moved_tree_is_found_under_its_new_root(tmp_path):
    made = aug_ref.write_tree(str(tmp_path), 2, W, H, named_root="/somewhere/else/OUT")
    pl = data.PairList(str(tmp_path))
    rgb1, rgb2, flow, skip = pl.load(0)
    assert np.array_equal(rgb1, made[0]["rgb1"][""]) and np.array_equal(skip, made[0]["fold"])
    assert pl[1].rgb2 == str(tmp_path / "wRGB" / "seq1" / "00001.png")


# ---- draw_sample --------------------------------------------------------------------------------------------------------
def linear(T):
    return np.asarray(T, np.float64).reshape(2, 3)[:, :2]


def test_draw_sample_is_a_pure_function():
    cfg = data.AUG_DEFAULT
    a = data.draw_sample(cfg, 3, 1, 17, 854, 480, 768, 384)
    assert a == data.draw_sample(cfg, 3, 1, 17, 854, 480, 768, 384)
    others = [data.draw_sample(cfg, 4, 1, 17, 854, 480, 768, 384), data.draw_sample(cfg, 3, 2, 17, 854, 480, 768, 384),
              data.draw_sample(cfg, 3, 1, 18, 854, 480, 768, 384)]
    assert all(o != a and o.T1 != a.T1 and o.gamma2 != a.gamma2 for o in others)
    for v in list(a.T1) + list(a.T2) + list(a.gain1) + [a.gamma1, a.gamma2] + list(a.fill):
        assert isinstance(v, float) and v == float(F(v))                   # rounded once, to float32
    ident = data.draw_sample(data.AUG_NONE, 0, 0, 0, 70, 9, 70, 9)
    assert ident == opt.AUG_NEUTRAL._replace(T1=[1, 0, 0, 0, 1, 0], T2=[1, 0, 0, 0, 1, 0], gain1=[1, 1, 1], gain2=[1, 1, 1], fill=[0, 0, 0])


def test_draw_sample_stays_within_its_ranges():
    cfg = data.AUG_DEFAULT._replace(erase_max=4, erase_prob=0.7)
    Ws, Hs, w, h = 854, 480, 384, 256
    eps = 1e-5
    seen = dict(flip_h=0, flip_v=0, rects=set(), inside=0)
    N = 3000
    for i in range(N):
        s = data.draw_sample(cfg, 5, i // 1000, i % 1000, Ws, Hs, w, h)
        L1, L2 = linear(s.T1), linear(s.T2)
        assert abs(np.linalg.det(L2)) > 1e-3 and abs(np.linalg.det(L1)) > 1e-3
        sv = np.linalg.svd(L1, compute_uv=False)
        lo, hi = 2.0 ** -(cfg.zoom[1] + cfg.stretch / 2), 2.0 ** -(cfg.zoom[0] - cfg.stretch / 2)
        assert lo * (1 - eps) <= sv.min() and sv.max() <= hi * (1 + eps)
        seen["flip_h"] += np.linalg.det(L1) < 0
        # frame 2 against frame 1: D = T1^-1 o T2 is a similarity close to the identity
        A1, A2 = np.eye(3), np.eye(3)
        A1[:2], A2[:2] = np.asarray(s.T1, np.float64).reshape(2, 3), np.asarray(s.T2, np.float64).reshape(2, 3)
        D = np.linalg.inv(A1) @ A2
        zoom = math.sqrt(abs(np.linalg.det(D[:2, :2])))
        assert abs(math.log2(zoom)) <= cfg.rel_zoom + 1e-4
        assert abs(math.atan2(D[1, 0], D[0, 0])) <= cfg.rel_rotate + 1e-4
        centre = np.asarray([(w - 1) / 2, (h - 1) / 2, 1.0])
        assert (np.abs((D @ centre)[:2] - centre[:2]) <= cfg.rel_shift + 1e-2).all()
        # the crop's corners lie inside the source (the zoom of this configuration always allows it)
        corners = np.asarray([[0, 0, 1], [w - 1, 0, 1], [0, h - 1, 1], [w - 1, h - 1, 1.0]]).T
        q = A1[:2] @ corners
        assert (q[0] >= -1e-2).all() and (q[0] <= Ws - 1 + 1e-2).all() and (q[1] >= -1e-2).all() and (q[1] <= Hs - 1 + 1e-2).all()
        g = cfg.gain + cfg.gain_rel + cfg.chan
        for gain, gamma in ((s.gain1, s.gamma1), (s.gain2, s.gamma2)):
            assert all(2.0 ** -g * (1 - eps) <= v <= 2.0 ** g * (1 + eps) for v in gain)
            assert 2.0 ** -(cfg.gamma + cfg.gamma_rel) * (1 - eps) <= gamma <= 2.0 ** (cfg.gamma + cfg.gamma_rel) * (1 + eps)
        assert abs(math.log2(s.gamma1 / s.gamma2)) <= 2 * cfg.gamma_rel + 1e-4
        assert len(s.erase) <= 4
        seen["rects"].add(len(s.erase))
        for x0, y0, x1, y1 in s.erase:
            assert 0 <= x0 < w and 0 <= y0 < h and cfg.erase_size[0] <= x1 - x0 <= cfg.erase_size[1] and cfg.erase_size[0] <= y1 - y0 <= cfg.erase_size[1]
        assert all(cfg.fill[0] <= v <= cfg.fill[1] for v in s.fill)
        opt.aug_sample(s)
    assert seen["rects"] == {0, 1, 2, 3, 4} and 0.4 * N < seen["flip_h"] < 0.6 * N
    # a zoom that does not allow it: the crop is centred on the source
    s = data.draw_sample(data.AUG_NONE, 0, 0, 0, 20, 30, 40, 10)
    assert s.T1[:2] == [1, 0] and s.T1[3:5] == [0, 1] and s.T1[2] == -10 and 0 <= s.T1[5] <= 20


def test_the_library_accepts_every_draw():
    from arap_flow_amd import build, capi
    build.build()
    lib = capi.load()
    for i in range(300):
        s = data.draw_sample(data.AUG_DEFAULT, 9, 0, i, 70, 9, 48, 8)
        P2, _ = opt.augment_tables(s, lib=lib)
        assert np.isfinite(P2).all()


# ---- AugmentLoader on the twin ------------------------------------------------------------------------------------------
CFG = data.AUG_DEFAULT._replace(erase_size=(3, 12), erase_max=4)


def loader(root, **kw):
    args = dict(batch=3, size=(48, 8), cfg=CFG, seed=1, jobs=4, augment=aug_ref.as_augment, scale=(1 / 64, 1 / 64, 1 / 64), bias=(-2, -2, -2))
    args.update(kw)
    return data.AugmentLoader(data.PairList(root, planes=("fold",)), None, **args)


def as_bytes(batch):
    assert sorted(batch) == ["flow", "img1", "img2", "valid"]
    return {k: np.asarray(v).tobytes() for k, v in batch.items()}


def test_loader_batches_are_a_function_of_seed_epoch_and_index(tmp_path):
    aug_ref.write_tree(str(tmp_path), 7, W, H)
    a, b = loader(str(tmp_path)), loader(str(tmp_path), jobs=1)
    assert len(a) == 3 and a.jobs == 4 and loader(str(tmp_path), jobs=400).jobs == 16
    e0 = [as_bytes(x) for x in a.epoch(0)]
    e1 = [as_bytes(x) for x in a]                    # iter(): epoch 0 again, then 1
    e2 = [as_bytes(x) for x in a]
    assert e0 == e1 and e0 != e2 and len(e0) == 3
    assert [as_bytes(x) for x in b.epoch(1)] == e2 and as_bytes(b.batch_at(1, 2)) == e2[2] and as_bytes(b.batch_at(0, 1)) == e0[1]
    assert all(len(set(x[k] for x in e0)) == 3 for k in ("img1", "img2", "flow"))
    other = [as_bytes(x) for x in loader(str(tmp_path), seed=2).epoch(0)]
    assert other != e0
    shapes = [{k: tuple(v.shape) for k, v in x.items()} for x in b.epoch(0)]
    assert [s["img1"] for s in shapes] == [(3, 3, 8, 48), (3, 3, 8, 48), (1, 3, 8, 48)]          # the ragged last batch
    assert shapes[2] == dict(img1=(1, 3, 8, 48), img2=(1, 3, 8, 48), flow=(1, 2, 8, 48), valid=(1, 8, 48))
    assert sorted(int(i) for i in a.order(0)) == list(range(7)) and list(a.order(0)) != list(a.order(1))
    a.close()
    b.close()


def test_loader_feeds_the_pairs_it_names(tmp_path):
    """without augmentation and shuffling a batch is the files themselves"""
    made = aug_ref.write_tree(str(tmp_path), 4, W, H)
    ld = loader(str(tmp_path), cfg=data.AUG_NONE, size=(W, H), shuffle=False, scale=(1, 1, 1), bias=(0, 0, 0), batch=4)
    (batch,) = list(ld.epoch(0))
    for i, m in enumerate(made):
        assert np.array_equal(np.asarray(batch["img1"][i]), np.moveaxis(m["rgb1"][""], -1, 0).astype(F))
        assert np.array_equal(np.asarray(batch["img2"][i]), np.moveaxis(m["rgb2"][""], -1, 0).astype(F))
        bad = ~np.isfinite(m["flow"]).all(-1) | ((m["fold"] != 0) if i % 2 == 0 else False)
        assert np.array_equal(np.asarray(batch["valid"][i]), np.where(bad, 0, 255))
        assert np.array_equal(np.asarray(batch["flow"][i]), np.where(bad[None], F(0), np.moveaxis(m["flow"], -1, 0)))
    ld.close()
    with pytest.raises(ValueError):
        loader(str(tmp_path), batch=65)


# ---- who owns the buffer sets -------------------------------------------------------------------------------------------
# nine pairs, two a batch: five batches, the last one ragged, every shared set used more than once
@pytest.fixture(scope="module")
def nine(tmp_path_factory):
    """(root, the bytes of the epochs 0 and 1 from a loader that nothing disturbs)"""
    root = str(tmp_path_factory.mktemp("nine"))
    aug_ref.write_tree(root, 9, W, H)
    ld = loader(root, batch=2)
    ref = [[as_bytes(x) for x in ld.epoch(e)] for e in range(2)]
    ld.close()
    assert [len(r) for r in ref] == [5, 5] and all(len(set(x[k] for r in ref for x in r)) == 10 for k in ("img1", "img2", "flow"))
    return root, ref


def test_batch_at_between_the_steps_of_an_epoch(nine):
    """after every next() of epoch 0, an even and an odd batch of either epoch on their own: every batch of the epoch and
    every batch_at equals the undisturbed loader's"""
    root, ref = nine
    ld = loader(root, batch=2)
    it = ld.epoch(0)
    for k in range(5):
        assert as_bytes(next(it)) == ref[0][k], k
        for e, j in ((0, (k + 2) % 5 // 2 * 2), (0, 3), (1, 4), (1, 1)):
            assert as_bytes(ld.batch_at(e, j)) == ref[e][j], (k, e, j)
    with pytest.raises(StopIteration):
        next(it)
    ld.close()


def test_two_epochs_at_once_the_older_one_raises(nine):
    """epoch() takes the shared sets over: the iterator asked for last yields the undisturbed batches, the older one raises
    at its next step, whether it had begun or not, and never yields another batch"""
    root, ref = nine
    ld = loader(root, batch=2)
    i0, i1 = ld.epoch(0), ld.epoch(1)
    for k in range(5):
        assert as_bytes(next(i1)) == ref[1][k], k
        if k < 2:
            with pytest.raises(RuntimeError if k == 0 else StopIteration):     # (a generator that raised has ended)
                next(i0)
    begun = ld.epoch(0)
    assert as_bytes(next(begun)) == ref[0][0] and as_bytes(next(begun)) == ref[0][1]
    later = iter(ld)                                                           # epoch 0, by iter()'s count
    assert as_bytes(next(later)) == ref[0][0]
    with pytest.raises(RuntimeError):
        next(begun)
    assert [as_bytes(x) for x in later] == ref[0][1:]
    ld.close()


def test_an_abandoned_epoch_costs_nothing(nine):
    root, ref = nine
    ld = loader(root, batch=2)
    it = ld.epoch(1)
    assert as_bytes(next(it)) == ref[1][0] and as_bytes(next(it)) == ref[1][1]      # batch 2 is being decoded into set 0
    del it
    assert [as_bytes(x) for x in ld.epoch(0)] == ref[0]
    assert as_bytes(ld.batch_at(1, 3)) == ref[1][3] and as_bytes(ld.batch_at(0, 4)) == ref[0][4]
    ld.close()


def test_a_pair_of_another_size_is_an_error_that_leaves_the_loader_usable(tmp_path):
    from PIL import Image
    from arap_flow_amd import flo
    root = str(tmp_path)
    aug_ref.write_tree(root, 9, W, H)
    ld = loader(root, batch=2, shuffle=False)
    ref = [as_bytes(x) for x in ld.epoch(0)]
    ld.close()
    pl = data.PairList(root, planes=("fold",))
    rng = np.random.default_rng(5)
    for f in (pl[5].rgb1, pl[5].rgb2):                                         # pair 5 (batch 2) becomes 71 x 9
        Image.fromarray(rng.integers(0, 256, (H, W + 1, 3)).astype(np.uint8)).save(f)
    flo.flow_write(pl[5].flow, np.zeros((H, W + 1, 2), F))
    ld = loader(root, batch=2, shuffle=False)
    it = ld.epoch(0)
    assert as_bytes(next(it)) == ref[0] and as_bytes(next(it)) == ref[1]
    with pytest.raises(ValueError):
        next(it)
    with pytest.raises(StopIteration):
        next(it)
    assert as_bytes(ld.batch_at(0, 3)) == ref[3]
    with pytest.raises(ValueError):
        ld.batch_at(0, 2)
    assert as_bytes(ld.batch_at(0, 4)) == ref[4] and as_bytes(ld.batch_at(0, 1)) == ref[1]
    it = ld.epoch(0)
    assert as_bytes(next(it)) == ref[0]
    ld.close()                                                                 # with batch 1 decoded ahead: returns


def test_one_and_sixteen_decoding_threads_give_the_same_bytes(nine):
    root, ref = nine
    for jobs in (1, 16):
        ld = loader(root, batch=2, jobs=jobs)
        assert ld.jobs == jobs and [[as_bytes(x) for x in ld.epoch(e)] for e in range(2)] == ref
        assert as_bytes(ld.batch_at(1, 2)) == ref[1][2]
        ld.close()
