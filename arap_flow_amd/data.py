"""From a generated dataset to training batches (DESIGN.md "Training batches").

  PairList        the pairs of OUT/all_files*.list with the planes that say where a pair has no ground truth
  draw_sample     one pair's augmentation, a pure function of (cfg, seed, epoch, index) and the sizes
  AugmentLoader   batches of augmented pairs: files decoded in a thread pool, stacked in pinned memory, uploaded, and
                  turned into img1 / img2 / flow / valid by one ArapFlow_AugmentPairs call per batch

The loader runs in the training process: only the calling process opens the GPU, there are no worker processes and
nothing forks.  torch is used for pinned memory, the upload and the stream; the arithmetic is the library's kernel.
"""
import collections
import concurrent.futures
import math
import os.path as osp

import numpy as np
import torch
from PIL import Image

from . import flo, opt

LISTS = {"": "all_files.list", "tex": "all_files_tex.list", "blur": "all_files_blur.list", "light": "all_files_light.list"}
# a plane's directory under OUT, and what of its picture means "no ground truth here"
PLANES = {"fold": "Fold", "mask": "inpMasks", "occ": "Occ"}
MAX_JOBS = 16

Pair = collections.namedtuple("Pair", "rgb1 rgb2 flow planes")


class PairList:
    """The pairs a list of a generated tree names: `rgb1 rgb2 flow` per line.  variant: "" (all_files.list), "tex",
    "blur" or "light", the twins that share the pair's flow.  planes: which of "fold" (OUT/Fold, non-zero: the flow is
    no valid correspondence), "mask" (OUT/inpMasks, red != 0: not an object, for the object-only flow of OUT/Flow) and
    "occ" (OUT/Occ, non-zero: occluded) are ORed into a pair's skip plane, each only where its file
    OUT/<dir>/<seq>/<frame>.png exists.  A file the list names under another root (the tree was moved) is looked up
    under `root` by its last three components."""

    def __init__(self, root, variant="", planes=("fold",)):
        if variant not in LISTS:
            raise ValueError("PairList: variant: one of %s" % ", ".join(repr(v) for v in LISTS))
        planes = tuple(planes)
        if set(planes) - set(PLANES):
            raise ValueError("PairList: planes: some of %s" % ", ".join(PLANES))
        self.root, self.variant, self.plane_names = root, variant, planes
        lst = osp.join(root, LISTS[variant])
        self.pairs = []
        for ln in open(lst).read().splitlines():
            if not ln.strip():
                continue
            names = ln.split(" ")
            if len(names) != 3:
                raise ValueError("%s: `rgb1 rgb2 flow` expected, got %r" % (lst, ln))
            rgb1, rgb2, flow = (self._find(p) for p in names)
            seq, stem = osp.basename(osp.dirname(flow)), osp.basename(flow)[:-4]
            named = {k: osp.join(root, PLANES[k], seq, stem + ".png") for k in planes}
            self.pairs.append(Pair(rgb1, rgb2, flow, {k: p for k, p in named.items() if osp.exists(p)}))

    def _find(self, path):
        if osp.exists(path):
            return path
        return osp.join(self.root, *path.replace("\\", "/").split("/")[-3:])

    def __len__(self):
        return len(self.pairs)

    def __getitem__(self, i):
        return self.pairs[i]

    def load(self, i):
        """-> (rgb1 u8[H,W,3], rgb2 u8[H,W,3], flow f32[H,W,2], skip u8[H,W] (0 / 255) or None when the pair has no plane)"""
        p = self.pairs[i]
        rgb1, rgb2 = (np.asarray(Image.open(f).convert("RGB")) for f in (p.rgb1, p.rgb2))
        flow = flo.flow_read(p.flow)
        if rgb1.shape != rgb2.shape or flow.shape[:2] != rgb1.shape[:2]:
            raise ValueError("pair %d (%s): frames and flow of one size expected" % (i, p.flow))
        skip = None
        for k, f in p.planes.items():
            a = np.asarray(Image.open(f).convert("RGB")) if k == "mask" else np.asarray(Image.open(f))
            if a.shape[:2] != flow.shape[:2]:
                raise ValueError("pair %d: %s of the flow's size expected" % (i, f))
            hit = a[..., 0] != 0 if k == "mask" else a.reshape(a.shape[0], a.shape[1], -1).any(-1)
            skip = hit if skip is None else skip | hit
        return rgb1, rgb2, flow, None if skip is None else np.where(skip, 255, 0).astype(np.uint8)


# The ranges of an augmentation.  Angles in radians, scales as log2, shifts in output pixels, sizes in output pixels.
#   zoom          (lo, hi): the source is shown 2^z times larger, z uniform
#   stretch       |log2| of the extra zoom in x against y, uniform, applied with probability stretch_prob
#   rotate        |angle|, uniform
#   flip_h, flip_v   probabilities
#   rel_zoom, rel_rotate, rel_shift   frame 2 against frame 1: |log2 zoom|, |angle|, |shift| per axis, uniform
#   gain, gamma   |log2| of the part both frames share;  gain_rel, gamma_rel: of the part each frame has of its own;
#   chan          |log2| of a channel's own gain, per frame
#   erase_prob    probability that frame 2 gets rectangles at all; then 1 .. erase_max of them (at most 4), each side
#                 uniform in erase_size = (lo, hi), anywhere with its corner in the crop
#   fill          (lo, hi): a rectangle's colour per channel, uniform, in the units of the output
AugConfig = collections.namedtuple("AugConfig", "zoom stretch stretch_prob rotate flip_h flip_v rel_zoom rel_rotate rel_shift "
                                   "gain gain_rel chan gamma gamma_rel erase_prob erase_max erase_size fill")
AUG_DEFAULT = AugConfig(zoom=(-0.2, 0.5), stretch=0.2, stretch_prob=0.8, rotate=0.3, flip_h=0.5, flip_v=0.1, rel_zoom=0.03,
                        rel_rotate=0.02, rel_shift=2.0, gain=0.3, gain_rel=0.05, chan=0.05, gamma=0.3, gamma_rel=0.05,
                        erase_prob=0.5, erase_max=2, erase_size=(50, 100), fill=(0.0, 255.0))
AUG_NONE = AugConfig(zoom=(0.0, 0.0), stretch=0.0, stretch_prob=0.0, rotate=0.0, flip_h=0.0, flip_v=0.0, rel_zoom=0.0, rel_rotate=0.0,
                     rel_shift=0.0, gain=0.0, gain_rel=0.0, chan=0.0, gamma=0.0, gamma_rel=0.0, erase_prob=0.0, erase_max=0,
                     erase_size=(1, 1), fill=(0.0, 0.0))


def _about(M, cx, cy, ox, oy):
    """the 3x3 map x -> M (x - (ox, oy)) + (cx, cy), M 2x2"""
    A = np.eye(3)
    A[:2, :2] = M
    A[:2, 2] = np.asarray([cx, cy]) - M @ np.asarray([ox, oy])
    return A


def _rot(angle):
    c, s = math.cos(angle), math.sin(angle)
    return np.asarray([[c, -s], [s, c]])


def draw_sample(cfg, seed, epoch, index, W, H, w, h):
    """The augmentation of pair `index` in epoch `epoch`: an opt.AugSample, a pure function of its arguments through
    np.random.default_rng([seed, epoch, index]).  Frame 1: a zoom with a stretch, a rotation and flips about the crop's
    centre, which shows a source point drawn so that the crop stays inside the W x H source where the zoom allows (the
    source's centre on an axis where it does not).  Frame 2: the same after a small zoom, rotation and shift of its own
    about the crop's centre (T2 = T1 o D).  Composed in double; every number is rounded once to float32."""
    rng = np.random.default_rng([int(seed), int(epoch), int(index)])
    u = lambda r: rng.uniform(-r, r) if r > 0 else 0.0 * rng.uniform()          # (one draw either way: the stream keeps its shape)
    z = rng.uniform(cfg.zoom[0], cfg.zoom[1])
    st = u(cfg.stretch) if rng.uniform() < cfg.stretch_prob else 0.0 * rng.uniform()
    angle = u(cfg.rotate)
    fh, fv = rng.uniform() < cfg.flip_h, rng.uniform() < cfg.flip_v
    # output -> source: undo the zoom (so divide), then rotate
    M = _rot(angle) @ np.diag([(-1.0 if fh else 1.0) * 2.0 ** -(z + st / 2), (-1.0 if fv else 1.0) * 2.0 ** -(z - st / 2)])
    ox, oy = (w - 1) / 2.0, (h - 1) / 2.0
    ex, ey = abs(M[0, 0]) * ox + abs(M[0, 1]) * oy, abs(M[1, 0]) * ox + abs(M[1, 1]) * oy     # half the crop's footprint
    r = rng.uniform(size=2)
    cx = ex + r[0] * (W - 1 - 2 * ex) if 2 * ex <= W - 1 else (W - 1) / 2.0
    cy = ey + r[1] * (H - 1 - 2 * ey) if 2 * ey <= H - 1 else (H - 1) / 2.0
    A1 = _about(M, cx, cy, ox, oy)
    D = _about(_rot(u(cfg.rel_rotate)) * 2.0 ** u(cfg.rel_zoom), ox + u(cfg.rel_shift), oy + u(cfg.rel_shift), ox, oy)
    A2 = A1 @ D
    shared_gain, shared_gamma = u(cfg.gain), u(cfg.gamma)
    tone = []
    for _ in range(2):
        own = u(cfg.gain_rel)
        tone.append(([2.0 ** (shared_gain + own + u(cfg.chan)) for _ in range(3)], 2.0 ** (shared_gamma + u(cfg.gamma_rel))))
    rects = []
    n = int(rng.integers(1, max(1, min(int(cfg.erase_max), 4)) + 1))
    gate = rng.uniform()
    for i in range(4):                                                          # (always four draws)
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        dx, dy = (int(v) for v in rng.integers(cfg.erase_size[0], cfg.erase_size[1] + 1, size=2))
        if gate < cfg.erase_prob and cfg.erase_max > 0 and i < n:
            rects.append((x0, y0, x0 + dx, y0 + dy))
    fill = rng.uniform(cfg.fill[0], cfg.fill[1], size=3)
    f32 = lambda v: [float(np.float32(x)) for x in v]
    return opt.AugSample(f32(A1[:2].reshape(6)), f32(A2[:2].reshape(6)), f32(tone[0][0]), f32([tone[0][1]])[0], f32(tone[1][0]),
                         f32([tone[1][1]])[0], tuple(rects), f32(fill))


class AugmentLoader:
    """Batches of augmented pairs.  pairs: a PairList (anything with len() and load(i)), all of one source size; state:
    the opt.State whose stream the batches are made on, or None for an `augment` that runs on the host (the numpy twin
    of the tests: nothing is uploaded); batch: pairs per batch, at most 64; size = (w, h), the crop; cfg: an AugConfig;
    jobs: decoding threads, at most 16 (never sized by the machine's core count).

    Batch k of epoch e is a pure function of (seed, e, k): the epoch's order is a permutation drawn from (seed, e), a
    pair's augmentation is draw_sample(cfg, seed, e, its index in the list).  epoch(e) iterates over one epoch; iter()
    over the next one (0, 1, ..).  A batch is a dict(img1, img2, flow, valid) of what `augment` returns: CUDA tensors of
    the current device, ready on torch's current stream.  While the caller works on a batch the files of the next one
    are decoded.  The last batch of an epoch is shorter when the list's length is no multiple of `batch`.

    Who owns the staging buffers.  There are three sets.  Two belong to the epoch in progress, which fills one while the
    other is uploaded; the third belongs to batch_at.  epoch(e) (and iter()) takes the two over at the call: the loader
    has one epoch in progress, the one asked for last.  An older iterator raises RuntimeError at its next step and
    never yields a batch of anybody else's pixels; one that was simply abandoned costs nothing.  batch_at may be
    called at any time, also between two next() of an epoch, and does not disturb it.  Nobody decodes into a set before
    the jobs last started on it have ended and its last upload has been read, whoever started them.  One thread calls
    the loader.

    Streams.  Every batch is made on the stream that is torch's current one when it is asked for (next() or batch_at),
    and the loader moves the state there.  The state has a single device table of samples, which a call overwrites, so
    a batch asked for under another stream than the batch before it makes its stream wait for that batch's call first;
    batches of one stream are ordered by the stream.  The loader orders only its own calls: whoever else calls
    augment_pairs on the loader's state from another stream has to order those calls against the loader's."""
    ALONE = 2                                   # batch_at's buffer set

    def __init__(self, pairs, state, batch, size, cfg=AUG_DEFAULT, seed=0, jobs=8, augment=opt.augment_pairs, scale=(1, 1, 1),
                 bias=(0, 0, 0), tau=1.0, shuffle=True):
        if not 1 <= int(batch) <= 64 or len(pairs) == 0:
            raise ValueError("AugmentLoader: 1 .. 64 pairs a batch of a list that is not empty expected")
        self.pairs, self.state, self.batch, self.size, self.cfg, self.seed = pairs, state, int(batch), tuple(size), cfg, int(seed)
        self.augment, self.scale, self.bias, self.tau, self.shuffle = augment, tuple(scale), tuple(bias), float(tau), shuffle
        self.jobs = max(1, min(int(jobs), MAX_JOBS))
        self.pool = concurrent.futures.ThreadPoolExecutor(self.jobs)
        self.next_epoch = 0
        self.source = None                      # (W, H), known from the first pair decoded
        self.generation = 0                     # of the epoch that owns the sets 0 and 1
        self.sets = [None, None, None]          # host buffers: 0 and 1 of the epoch in progress, ALONE of batch_at
        self.uploaded = [None, None, None]      # the event behind a set's last upload
        self.filling = [(), (), ()]             # the decoding jobs last started on a set (an abandoned epoch may leave some)
        self.called = None                      # (stream, event) of the last call made on the state

    def __len__(self):
        return (len(self.pairs) + self.batch - 1) // self.batch

    def __iter__(self):
        e = self.next_epoch
        self.next_epoch += 1
        return self.epoch(e)

    def close(self):
        self.pool.shutdown(wait=True)

    def order(self, epoch):
        n = len(self.pairs)
        return np.random.default_rng([self.seed, int(epoch)]).permutation(n) if self.shuffle else np.arange(n)

    def _buffers(self, which):
        if self.sets[which] is None:
            W, H = self.source
            pin = self.state is not None
            new = lambda shape, dt: torch.empty((self.batch,) + shape, dtype=dt, pin_memory=pin)
            self.sets[which] = dict(rgb1=new((H, W, 3), torch.uint8), rgb2=new((H, W, 3), torch.uint8),
                                    flow=new((H, W, 2), torch.float32), skip=new((H, W), torch.uint8))
        return self.sets[which]

    def _decode_into(self, bufs, slot, index):
        rgb1, rgb2, flow, skip = self.pairs.load(index)
        if (rgb1.shape[1], rgb1.shape[0]) != self.source:
            raise ValueError("AugmentLoader: pair %d is %dx%d, the first one %dx%d" % ((index, rgb1.shape[1], rgb1.shape[0]) + self.source))
        bufs["rgb1"][slot].numpy()[...] = rgb1
        bufs["rgb2"][slot].numpy()[...] = rgb2
        bufs["flow"][slot].numpy()[...] = flow
        bufs["skip"][slot].numpy()[...] = 0 if skip is None else skip

    def _start(self, order, k, which):
        """the decoding of batch k into the buffer set `which` -> (indices, futures)"""
        idx = [int(i) for i in order[k * self.batch:(k + 1) * self.batch]]
        if self.source is None:
            first = self.pairs.load(idx[0])[0]
            self.source = (first.shape[1], first.shape[0])
        if self.uploaded[which] is not None:
            self.uploaded[which].synchronize()              # the set's last upload has read it
            self.uploaded[which] = None
        concurrent.futures.wait(self.filling[which])         # (and nobody's job still writes it)
        bufs = self._buffers(which)
        self.filling[which] = [self.pool.submit(self._decode_into, bufs, slot, i) for slot, i in enumerate(idx)]
        return idx, self.filling[which]

    def _make(self, epoch, idx, futures, which):
        for f in futures:
            f.result()
        B, bufs = len(idx), self.sets[which]
        ins = {name: t[:B] for name, t in bufs.items()}
        if self.state is not None:
            stream = torch.cuda.current_stream()
            ins = {name: t.cuda(non_blocking=True) for name, t in ins.items()}
            self.uploaded[which] = torch.cuda.Event()
            self.uploaded[which].record()
            if self.called is not None and self.called[0] != stream:
                stream.wait_event(self.called[1])           # the state has one sample table, which the last call's kernel reads
            self.state.set_stream(stream)
        W, H = self.source
        samples = [draw_sample(self.cfg, self.seed, epoch, i, W, H, *self.size) for i in idx]
        out = self.augment(self.state, ins["rgb1"], ins["rgb2"], ins["flow"], samples, self.size, skip=ins["skip"],
                           scale=self.scale, bias=self.bias, tau=self.tau)
        if self.state is not None:
            self.called = (stream, torch.cuda.Event())
            self.called[1].record()
        return out

    def epoch(self, epoch):
        """an iterator over the batches of one epoch, which becomes the loader's epoch in progress at this call"""
        self.generation += 1
        return self._epoch(epoch, self.generation)

    def _epoch(self, epoch, generation):
        order, n = self.order(epoch), len(self)
        pending = None
        for k in range(n):
            if generation != self.generation:               # checked after every yield, before a shared set is touched
                raise RuntimeError("AugmentLoader: epoch %d was replaced by a later epoch() of this loader" % epoch)
            idx, futures = pending or self._start(order, k, k % 2)
            concurrent.futures.wait(futures)
            pending = self._start(order, k + 1, (k + 1) % 2) if k + 1 < n else None
            yield self._make(epoch, idx, futures, k % 2)

    def batch_at(self, epoch, k):
        """batch k of an epoch on its own (nothing is decoded ahead), in a buffer set that no epoch uses"""
        if not 0 <= k < len(self):
            raise IndexError(k)
        idx, futures = self._start(self.order(epoch), k, self.ALONE)
        return self._make(epoch, idx, futures, self.ALONE)
