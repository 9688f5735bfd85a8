"""From a generated dataset to training batches (DESIGN.md "Training batches").

  PairList        the pairs of OUT/all_files*.list with the planes that say where a pair has no ground truth
  draw_sample     one pair's augmentation, a pure function of (cfg, seed, epoch, index) and the sizes
  AugmentLoader   batches of augmented pairs: files decoded in a thread pool, stacked in pinned memory, uploaded, and
                  turned into img1 / img2 / flow / valid by one ArapFlow_AugmentPairs call per batch
  ClipList        the clips of a --mid K --tracks P tree: T frames, the flows of their links, point tracks
  draw_clip       one clip's augmentation: draw_sample's two frames and a steady motion between them
  ClipLoader      AugmentLoader over clips: video / flows / valid / tracks / vis by one ArapFlow_AugmentClips call per
                  batch (DESIGN.md "Training clips")

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
    d = _draw_pair(cfg, seed, epoch, index, W, H, w, h)
    f32 = lambda v: [float(np.float32(x)) for x in v]
    A2 = d["A1"] @ _rel_motion(d, 1.0, w, h)
    tone = d["tone"]
    return opt.AugSample(f32(d["A1"][:2].reshape(6)), f32(A2[:2].reshape(6)), f32(tone[0][0]), f32([tone[0][1]])[0], f32(tone[1][0]),
                         f32([tone[1][1]])[0], d["rects"], f32(d["fill"]))


def _uniform(rng):
    """u(r): uniform in (-r, r), one draw either way (the stream keeps its shape)"""
    return lambda r: rng.uniform(-r, r) if r > 0 else 0.0 * rng.uniform()


def _draw_erase(rng, cfg, w, h):
    """the cfg's eraser rule -> (rectangles, fill): always the same number of draws"""
    rects = []
    n = int(rng.integers(1, max(1, min(int(cfg.erase_max), 4)) + 1))
    gate = rng.uniform()
    for i in range(4):                                                          # (always four draws)
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        dx, dy = (int(v) for v in rng.integers(cfg.erase_size[0], cfg.erase_size[1] + 1, size=2))
        if gate < cfg.erase_prob and cfg.erase_max > 0 and i < n:
            rects.append((x0, y0, x0 + dx, y0 + dy))
    return tuple(rects), rng.uniform(cfg.fill[0], cfg.fill[1], size=3)


def _rel_motion(d, s, w, h):
    """D(s): frame 2's own zoom, rotation and shift about the crop's centre, each scaled by s (D(1) = D)"""
    ox, oy = (w - 1) / 2.0, (h - 1) / 2.0
    return _about(_rot(s * d["rel_rotate"]) * 2.0 ** (s * d["rel_zoom"]), ox + s * d["rel_shift"][0], oy + s * d["rel_shift"][1], ox, oy)


def _draw_pair(cfg, seed, epoch, index, W, H, w, h):
    """draw_sample's draws from default_rng([seed, epoch, index]), in its order, as doubles: A1 (3x3), the parts of D,
    the shared tone, the two frames' tones, frame 2's rectangles and fill"""
    rng = np.random.default_rng([int(seed), int(epoch), int(index)])
    u = _uniform(rng)
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
    rel_rotate, rel_zoom = u(cfg.rel_rotate), u(cfg.rel_zoom)
    rel_shift = (u(cfg.rel_shift), u(cfg.rel_shift))
    shared_gain, shared_gamma = u(cfg.gain), u(cfg.gamma)
    tone = []
    for _ in range(2):
        own = u(cfg.gain_rel)
        tone.append(([2.0 ** (shared_gain + own + u(cfg.chan)) for _ in range(3)], 2.0 ** (shared_gamma + u(cfg.gamma_rel))))
    rects, fill = _draw_erase(rng, cfg, w, h)
    return dict(A1=A1, rel_rotate=rel_rotate, rel_zoom=rel_zoom, rel_shift=rel_shift, shared_gain=shared_gain, shared_gamma=shared_gamma,
                tone=tone, rects=rects, fill=fill)


def draw_clip(cfg, seed, epoch, index, W, H, w, h, T):
    """The augmentation of clip `index` in epoch `epoch`: T opt.ClipFrame, a pure function of its arguments.  Frames 0 and
    T - 1 are draw_sample's frame 1 and frame 2 (the same generator, the same order: A1 and A1 o D, their tones, the
    rectangles on the last frame); for T = 2 the result is draw_sample's sample field for field.  Frame t in between
    shows A1 o D(s), D's angle, log-zoom and shifts scaled by s = t / (T - 1): a steady relative motion from the first
    frame to the last.  The tones of the frames in between (around the clip's shared gain and gamma) and their
    rectangles, each frame's own draw of the cfg's eraser rule, come from a second generator,
    default_rng([seed, epoch, index, 1]).  Composed in double; every number is rounded once to float32."""
    T = int(T)
    if T < 1:
        raise ValueError("draw_clip: T >= 1 expected")
    d = _draw_pair(cfg, seed, epoch, index, W, H, w, h)
    rng = np.random.default_rng([int(seed), int(epoch), int(index), 1])
    u = _uniform(rng)
    f32 = lambda v: [float(np.float32(x)) for x in v]
    frame = lambda A, tone, rects, fill: opt.ClipFrame(f32(A[:2].reshape(6)), f32(tone[0]), f32([tone[1]])[0], tuple(rects), f32(fill))
    out = [frame(d["A1"], d["tone"][0], (), d["fill"])]
    for t in range(1, T - 1):
        own = u(cfg.gain_rel)
        tone = ([2.0 ** (d["shared_gain"] + own + u(cfg.chan)) for _ in range(3)], 2.0 ** (d["shared_gamma"] + u(cfg.gamma_rel)))
        rects, fill = _draw_erase(rng, cfg, w, h)
        out.append(frame(d["A1"] @ _rel_motion(d, t / (T - 1.0), w, h), tone, rects, fill))
    if T > 1:
        out.append(frame(d["A1"] @ _rel_motion(d, 1.0, w, h), d["tone"][1], d["rects"], d["fill"]))
    return out


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
    NAME = "AugmentLoader"
    # what a subclass with another kind of item restates (ClipLoader): _probe, _new_set, _decode_into, _augment

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
            pin = self.state is not None
            self.sets[which] = self._new_set(lambda shape, dt: torch.empty((self.batch,) + shape, dtype=dt, pin_memory=pin))
        return self.sets[which]

    def _probe(self, index):
        """the source size (W, H) all items must have, from the first item decoded"""
        first = self.pairs.load(index)[0]
        return (first.shape[1], first.shape[0])

    def _new_set(self, new):
        """one set of staging buffers: {input name: new(shape of one item, dtype)}"""
        W, H = self.source
        return dict(rgb1=new((H, W, 3), torch.uint8), rgb2=new((H, W, 3), torch.uint8), flow=new((H, W, 2), torch.float32),
                    skip=new((H, W), torch.uint8))

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
            self.source = self._probe(idx[0])
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
        out = self._augment(epoch, idx, ins)
        if self.state is not None:
            self.called = (stream, torch.cuda.Event())
            self.called[1].record()
        return out

    def _augment(self, epoch, idx, ins):
        """the batch of the items `idx` from their uploaded inputs: the draws and the one call"""
        W, H = self.source
        samples = [draw_sample(self.cfg, self.seed, epoch, i, W, H, *self.size) for i in idx]
        return self.augment(self.state, ins["rgb1"], ins["rgb2"], ins["flow"], samples, self.size, skip=ins["skip"],
                            scale=self.scale, bias=self.bias, tau=self.tau)

    def epoch(self, epoch):
        """an iterator over the batches of one epoch, which becomes the loader's epoch in progress at this call"""
        self.generation += 1
        return self._epoch(epoch, self.generation)

    def _epoch(self, epoch, generation):
        order, n = self.order(epoch), len(self)
        pending = None
        for k in range(n):
            if generation != self.generation:               # checked after every yield, before a shared set is touched
                raise RuntimeError("%s: epoch %d was replaced by a later epoch() of this loader" % (self.NAME, epoch))
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


# ---- clips (DESIGN.md "Training clips") ------------------------------------------------------------------------------------
LINK_KINDS = ("next", "first")
Clip = collections.namedtuple("Clip", "frames links flows skips track")


class ClipList:
    """The clips of a tree written with --mid K (and --tracks P): a clip is a line of OUT/all_files.list that has at least
    one OUT/Mid/<seq>/<frame>_sII.png.  Its steps are the sorted II, n of them; its T = n + 2 frames are rgb1, the n
    in-between PNGs and rgb2.  links: which of
      "next"   the links (t, t + 1): link 0 is the first snapshot's flow from frame 1 (_sII.flo of the first step), link k
               the flow from snapshot k to the next state (_sII_step.flo of step k);
      "first"  the links (0, k): the snapshots' flows from frame 1 (_sII.flo), and (0, T - 1), the pair's OUT/Flow file;
    in that order when both are named.  A link's skip plane is the occlusion of that link where its file exists: for a
    "next" link <frame>_sII_occ.png (lines.mid_layer_files; step 0 for link 0), for (0, 1) that of step 0 too, for
    (0, T - 1) OUT/Occ/<seq>/<frame>.png; zeros otherwise.  tracks: read OUT/Tracks/<seq>/<frame>.trk, whose F must be T;
    its first P points are used, P the fewest points of any clip's file (so all clips have one P).  With `tracks` a clip
    without its file is a ValueError that names it.  A file the list names under another root (the tree was moved) is
    looked up under `root` by its last three components.  Trees of --mid_bg (OUT/MidFull) are not read."""

    def __init__(self, root, links=("next",), tracks=True):
        import glob
        import re
        from . import lines, trk
        links = tuple(links)
        if not links or set(links) - set(LINK_KINDS) or len(set(links)) != len(links):
            raise ValueError("ClipList: links: some of %s" % ", ".join(LINK_KINDS))
        self.root, self.link_kinds, self.tracks = root, links, bool(tracks)
        lst = osp.join(root, LISTS[""])
        self.clips, self.P = [], None
        for ln in open(lst).read().splitlines():
            if not ln.strip():
                continue
            names = ln.split(" ")
            if len(names) != 3:
                raise ValueError("%s: `rgb1 rgb2 flow` expected, got %r" % (lst, ln))
            rgb1, rgb2, flow = (self._find(p) for p in names)
            seq, stem = osp.basename(osp.dirname(flow)), osp.basename(flow)[:-4]
            prefix = osp.join(root, "Mid", seq, stem)
            steps = sorted(int(m.group(1)) for m in (re.fullmatch(re.escape(stem) + r"_s(\d+)\.png", osp.basename(f))
                                                     for f in glob.glob(glob.escape(prefix) + "_s*.png")) if m)
            if not steps:
                continue
            mid = [lines.mid_files(prefix, i) for i in steps]
            occ = lambda step: lines.mid_layer_files(prefix, step)["occ"]
            found = lambda f: f if osp.exists(f) else None
            table, flows, skips = [], [], []
            if "next" in links:
                for k in range(len(steps) + 1):
                    table.append((k, k + 1))
                    flows.append(mid[0]["flow"] if k == 0 else mid[k - 1]["step"])
                    skips.append(found(occ(0 if k == 0 else steps[k - 1])))
            if "first" in links:
                for k in range(1, len(steps) + 1):
                    table.append((0, k))
                    flows.append(mid[k - 1]["flow"])
                    skips.append(found(occ(0)) if k == 1 else None)
                table.append((0, len(steps) + 1))
                flows.append(flow)
                skips.append(found(osp.join(root, PLANES["occ"], seq, stem + ".png")))
            track = None
            if self.tracks:
                track = osp.join(root, "Tracks", seq, stem + ".trk")
                if not osp.exists(track):
                    raise ValueError("ClipList: tracks=True, but %s does not exist" % track)
                head = trk.read(track)
                if head["pos"].shape[0] != len(steps) + 2:
                    raise ValueError("%s: F = %d, but the clip has T = %d frames" % (track, head["pos"].shape[0], len(steps) + 2))
                self.P = head["pos"].shape[1] if self.P is None else min(self.P, head["pos"].shape[1])
            self.clips.append(Clip([rgb1] + [m["rgb"] for m in mid] + [rgb2], tuple(table), flows, skips, track))

    _find = PairList._find

    def __len__(self):
        return len(self.clips)

    def __getitem__(self, i):
        return self.clips[i]

    def load(self, i):
        """-> (frames u8[T,H,W,3], links ((i, j), ..), flows f32[L,H,W,2], skip u8[L,H,W] (0 / 255), pos f32[T,P,2] and
        occ u8[T,P], or None and None without tracks)"""
        from . import trk
        c = self.clips[i]
        frames = np.stack([np.asarray(Image.open(f).convert("RGB")) for f in c.frames])
        flows = np.stack([flo.flow_read(f) for f in c.flows])
        if flows.shape[1:3] != frames.shape[1:3]:
            raise ValueError("clip %d (%s): frames and flows of one size expected" % (i, c.frames[0]))
        skip = np.zeros(flows.shape[:3], np.uint8)
        for l, f in enumerate(c.skips):
            if f is not None:
                a = np.asarray(Image.open(f))
                if a.shape[:2] != flows.shape[1:3]:
                    raise ValueError("clip %d: %s of the flow's size expected" % (i, f))
                skip[l] = np.where(a.reshape(a.shape[0], a.shape[1], -1).any(-1), 255, 0)
        pos = occ = None
        if c.track is not None:
            t = trk.read(c.track)
            pos, occ = np.ascontiguousarray(t["pos"][:, :self.P]), np.ascontiguousarray(t["occ"][:, :self.P])
        return frames, c.links, flows, skip, pos, occ


class ClipLoader(AugmentLoader):
    """Batches of augmented clips: AugmentLoader's ownership, generation and stream rules (its code) over a ClipList
    (anything with len() and load(i) -> frames, links, flows, skip, pos, occ).  All clips have one source size, one T,
    one link table and one P: a clip that differs makes next() and batch_at raise ValueError.  batch: clips per batch, at
    most 64 and at most 256 // T.  A clip's augmentation is draw_clip(cfg, seed, e, its index in the list, ..); a batch
    is a dict(video, flows, valid) and, when the clips have tracks, (tracks, vis) of what `augment` returns
    (opt.augment_clips; the numpy twin of the tests with state = None)."""
    NAME = "ClipLoader"

    def __init__(self, clips, state, batch, size, cfg=AUG_DEFAULT, seed=0, jobs=8, augment=opt.augment_clips, scale=(1, 1, 1),
                 bias=(0, 0, 0), tau=1.0, shuffle=True):
        super().__init__(clips, state, batch, size, cfg=cfg, seed=seed, jobs=jobs, augment=augment, scale=scale, bias=bias, tau=tau,
                         shuffle=shuffle)
        self.shape = None                       # (T, links, P), known from the first clip decoded

    def _probe(self, index):
        frames, links, flows, skip, pos, occ = self.pairs.load(index)
        T = frames.shape[0]
        if self.batch > 256 // T:
            raise ValueError("ClipLoader: at most 256 // T = %d clips of %d frames a batch, not %d" % (256 // T, T, self.batch))
        self.shape = (T, tuple(tuple(l) for l in links), None if pos is None else pos.shape[1])
        return (frames.shape[2], frames.shape[1])

    def _new_set(self, new):
        W, H = self.source
        T, links, P = self.shape
        bufs = dict(frames=new((T, H, W, 3), torch.uint8), flows=new((len(links), H, W, 2), torch.float32),
                    skip=new((len(links), H, W), torch.uint8))
        if P is not None:
            bufs.update(pos=new((T, P, 2), torch.float32), occ=new((T, P), torch.uint8))
        return bufs

    def _decode_into(self, bufs, slot, index):
        frames, links, flows, skip, pos, occ = self.pairs.load(index)
        shape = (frames.shape[0], tuple(tuple(l) for l in links), None if pos is None else pos.shape[1])
        if (frames.shape[2], frames.shape[1]) != self.source or shape != self.shape:
            raise ValueError("ClipLoader: clip %d is %dx%d with T = %d, %d links and P = %s, the first one %dx%d with T = %d, %d links "
                             "and P = %s" % ((index, frames.shape[2], frames.shape[1], shape[0], len(shape[1]), shape[2]) + self.source +
                                             (self.shape[0], len(self.shape[1]), self.shape[2])))
        bufs["frames"][slot].numpy()[...] = frames
        bufs["flows"][slot].numpy()[...] = flows
        bufs["skip"][slot].numpy()[...] = skip
        if pos is not None:
            bufs["pos"][slot].numpy()[...] = pos
            bufs["occ"][slot].numpy()[...] = occ

    def _augment(self, epoch, idx, ins):
        W, H = self.source
        T, links, _ = self.shape
        samples = [draw_clip(self.cfg, self.seed, epoch, i, W, H, *self.size, T) for i in idx]
        return self.augment(self.state, ins["frames"], samples, self.size, links=links, flows=ins["flows"], skip=ins["skip"],
                            pos=ins.get("pos"), occ=ins.get("occ"), scale=self.scale, bias=self.bias, tau=self.tau)
