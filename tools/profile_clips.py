#!/usr/bin/env python3
"""Device time of a batch of training clips (profiles/clips/README.md).

One ArapFlow_AugmentClips call (video, flows, valid, tracks, vis) at B = 8 for 854x480 -> 512x384, T = 5 (the --mid 3
example) and T = 10, "next" links, P = 4096, under augmentations drawn by data.draw_clip(AUG_DEFAULT); against
  pairs   the code before the clip call making the same tensors: T - 1 ArapFlow_AugmentPairs calls -- call t gives frame
          t, link t's flow and its valid plane, the last one also img2 -- and the tracks as batched torch ops (the inverse
          maps applied with one einsum, the crop test, the rectangles)
  copy    one device copy whose traffic (bytes read + bytes written) equals the clip call's algorithmic traffic: every
          input plane it reads once, every output once
The three are timed in one run, alternating, REPS windows of ITER calls each after WARM warm-up calls, every window between
device events on the stream the work runs on.  After the windows the two kernels of the clip call are timed on their own
with the state's kernel timer (events around each launch).  Prints one JSON line and, with --out, writes it to
DIR/numbers.json.  For the kernel table:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/profile_clips.py --only clips
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.profile_augment import frames, stats, window       # noqa: E402

WARM, ITER, REPS, B, P = 3, 20, 9, 8, 4096
SOURCE, CROP, LENGTHS = (854, 480), (512, 384), (5, 10)
SCALE, BIAS = (1 / 58.395, 1 / 57.12, 1 / 57.375), (-2.1179, -2.0357, -1.8044)


def torch_tracks(torch, pos, occ, samples, tables, size):
    """the tracks and their visibility as batched torch ops -> a closure"""
    w, h = size
    Bn, T = pos.shape[:2]
    dev = lambda a, dt=torch.float32: torch.as_tensor(np.asarray(a), dtype=dt).cuda()
    Pm = dev(np.stack([[tables[b][t][0] for t in range(T)] for b in range(Bn)])).view(Bn, T, 2, 3)
    rects = np.zeros((Bn, T, 4, 4), np.float32)
    for b, clip in enumerate(samples):
        for t, f in enumerate(clip):
            for i, r in enumerate(f.erase):
                rects[b, t, i] = r
    rects = dev(rects)

    def run():
        o = torch.einsum("btij,btpj->btpi", Pm[..., :2], pos) + Pm[:, :, None, :, 2]
        fin = torch.isfinite(o).all(-1)
        o = torch.where(fin[..., None], o, torch.zeros((), device="cuda"))
        inn = fin & (o[..., 0] >= 0) & (o[..., 0] <= w - 1) & (o[..., 1] >= 0) & (o[..., 1] <= h - 1)
        r = torch.floor(o + 0.5)
        hit = ((r[..., None, 0] >= rects[:, :, None, :, 0]) & (r[..., None, 0] < rects[:, :, None, :, 2]) &
               (r[..., None, 1] >= rects[:, :, None, :, 1]) & (r[..., None, 1] < rects[:, :, None, :, 3])).any(-1)
        return o, ((occ == 0) & inn & ~hit).to(torch.uint8) * 255
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="directory for numbers.json")
    ap.add_argument("--only", default=None, choices=("clips", "pairs", "copy"), help="run this contender alone (for the profiler)")
    ap.add_argument("--iter", type=int, default=ITER)
    ap.add_argument("--reps", type=int, default=REPS)
    args = ap.parse_args()
    import torch
    from arap_flow_amd import data, opt
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    st = opt.State()
    st.set_stream(torch.cuda.current_stream())
    (W, H), (w, h) = SOURCE, CROP
    res = dict(B=B, P=P, source=[W, H], crop=[w, h], iter=args.iter, reps=args.reps, lengths=[])
    for T in LENGTHS:
        L = T - 1
        links = [(t, t + 1) for t in range(L)]
        rng = np.random.default_rng(T)
        pics = frames(W, H, T, T)
        video = torch.from_numpy(np.stack([np.roll(pics, 7 * b, axis=2) for b in range(B)])).cuda()
        ys, xs = np.mgrid[0:H, 0:W]
        fl = np.stack([np.stack([np.stack([8 * np.sin(xs / 97.0 + b + l) + np.where(xs > W // 2, 5.0, 0.0), 6 * np.cos(ys / 71.0 - b)], -1)
                                 for l in range(L)]) for b in range(B)])
        flows = torch.from_numpy(fl.astype(np.float32)).cuda()
        skip = torch.from_numpy(np.where(rng.random((B, L, H, W)) < 0.02, 255, 0).astype(np.uint8)).cuda()
        pos = torch.from_numpy((rng.uniform(0, 1, (B, T, P, 2)) * [W - 1, H - 1]).astype(np.float32)).cuda()
        occ = torch.from_numpy(np.where(rng.random((B, T, P)) < 0.2, 255, 0).astype(np.uint8)).cuda()
        samples = [data.draw_clip(data.AUG_DEFAULT, 0, 0, b, W, H, w, h, T) for b in range(B)]
        tables = [[opt.clip_tables(f, SCALE, BIAS) for f in clip] for clip in samples]
        kw = dict(links=links, flows=flows, skip=skip, pos=pos, occ=occ, scale=SCALE, bias=BIAS)
        outs = opt.augment_clips(st, video, samples, (w, h), **kw)
        clips = lambda: opt.augment_clips(st, video, samples, (w, h), out=outs, **kw)
        # the pair path: its inputs as contiguous tensors per call (made once, outside the windows), its outputs too
        pair_in = [(video[:, t].contiguous(), video[:, t + 1].contiguous(), flows[:, t].contiguous(), skip[:, t].contiguous()) for t in range(L)]
        pair_samples = [[opt.AugSample(c[t].T, c[t + 1].T, c[t].gain, c[t].gamma, c[t + 1].gain, c[t + 1].gamma, c[t + 1].erase, c[t + 1].fill)
                         for c in samples] for t in range(L)]
        pair_want = [("img1", "flow", "valid") if t < L - 1 else opt.AUG_OUTPUTS for t in range(L)]
        pair_out = [opt.augment_pairs(st, *pair_in[t][:3], pair_samples[t], (w, h), skip=pair_in[t][3], scale=SCALE, bias=BIAS,
                                      want=pair_want[t]) for t in range(L)]
        tracks = torch_tracks(torch, pos, occ, samples, tables, (w, h))

        def pairs():
            for t in range(L):
                opt.augment_pairs(st, pair_in[t][0], pair_in[t][1] if t == L - 1 else None, pair_in[t][2], pair_samples[t], (w, h),
                                  skip=pair_in[t][3], scale=SCALE, bias=BIAS, want=pair_want[t], out=pair_out[t])
            return tracks()
        o, vis = pairs()
        torch.cuda.synchronize()
        agree = dict(flows=bool(all(torch.equal(outs["flows"][:, t], pair_out[t]["flow"]) for t in range(L))),
                     valid=bool(all(torch.equal(outs["valid"][:, t], pair_out[t]["valid"]) for t in range(L))),
                     tracks_max_abs_deviation=float((outs["tracks"] - o).abs().max()), vis_differ=int((outs["vis"] != vis).sum()))
        read = B * T * W * H * 3 + B * L * W * H * 9 + B * T * P * 9
        written = B * T * w * h * 12 + B * L * w * h * 9 + B * T * P * 9
        src = torch.empty((read + written) // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        contenders = dict(clips=clips, pairs=pairs, copy=lambda: dst.copy_(src))
        if args.only:
            contenders = {args.only: contenders[args.only]}
        for fn in contenders.values():
            for _ in range(WARM):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in contenders}
        for _ in range(args.reps):
            for k, fn in contenders.items():
                times[k].append(window(torch, fn, args.iter))
        row = dict(T=T, L=L, bytes_read=read, bytes_written=written, us_per_call={k: stats(v) for k, v in times.items()}, agree=agree)
        if args.only in (None, "clips"):
            st.set_kernel_timing(True)
            for _ in range(args.iter):
                clips()
            torch.cuda.synchronize()
            row["kernel_us"] = {k: (lambda r: r[0] * 1000.0 / r[1])(st.kernel_time(k)) for k in ("k_augment_clip", "k_clip_tracks")}
            st.set_kernel_timing(False)
        res["lengths"].append(row)
        del video, flows, skip, pos, occ, outs, pair_in, pair_out, src, dst
        torch.cuda.empty_cache()
    st.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        open(os.path.join(args.out, "numbers.json"), "w").write(line + "\n")


if __name__ == "__main__":
    main()
