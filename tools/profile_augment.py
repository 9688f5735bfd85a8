#!/usr/bin/env python3
"""Device time of a training batch (profiles/augment/README.md).

One ArapFlow_AugmentPairs call at B = 8 for 854x480 -> 768x384 and 1920x1080 -> 960x544, with all outputs and with the
two images only, under augmentations drawn by data.draw_sample(AUG_DEFAULT); against
  copy    one device copy whose traffic (bytes read + bytes written) equals the call's algorithmic traffic: every input
          plane it reads once, every output once
  torch   the same batch as a chain of torch ops written here: the table lookup on the source frames, affine_grid and
          grid_sample (bilinear, border) for the frames and the flow, the masks of bad and outside pixels, the flow in
          the new coordinates, the rectangles.  Approximately the same result, not bit-equal (its largest deviation from
          the fused images is printed); the motion-boundary guard is left out of it.
The three are timed in one run, alternating, REPS windows of ITER calls each after WARM warm-up calls, every window between
device events on the stream the work runs on.  Then the loader end to end: a tree of PAIRS pairs at 854x480 written to a
temporary directory, one epoch to warm the page cache, one epoch timed (decoding in 16 threads, pinned staging, upload, one
call per batch of 8).  Prints one JSON line and, with --out, writes it to DIR/numbers.json.  For the kernel table:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/profile_augment.py --only fused --no-loader
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARM, ITER, REPS, B, PAIRS = 3, 20, 9, 8, 64
SHAPES = [((854, 480), (768, 384)), ((1920, 1080), (960, 544))]
DEVICE = "cuda"
SCALE, BIAS = (1 / 58.395, 1 / 57.12, 1 / 57.375), (-2.1179, -2.0357, -1.8044)


def frames(W, H, n, seed):
    """n frames with structure at every scale (a PNG of pure noise would decode unlike a picture)"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    out = []
    for i in range(n):
        base = [128 + 90 * np.sin(xs / rng.uniform(20, 90) + rng.uniform(0, 6)) * np.cos(ys / rng.uniform(20, 90)) for _ in range(3)]
        out.append(np.clip(np.stack(base, -1) + rng.normal(0, 6, (H, W, 3)), 0, 255).astype(np.uint8))
    return np.stack(out)


def torch_chain(torch, rgb1, rgb2, flow, skip, samples, size, tables, want_flow):
    """formulation (b): -> a closure that computes the batch with torch ops alone"""
    import torch.nn.functional as Fn
    Bn, H, W = rgb1.shape[:3]
    w, h = size
    A = lambda T: np.vstack([np.asarray(T, np.float64).reshape(2, 3), [0, 0, 1]])
    n_out = np.asarray([[(w - 1) / 2, 0, (w - 1) / 2], [0, (h - 1) / 2, (h - 1) / 2], [0, 0, 1]])
    n_src = np.asarray([[2 / (W - 1), 0, -1], [0, 2 / (H - 1), -1], [0, 0, 1]])
    dev = lambda a, dt=torch.float32: torch.as_tensor(np.asarray(a), dtype=dt).to(DEVICE)
    theta = [dev(np.stack([(n_src @ A(s[k]) @ n_out)[:2] for s in samples])) for k in (0, 1)]
    lut = dev(np.stack([t[1] for t in tables]))                                  # [B,2,3,256]
    P2 = dev(np.stack([t[0] for t in tables])).view(Bn, 2, 3)
    rects = np.zeros((Bn, 4, 4), np.float32)
    for b, s in enumerate(samples):
        for i, r in enumerate(s.erase):
            rects[b, i] = r
    rects, fill = dev(rects), dev(np.stack([s.fill for s in samples]))
    ys, xs = torch.meshgrid(torch.arange(h, device=DEVICE, dtype=torch.float32), torch.arange(w, device=DEVICE, dtype=torch.float32), indexing="ij")

    def image(rgb, k):
        idx = rgb.permute(0, 3, 1, 2).reshape(Bn, 3, -1).long()
        src = torch.gather(lut[:, k], 2, idx).view(Bn, 3, H, W)
        grid = Fn.affine_grid(theta[k], (Bn, 3, h, w), align_corners=True)
        return Fn.grid_sample(src, grid, mode="bilinear", padding_mode="border", align_corners=True), grid

    def run():
        img1, grid1 = image(rgb1, 0)
        img2, _ = image(rgb2, 1)
        inside = [(xs[None, None] >= rects[:, :, 0, None, None]) & (xs[None, None] < rects[:, :, 2, None, None]) &
                  (ys[None, None] >= rects[:, :, 1, None, None]) & (ys[None, None] < rects[:, :, 3, None, None])][0].any(1)
        img2 = torch.where(inside[:, None], fill[:, :, None, None], img2)
        if not want_flow:
            return img1, img2
        fl = flow.permute(0, 3, 1, 2)
        bad = ~torch.isfinite(fl).all(1) | (skip != 0)
        u = Fn.grid_sample(torch.where(bad[:, None], torch.zeros((), device=DEVICE), fl), grid1, mode="bilinear", padding_mode="border", align_corners=True)
        hit = Fn.grid_sample(bad[:, None].float(), grid1, mode="bilinear", padding_mode="border", align_corners=True)[:, 0] > 0
        q = torch.stack([(grid1[..., 0] + 1) * ((W - 1) / 2), (grid1[..., 1] + 1) * ((H - 1) / 2)], 1)
        p = torch.einsum("bij,bjhw->bihw", P2[:, :, :2], q + u) + P2[:, :, 2, None, None]
        out = p - torch.stack([xs, ys])[None]
        valid = (grid1.abs() <= 1).all(-1) & ~hit & torch.isfinite(out).all(1)
        return img1, img2, torch.where(valid[:, None], out, torch.zeros((), device=DEVICE)), valid.to(torch.uint8) * 255
    return run


def window(torch, fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / calls           # microseconds a call


def stats(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="directory for numbers.json")
    ap.add_argument("--only", default=None, choices=("fused", "copy", "torch"), help="run this contender alone (for the profiler)")
    ap.add_argument("--iter", type=int, default=ITER)
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--no-loader", action="store_true")
    ap.add_argument("--pairs", type=int, default=PAIRS)
    args = ap.parse_args()
    import torch
    from arap_flow_amd import data, flo, opt
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    st = opt.State()
    st.set_stream(torch.cuda.current_stream())
    res = dict(B=B, iter=args.iter, reps=args.reps, shapes=[])
    for (W, H), (w, h) in SHAPES:
        rng = np.random.default_rng(W)
        rgb1, rgb2 = (torch.from_numpy(frames(W, H, B, seed)).cuda() for seed in (1, 2))
        ys, xs = np.mgrid[0:H, 0:W]
        fl = np.stack([np.stack([8 * np.sin(xs / 97.0 + b) + np.where(xs > W // 2, 5.0, 0.0), 6 * np.cos(ys / 71.0 - b)], -1) for b in range(B)])
        flow = torch.from_numpy(fl.astype(np.float32)).cuda()
        skip = torch.from_numpy(np.where(rng.random((B, H, W)) < 0.02, 255, 0).astype(np.uint8)).cuda()
        samples = [data.draw_sample(data.AUG_DEFAULT, 0, 0, b, W, H, w, h) for b in range(B)]
        tables = [opt.augment_tables(s, SCALE, BIAS) for s in samples]
        row = dict(source=[W, H], crop=[w, h], modes={})
        for mode, want in (("all", opt.AUG_OUTPUTS), ("img", ("img1", "img2"))):
            outs = opt.augment_pairs(st, rgb1, rgb2, flow, samples, (w, h), skip=skip, scale=SCALE, bias=BIAS, want=want)
            need_flow = mode == "all"
            fused = lambda: opt.augment_pairs(st, rgb1, rgb2, flow if need_flow else None, samples, (w, h), skip=skip if need_flow else None,
                                              scale=SCALE, bias=BIAS, want=want, out=outs)
            read = B * W * H * (6 + (9 if need_flow else 0))
            written = B * w * h * (24 + (9 if need_flow else 0))
            src = torch.empty((read + written) // 2, dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)
            chain = torch_chain(torch, rgb1, rgb2, flow, skip, samples, (w, h), tables, need_flow)
            ref = chain()
            torch.cuda.synchronize()
            dev = {k: float((outs[k] - r).abs().max()) for k, r in zip(("img1", "img2"), ref)}
            contenders = dict(fused=fused, copy=lambda: dst.copy_(src), torch=chain)
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
            row["modes"][mode] = dict(bytes_read=read, bytes_written=written, us_per_call={k: stats(v) for k, v in times.items()},
                                      torch_max_abs_deviation=dev)
            del src, dst, ref, chain
        res["shapes"].append(row)
        del rgb1, rgb2, flow, skip
        torch.cuda.empty_cache()
    if not args.no_loader:
        W, H, w, h = 854, 480, 768, 384
        from PIL import Image
        with tempfile.TemporaryDirectory() as root:
            pics = frames(W, H, 8, 3)
            lines = []
            for i in range(args.pairs):
                names = []
                for d, shift in (("inpRGB", 0), ("wRGB", 3)):
                    os.makedirs(os.path.join(root, d, "seq"), exist_ok=True)
                    names.append(os.path.join(root, d, "seq", "%05d.png" % i))
                    Image.fromarray(np.roll(pics[i % 8], shift + i, axis=1)).save(names[-1])
                os.makedirs(os.path.join(root, "Flow", "seq"), exist_ok=True)
                names.append(os.path.join(root, "Flow", "seq", "%05d.flo" % i))
                flo.flow_write(names[-1], np.full((H, W, 2), 3.0, np.float32))
                lines.append(" ".join(names))
            open(os.path.join(root, "all_files.list"), "w").write("\n".join(lines))
            ld = data.AugmentLoader(data.PairList(root), st, B, (w, h), data.AUG_DEFAULT, seed=0, jobs=16, scale=SCALE, bias=BIAS)
            rates = []
            for e in range(3):
                t0 = time.perf_counter()
                for batch in ld:
                    pass
                torch.cuda.synchronize()
                rates.append(args.pairs / (time.perf_counter() - t0))
            ld.close()
            res["loader"] = dict(source=[W, H], crop=[w, h], pairs=args.pairs, batch=B, jobs=16, pairs_per_s_by_epoch=rates)
    st.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        open(os.path.join(args.out, "numbers.json"), "w").write(line + "\n")


if __name__ == "__main__":
    main()
