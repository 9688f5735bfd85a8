#!/usr/bin/env python3
"""Cost of the in-between frames (DESIGN.md "In-between frames"): one batch of synthetic DAVIS-shaped frames through
FrameSolver.solve_async(warp, download) + wait, with a given snapshot set (none by default), timed on the host per batch.

  python tools/mid_probe.py [--size 854 480] [--batch 8] [--schedule 19 8 400] [--snapshots 4 9 14] [--reps 5]

Prints one JSON line.  Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel times
(profiles/mid_frames/README.md)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=[854, 480])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--schedule", type=int, nargs=3, default=[19, 8, 400])
    ap.add_argument("--snapshots", type=int, nargs="*", default=[])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    from arap_flow_amd import opt, synth
    W, H = a.size
    frames = [synth.make_frame(W, H, seed=s, K=1, fd=1) for s in range(a.batch)]
    st = opt.State()
    st.use_own_stream()
    fs = opt.FrameSolver(st, W, H, batch=a.batch)
    fs.set_snapshots(a.snapshots)
    for b, f in enumerate(frames):
        fs.set_frame(b, f["mask_red"], f["constraints"], rgb=f["rgb"])
    ms = []
    for r in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        fs.solve_async(a.batch, *a.schedule, warp=True, download=True)
        fs.wait()
        if r >= a.warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    if a.snapshots:
        fs.host_snapshot(a.batch - 1, len(a.snapshots) - 1)
    out = dict(size=[W, H], batch=a.batch, schedule=a.schedule, snapshots=a.snapshots, ms_per_batch=[round(v, 3) for v in ms],
               ms_min=round(min(ms), 3), ms_median=round(sorted(ms)[len(ms) // 2], 3),
               resident_launches=fs.stats()["resident_launches"])
    fs.close()
    st.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
