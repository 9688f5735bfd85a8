#!/usr/bin/env python3
"""Cost of the fold diagnostics (DESIGN.md "Fold diagnostics"): one batch of synthetic DAVIS-shaped frames through
FrameSolver.solve_async(warp, download) + wait, with the diagnostics off (default) or on, timed on the host per batch.

  python tools/diag_probe.py [--size 854 480] [--batch 8] [--schedule 19 8 400] [--diag] [--reps 5]

Prints one JSON line.  Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel times
(profiles/diag/README.md)."""
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
    ap.add_argument("--diag", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    from arap_flow_amd import opt, synth
    W, H = a.size
    frames = [synth.make_frame(W, H, seed=s, K=1, fd=1) for s in range(a.batch)]
    st = opt.State()
    st.use_own_stream()
    fs = opt.FrameSolver(st, W, H, batch=a.batch)
    if a.diag:
        fs.set_diag(True)
    for b, f in enumerate(frames):
        fs.set_frame(b, f["mask_red"], f["constraints"], rgb=f["rgb"])
    ms = []
    for r in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        fs.solve_async(a.batch, *a.schedule, warp=True, download=True)
        fs.wait()
        if r >= a.warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    out = dict(size=[W, H], batch=a.batch, schedule=a.schedule, diag=a.diag, ms_per_batch=[round(v, 3) for v in ms],
               ms_min=round(min(ms), 3), ms_median=round(sorted(ms)[len(ms) // 2], 3),
               resident_launches=fs.stats()["resident_launches"])
    if a.diag:
        out["mesh_stats"] = [{k: (int(v) if isinstance(v, int) else float(v)) for k, v in fs.host_results(b)["mesh_stats"].items()}
                             for b in range(a.batch)]
    fs.close()
    st.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
