#!/usr/bin/env python3
"""Kernel times of one point-track call (profiles/tracks/README.md).

Run it under the profiler, in a run of its own and with one number of points per run:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/profile_tracks.py --points 4096
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/profile_tracks.py --points N
One ArapFlow_TrackPoints call with both outputs on: 3 layers at 854x480, T = 4 states, P = 4096 (sparse) and P = N (one
point per pixel) uniform sub-pixel points.  ITER calls after WARM warm-up calls per P.  Without the profiler it prints
the device-event times of a call for both P.
Inputs: tools/profile_layers_step.py's two states a and b; the four states are a / 2, a, (a + b) / 2, b.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
WARM, ITER = 5, 50


def inputs():
    import profile_layers_step
    _, masks, fa, fb = profile_layers_step.inputs()
    states = np.stack([0.5 * fa, fa, 0.5 * (fa + fb), fb]).astype(np.float32)
    return masks, states


def points(P, W, H):
    rng = np.random.default_rng(P)
    return np.stack([rng.uniform(0, W - 1, P), rng.uniform(0, H - 1, P)], -1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", nargs="*", default=["4096", "N"], help="numbers of points; N = one per pixel")
    flags = ap.parse_args()
    import torch
    from arap_flow_amd import opt
    masks, states = inputs()
    n, H, W = masks.shape
    T = len(states)
    st = opt.State()
    lib, dev = st.lib, "cuda"
    d_msk, d_flow = torch.from_numpy(masks).to(dev), torch.from_numpy(states).to(dev)
    p = lambda t: t.data_ptr()
    out = dict(W=W, H=H, layers=n, states=T, rounds=ITER, note="device events around one ArapFlow_TrackPoints call")
    for word in flags.points:
        P = W * H if word == "N" else int(word)
        d_pts = torch.from_numpy(points(P, W, H)).to(dev)
        o_pos = torch.empty(T, P, 2, dtype=torch.float32, device=dev)
        o_occ = torch.empty(T, P, dtype=torch.uint8, device=dev)
        scr = torch.empty(int(lib.ArapFlow_TrackPointsScratchBytes(W, H, T, P)), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ms = []
        for it in range(WARM + ITER):
            st.timer_begin()
            rc = lib.ArapFlow_TrackPoints(st.handle, W, H, n, p(d_msk), T, p(d_flow), P, p(d_pts), p(o_pos), p(o_occ), p(scr))
            assert rc == 0, rc
            t = st.timer_end()
            if it >= WARM:
                ms.append(t)
        torch.cuda.synchronize()
        out["P=%s" % word] = dict(points=P, median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)),
                                  hidden=float((o_occ == 255).float().mean().item()), scratch_bytes=scr.numel())
    print(json.dumps(out))
    st.close()


if __name__ == "__main__":
    main()
