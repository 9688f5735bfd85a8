#!/usr/bin/env python3
"""Device time of the relight pass (profiles/relight/README.md).

ArapFlow_Relight at 854x480 on a frame whose cover is three overlapping ellipses, under a light with every stage on
(field of 200-pixel cells, vignette, tone curve, noise): without a shadow, and with the shadow at r = 0, 1 and 16 (offset
(9, -6), depth 160), cover and solver-mask conventions; then the device work of a whole `light` line, the two calls of a
pair (frame 1 with the solver's mask, frame 2 with a cover, r = 16).  Per configuration REPS windows of ITER calls after
WARM warm-up calls, each window timed with the library's device events (ArapFlow_TimerBegin / End).  Prints one JSON
line: microseconds per call (the median window, and the smallest and largest) and the algorithmic bytes of k_relight (3 of
RGB read and written, one cover byte with a shadow).  For the kernel table run it under the profiler, in a run of its
own, one configuration per run:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/profile_relight.py --only shadow_r16
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARM, ITER, REPS = 20, 2000, 5
W, H, CELL = 854, 480, 200.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, help="time this configuration alone (for the profiler)")
    ap.add_argument("--iter", type=int, default=ITER)
    args = ap.parse_args()
    import torch
    from arap_flow_amd import opt, pipeline
    rng = np.random.default_rng(0)
    ys, xs = np.mgrid[0:H, 0:W]
    ell = lambda cx, cy, rx, ry: ((xs - cx) / rx) ** 2 + ((ys - cy) / ry) ** 2 <= 1
    obj = ell(0.35 * W, 0.5 * H, 0.3 * W, 0.45 * H) | ell(0.55 * W, 0.4 * H, 0.25 * W, 0.35 * H) | ell(0.7 * W, 0.6 * H, 0.22 * W, 0.38 * H)
    rgb = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    st = opt.State()
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_rgb, d_cover, d_mask = up(rgb), up(np.where(obj, 255, 0).astype(np.uint8)), up(np.where(obj, 0, 255).astype(np.uint8))
    out = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())
    light = pipeline.LightFrame(17, (0.94 / CELL, 0.34 / CELL, 1536.0, -0.34 / CELL, 0.94 / CELL, 512.0), 0.25, 0.4, (1.05, 1.0, 0.95),
                                0.9, 9, -6, 16, 160, 2.0, 0.01)

    def relight(frame, cover, is_mask):
        q = opt.light_frame(frame)

        def call():
            rc = st.lib.ArapFlow_Relight(st.handle, W, H, p(d_rgb), None if cover is None else p(cover), is_mask, C.byref(q), p(out))
            assert rc == 0, rc
        return call

    def timed(call):
        torch.cuda.synchronize()
        for _ in range(WARM):
            call()
        torch.cuda.synchronize()
        windows = []
        for _ in range(REPS):
            st.timer_begin()
            for _ in range(args.iter):
                call()
            windows.append(1e3 * st.timer_end() / args.iter)
        windows.sort()
        return dict(median=windows[len(windows) // 2], min=windows[0], max=windows[-1])

    first, second = relight(light, d_mask, 1), relight(light._replace(seed=pipeline.light_twin_seed(17)), d_cover, 0)

    def line():
        first()
        second()
    configs = dict(neutral=relight(pipeline.LIGHT_NEUTRAL, None, 0), plain=relight(light._replace(sh_g=0), None, 0),
                   shadow_r0=relight(light._replace(sh_r=0), d_cover, 0), shadow_r1=relight(light._replace(sh_r=1), d_cover, 0),
                   shadow_r16=relight(light, d_cover, 0), shadow_r16_mask=first, line_r16=line)
    if args.only:
        configs = {args.only: configs[args.only]}
    us = {name: timed(call) for name, call in configs.items()}
    print(json.dumps(dict(what="ArapFlow_Relight per configuration; line_r16: the two calls of a light line", W=W, H=H,
                          calls_per_window=args.iter, windows=REPS, us_per_call=us,
                          algorithmic_bytes=dict(plain=W * H * 6, shadow=W * H * 7))))
    st.close()


if __name__ == "__main__":
    main()
