#!/usr/bin/env python3
"""Device time of the moving-background pass (profiles/bg_motion/README.md).

One ArapFlow_Background call with every output on at 854x480 over a 1200x700 picture, a 1.5 degree / 1.01 / (4, -2) px
similarity, on the outputs of one ArapFlow_WarpEx of a synthetic object; ITER calls after WARM warm-up calls, timed with
the library's device events (ArapFlow_TimerBegin / End).  Prints one JSON line: microseconds per call, the bytes the call
streams (inputs read and outputs written once, the picture's gathers not counted) and the rate that makes.  For the
kernel table run it under the profiler, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/profile_background.py
"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARM, ITER = 5, 50
W, H, BW, BH = 854, 480, 1200, 700


def main():
    import torch
    from arap_flow_amd import opt
    rng = np.random.default_rng(0)
    ys, xs = np.mgrid[0:H, 0:W]
    inside = ((xs - 0.45 * W) / (0.22 * W)) ** 2 + ((ys - 0.5 * H) / (0.3 * H)) ** 2 <= 1
    mask = np.where(inside, 0, 255).astype(np.uint8)
    flow = np.stack([6.0 + 0.01 * (ys - H / 2), -3.0 + 0.01 * (xs - W / 2)], -1).astype(np.float32)
    flow[~inside] = 0
    rgb1 = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    bg = rng.integers(0, 256, (BH, BW, 3)).astype(np.uint8)
    st = opt.State()
    r = opt.warp_image_ex(st, rgb1, mask, flow)
    t = np.deg2rad(1.5)
    a, b, cx, cy = 1.01 * np.cos(t), 1.01 * np.sin(t), (W - 1) / 2.0, (H - 1) / 2.0
    M1 = (C.c_float * 6)(1, 0, 170, 0, 1, 110)
    M2 = (C.c_float * 6)(a, -b, 170 + cx - a * cx + b * cy + 4, b, a, 110 + cy - b * cx - a * cy - 2)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    ins = [up(x) for x in (rgb1, mask, r["warped_rgb"], r["warped_mask"], flow, r["occlusion"], r["backward_flow"],
                           r["occlusion_bwd"])]
    dbg = up(bg)
    outs = [torch.empty(s, dtype=d, device="cuda") for s, d in (((H, W, 3), torch.uint8), ((H, W, 3), torch.uint8),
            ((H, W, 2), torch.float32), ((H, W), torch.uint8), ((H, W, 2), torch.float32), ((H, W), torch.uint8))]
    p = lambda x: C.c_void_p(x.data_ptr())

    def call():
        rc = st.lib.ArapFlow_Background(st.handle, W, H, p(dbg), BW, BH, M1, M2, *[p(x) for x in ins], *[p(x) for x in outs])
        assert rc == 0, rc

    torch.cuda.synchronize()
    for _ in range(WARM):
        call()
    torch.cuda.synchronize()
    st.timer_begin()
    for _ in range(ITER):
        call()
    ms = st.timer_end()
    N = W * H
    streamed = N * (2 * (3 + 1 + 8 + 1) + 2 * (3 + 8 + 1))      # per domain: rgb, mask, flow, occ in; rgb, flow, occ out
    us = 1e3 * ms / ITER
    print(json.dumps(dict(what="ArapFlow_Background, every output", W=W, H=H, bg=[BW, BH], calls=ITER, us_per_call=us,
                          streamed_bytes=streamed, streamed_GBps=streamed / us * 1e-3)))
    st.close()


if __name__ == "__main__":
    main()
