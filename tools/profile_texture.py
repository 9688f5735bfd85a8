#!/usr/bin/env python3
"""Device time of the random-texture pass (profiles/retex/README.md).

ArapFlow_Texture at 854x480 on a frame of three overlapping elliptic layers, cells of 24 pixels under a 20 degree
rotation: per kind (every layer of that kind) ITER calls after WARM warm-up calls, timed with the library's device events
(ArapFlow_TimerBegin / End); then the device work of a whole `tex` line, ArapFlow_Texture + ArapFlow_WarpLayers for rgb2
and mask2 on the result.  Prints one JSON line: microseconds per call and the algorithmic bytes of k_tex_fill (n mask
bytes and 3 of RGB read, 3 written per pixel).  For the kernel table run it under the profiler, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/profile_texture.py
"""
import ctypes as C
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARM, ITER = 5, 50
W, H, N_LAYERS, CELL = 854, 480, 3, 24.0


def main():
    import torch
    from arap_flow_amd import opt, pipeline
    rng = np.random.default_rng(0)
    ys, xs = np.mgrid[0:H, 0:W]
    ell = lambda cx, cy, rx, ry: np.where(((xs - cx) / rx) ** 2 + ((ys - cy) / ry) ** 2 <= 1, 0, 255).astype(np.uint8)
    masks = np.stack([ell(0.35 * W, 0.5 * H, 0.3 * W, 0.45 * H), ell(0.55 * W, 0.4 * H, 0.25 * W, 0.35 * H),
                      ell(0.7 * W, 0.6 * H, 0.22 * W, 0.38 * H)])
    flows = np.stack([np.stack([6.0 + 0.01 * (ys - H / 2) + l, -3.0 + 0.01 * (xs - W / 2) - l], -1)
                      for l in range(N_LAYERS)]).astype(np.float32)
    rgb = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    co, si = math.cos(math.radians(20)) / CELL, math.sin(math.radians(20)) / CELL
    st = opt.State()
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_rgb, d_masks, d_flows = up(rgb), up(masks), up(flows)
    out1, out2 = (torch.empty((H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(2))
    mask2 = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    scratch = torch.empty(int(st.lib.ArapFlow_WarpLayersScratchBytes(W, H, N_LAYERS)), dtype=torch.uint8, device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())

    def table(kind):
        return opt.tex_table([pipeline.TexLayer(kind, 17 + l, (co, si, -3.5 * l, -si, co, 2.25 * l), 0.1, 0.5, (250, 10, 30),
                                                (20, 200, 90), (5, 5, 120)) for l in range(N_LAYERS)])

    def timed(call):
        torch.cuda.synchronize()
        for _ in range(WARM):
            call()
        torch.cuda.synchronize()
        st.timer_begin()
        for _ in range(ITER):
            call()
        return 1e3 * st.timer_end() / ITER

    def texture(tab):
        rc = st.lib.ArapFlow_Texture(st.handle, W, H, N_LAYERS, p(d_rgb), p(d_masks), tab, p(out1))
        assert rc == 0, rc

    def line(tab):
        texture(tab)
        rc = st.lib.ArapFlow_WarpLayers(st.handle, W, H, N_LAYERS, p(out1), p(d_masks), p(d_flows), p(out2), p(mask2), None,
                                        None, None, p(scratch))
        assert rc == 0, rc

    us = {}
    for kind, name in enumerate(pipeline.TEX_KINDS):
        tab = table(kind)
        us[name] = timed(lambda: texture(tab))
    tab = table(pipeline.TEX_KINDS.index("noise"))
    us_line = timed(lambda: line(tab))
    bytes_px = N_LAYERS + 3 + 3
    print(json.dumps(dict(what="ArapFlow_Texture per kind; texture + layered warp of a tex line (noise)", W=W, H=H,
                          layers=N_LAYERS, calls=ITER, us_per_call=us, us_per_tex_line=us_line,
                          algorithmic_bytes=W * H * bytes_px)))
    st.close()


if __name__ == "__main__":
    main()
