#!/usr/bin/env python3
"""Kernel times of one layered step call against the calls it replaces (profiles/mid_layers/README.md).

Run it under the profiler, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/profile_layers_step.py
One ArapFlow_WarpLayersStep call with every output on, 3 layers at 854x480, alternating with n ArapFlow_WarpStep calls
plus one ArapFlow_WarpLayers call (RGB, mask, forward occlusion) on the same inputs: those give the per-layer steps and
the composite, but no step occlusion.  ITER rounds after WARM warm-up rounds.  Also prints device-event times of both.
Inputs: tools/profile_layers.py's frame for state a; state b moves every layer but the top one on towards the next
label's centroid and deforms a little further.
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
WARM, ITER = 5, 50


def inputs():
    import profile_layers
    rgb, masks, fa = profile_layers.inputs()
    fb = 1.3 * fa
    cen = [np.argwhere(m == 0).mean(0)[::-1] for m in masks]
    for l in range(len(masks) - 1):
        fb[l] += np.round(0.15 * (cen[l + 1] - cen[l])).astype(np.float32)
        fb[l][masks[l] != 0] = 0
    return rgb, masks, fa, fb.astype(np.float32)


def main():
    import torch
    from arap_flow_amd import opt
    rgb, masks, fa, fb = inputs()
    n, H, W = masks.shape
    st = opt.State()
    lib, dev = st.lib, "cuda"
    d_rgb, d_msk = torch.from_numpy(rgb).to(dev), torch.from_numpy(masks).to(dev)
    d_a, d_b = torch.from_numpy(fa).to(dev), torch.from_numpy(fb).to(dev)
    u8 = lambda *s: torch.empty(*s, dtype=torch.uint8, device=dev)
    o_rgb, o_msk, o_occ = u8(H, W, 3), u8(H, W), u8(H, W)
    o_step = torch.empty(H, W, 2, dtype=torch.float32, device=dev)
    scr_s = u8(int(lib.ArapFlow_WarpLayersStepScratchBytes(W, H, n)))
    scr_l = u8(int(lib.ArapFlow_WarpLayersScratchBytes(W, H, n)))
    p = lambda t: t.data_ptr()
    torch.cuda.synchronize()

    def layered_step():
        rc = lib.ArapFlow_WarpLayersStep(st.handle, W, H, n, p(d_rgb), p(d_msk), p(d_a), p(d_b), p(o_rgb), p(o_msk),
                                         p(o_step), p(o_occ), p(scr_s))
        assert rc == 0, rc

    def replaced():
        for l in range(n):
            rc = lib.ArapFlow_WarpStep(st.handle, W, H, p(d_rgb), p(d_msk[l]), p(d_a[l]), p(d_b[l]), p(o_rgb), p(o_msk),
                                       p(o_step))
            assert rc == 0, rc
        rc = lib.ArapFlow_WarpLayers(st.handle, W, H, n, p(d_rgb), p(d_msk), p(d_a), p(o_rgb), p(o_msk), None, None,
                                     p(o_occ), p(scr_l))
        assert rc == 0, rc

    t = dict(layered_step=[], replaced=[])
    for it in range(WARM + ITER):
        for name, fn in (("layered_step", layered_step), ("replaced", replaced)):
            st.timer_begin()
            fn()
            ms = st.timer_end()
            if it >= WARM:
                t[name].append(ms)
    torch.cuda.synchronize()
    out = {k: dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)))
           for k, v in t.items()}
    out.update(W=W, H=H, layers=n, rounds=ITER,
               note="device events around one layered step call / n WarpStep calls (each allocates and waits) + one "
                    "WarpLayers call")
    print(json.dumps(out))
    st.close()


if __name__ == "__main__":
    main()
