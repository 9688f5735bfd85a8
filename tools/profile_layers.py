#!/usr/bin/env python3
"""Kernel times of the layered warp against n single-layer warps on the same inputs (profiles/occ_layers/README.md).

Run it under the profiler, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/profile_layers.py
One ArapFlow_WarpLayers call with every output on, 3 layers at 854x480, alternating with three ArapFlow_WarpEx calls
with every output on; ITER rounds after WARM warm-up rounds.  Also prints device-event times of both (per round).
Inputs: synth.make_frame(854, 480, 3, K=3) segment masks, a smooth 2-pixel deformation per layer, and a whole-pixel shift
of every layer but the top one 0.8 of the way to the next label's centroid, so that the layers overlap.
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARM, ITER = 5, 50


def inputs(W=854, H=480, seed=3):
    from arap_flow_amd import synth
    frame = synth.make_frame(W, H, seed, K=3, fd=2)
    masks = np.stack([s["mask_red"] for s in synth.segment_masks(frame)])
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    flows = np.zeros(masks.shape + (2,), np.float32)
    cen = [np.argwhere(m == 0).mean(0)[::-1] for m in masks]
    for l in range(len(masks)):
        flows[l, ..., 0] = 2.0 * np.sin(xs / 37.0 + l) * np.cos(ys / 29.0)
        flows[l, ..., 1] = 2.0 * np.cos(xs / 31.0) * np.sin(ys / 41.0 + l)
        if l + 1 < len(masks):
            flows[l] += np.round(0.8 * (cen[l + 1] - cen[l])).astype(np.float32)
        flows[l][masks[l] != 0] = 0
    return frame["rgb"], masks, flows


def main():
    import torch
    from arap_flow_amd import opt
    rgb, masks, flows = inputs()
    n, H, W = masks.shape
    st = opt.State()
    lib, dev = st.lib, "cuda"
    d_rgb = torch.from_numpy(rgb).to(dev)
    d_msk = torch.from_numpy(masks).to(dev)
    d_flo = torch.from_numpy(flows).to(dev)
    u8 = lambda *s: torch.empty(*s, dtype=torch.uint8, device=dev)
    o_rgb, o_msk, o_obwd, o_occ = u8(H, W, 3), u8(H, W), u8(H, W), u8(H, W)
    o_bwd = torch.empty(H, W, 2, dtype=torch.float32, device=dev)
    scr_l = u8(int(lib.ArapFlow_WarpLayersScratchBytes(W, H, n)))
    scr_e = u8(int(lib.ArapFlow_WarpExScratchBytes(W, H)))
    p = lambda t: t.data_ptr()
    torch.cuda.synchronize()

    def layered():
        rc = lib.ArapFlow_WarpLayers(st.handle, W, H, n, p(d_rgb), p(d_msk), p(d_flo), p(o_rgb), p(o_msk), p(o_bwd),
                                     p(o_obwd), p(o_occ), p(scr_l))
        assert rc == 0, rc

    def single():
        for l in range(n):
            rc = lib.ArapFlow_WarpEx(st.handle, W, H, p(d_rgb), p(d_msk[l]), p(d_flo[l]), p(o_rgb), p(o_msk), p(o_bwd),
                                     p(o_obwd), p(o_occ), p(scr_e))
            assert rc == 0, rc

    t = dict(layered=[], single=[])
    for it in range(WARM + ITER):
        for name, fn in (("layered", layered), ("single", single)):
            st.timer_begin()
            fn()
            ms = st.timer_end()
            if it >= WARM:
                t[name].append(ms)
    torch.cuda.synchronize()
    out = {k: dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v))) for k, v in t.items()}
    out.update(W=W, H=H, layers=n, rounds=ITER, note="device events around the enqueue of one layered call / three single calls")
    print(json.dumps(out))
    st.close()


if __name__ == "__main__":
    main()
