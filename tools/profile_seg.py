#!/usr/bin/env python3
"""Device time of the segment maps (profiles/seg/README.md).

ArapFlow_SegMaps at 854x480 on a frame of three overlapping elliptic layers (those of tools/profile_blur.py), tau = 1, at
radius 16 and 140, all six outputs (`both`) and the frame-1 outputs alone (`frame1`: nothing is rasterised) -- and, as the
yardstick, ArapFlow_WarpLayers with out_mask and out_bwd on the same inputs (`warp_layers`): the rasteriser work the
frame-2 side shares.  Each ITER times after WARM warm-up rounds, device times with the library's events
(ArapFlow_TimerBegin / End); then one round per configuration with the per-kernel timer (ArapFlow_SetKernelTiming) for the
time of every pass.  Prints one JSON line.  For a kernel table run ONE configuration under the profiler, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/profile_seg.py --only both --radius 140
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARM, ITER = 3, 20
W, H, N_LAYERS = 854, 480, 3
KERNELS = ("k_seg_index1", "k_layers_raster", "k_layers_keys", "k_seg_index2", "k_warp_resolve", "k_seg_jump", "k_seg_cols",
           "k_seg_rows")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["both", "frame1", "warp_layers"], default=None)
    ap.add_argument("--radius", type=int, nargs="*", default=[16, 140])
    args = ap.parse_args()
    import torch
    from arap_flow_amd import opt
    ys, xs = np.mgrid[0:H, 0:W]
    ell = lambda cx, cy, rx, ry: np.where(((xs - cx) / rx) ** 2 + ((ys - cy) / ry) ** 2 <= 1, 0, 255).astype(np.uint8)
    masks = np.stack([ell(0.35 * W, 0.5 * H, 0.3 * W, 0.45 * H), ell(0.55 * W, 0.4 * H, 0.25 * W, 0.35 * H),
                      ell(0.7 * W, 0.6 * H, 0.22 * W, 0.38 * H)])
    flows = np.stack([np.stack([6.0 + 0.01 * (ys - H / 2) + l, -3.0 + 0.01 * (xs - W / 2) - l], -1)
                      for l in range(N_LAYERS)]).astype(np.float32)
    st = opt.State()
    lib = st.lib
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_masks, d_flows = up(masks), up(flows)
    new = lambda dt: torch.empty((H, W), dtype=dt, device="cuda")
    outs = [new(torch.uint8) for _ in range(4)] + [new(torch.int16) for _ in range(2)]      # idx1 idx2 mb1 mb2 dist1 dist2
    out_mask, out_bwd = new(torch.uint8), torch.empty((H, W, 2), dtype=torch.float32, device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())
    scr_layers = torch.empty(int(lib.ArapFlow_WarpLayersScratchBytes(W, H, N_LAYERS)), dtype=torch.uint8, device="cuda")
    scr_seg = torch.empty(int(lib.ArapFlow_SegMapsScratchBytes(W, H, N_LAYERS)), dtype=torch.uint8, device="cuda")

    def device_us(call):
        torch.cuda.synchronize()
        for _ in range(WARM):
            call()
        torch.cuda.synchronize()
        st.timer_begin()
        for _ in range(ITER):
            call()
        return 1e3 * st.timer_end() / ITER

    def per_kernel_us(call):
        st.set_kernel_timing(True)
        call()
        got = {k: st.kernel_time(k) for k in KERNELS}
        st.set_kernel_timing(False)
        return {k: dict(us=1e3 * v[0], launches=v[1]) for k, v in got.items() if v is not None}

    res, kern = {}, {}
    if args.only in (None, "warp_layers"):
        def warp_layers():
            rc = lib.ArapFlow_WarpLayers(st.handle, W, H, N_LAYERS, None, p(d_masks), p(d_flows), None, p(out_mask), p(out_bwd), None,
                                         None, p(scr_layers))
            assert rc == 0, rc
        res["warp_layers_bwd"] = device_us(warp_layers)
    for radius in args.radius:
        for name, frame2 in (("both", True), ("frame1", False)):
            if args.only not in (None, name):
                continue
            o = [p(t) if frame2 or k % 2 == 0 else None for k, t in enumerate(outs)]

            def seg():
                rc = lib.ArapFlow_SegMaps(st.handle, W, H, N_LAYERS, p(d_masks), p(d_flows), None, None, 1.0, radius, *o, p(scr_seg))
                assert rc == 0, rc
            res["%s_r%d" % (name, radius)] = device_us(seg)
            kern["%s_r%d" % (name, radius)] = per_kernel_us(seg)
    near = outs[4].cpu().numpy().view(np.uint16)
    print(json.dumps(dict(what="ArapFlow_SegMaps (both: six outputs; frame1: idx1, mb1, dist1) against ArapFlow_WarpLayers with "
                               "out_mask and out_bwd, microseconds per call; kernels: one call under the per-kernel timer",
                          W=W, H=H, layers=N_LAYERS, tau=1.0, calls=ITER, us=res, kernels=kern,
                          boundary_pixels=int((outs[2].cpu().numpy() != 0).sum()), reached=int((near != 65535).sum()))))
    st.close()


if __name__ == "__main__":
    main()
