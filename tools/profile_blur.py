#!/usr/bin/env python3
"""Device time of a motion-blurred frame (profiles/blur/README.md).

ArapFlow_BlurLayers at 854x480 on a frame of three overlapping elliptic layers (those of tools/profile_texture.py), a
shutter of 0.5 around t = 1, S in {1, 9, 32} samples, with and without a moving camera over a background picture -- and
the same frames made the way the library could make them before the call existed:
  warps       S ArapFlow_WarpLayers calls (RGB and mask) on flows interpolated beforehand and resident on the device:
              device time only, nothing uploaded, downloaded or averaged
  warps_host  the same plus what a host that averages images has to do per sample: upload the interpolated flows,
              download RGB and mask, add them in numpy (without bg: sampling the picture on the host is not counted);
              wall clock
Each ITER times after WARM warm-up rounds; device times with the library's events (ArapFlow_TimerBegin / End).  Prints one
JSON line.  For a kernel table run ONE configuration under the profiler, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/profile_blur.py --only fused --samples 9 --bg 1
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARM, ITER = 3, 20
W, H, N_LAYERS = 854, 480, 3
CENTRE, SHUTTER = 1.0, 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["fused", "warps", "warps_host"], default=None)
    ap.add_argument("--samples", type=int, nargs="*", default=[1, 9, 32])
    ap.add_argument("--bg", type=int, nargs="*", default=[0, 1])
    args = ap.parse_args()
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
    bg = rng.integers(0, 256, (H + 40, W + 60, 3)).astype(np.uint8)
    Ma = (C.c_float * 6)(1.0, 0.0, 20.0, 0.0, 1.0, 15.0)
    Mb = (C.c_float * 6)(0.9986295104, -0.0523359552, 24.5, 0.0523359552, 0.9986295104, 12.25)        # 3 degrees on
    st = opt.State()
    lib = st.lib
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_rgb, d_masks, d_flows, d_bg = up(rgb), up(masks), up(flows), up(bg)
    out_rgb = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    out_a = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())
    scr_layers = torch.empty(int(lib.ArapFlow_WarpLayersScratchBytes(W, H, N_LAYERS)), dtype=torch.uint8, device="cuda")

    def device_us(call):
        torch.cuda.synchronize()
        for _ in range(WARM):
            call()
        torch.cuda.synchronize()
        st.timer_begin()
        for _ in range(ITER):
            call()
        return 1e3 * st.timer_end() / ITER

    def wall_us(call):
        for _ in range(WARM):
            call()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(ITER):
            call()
        torch.cuda.synchronize()
        return 1e6 * (time.perf_counter() - t0) / ITER

    res = {}
    for S in args.samples:
        times = pipeline.blur_times(CENTRE, SHUTTER, S)
        mixed = [((np.float32(1.0) - t) * np.zeros_like(flows) + t * flows).astype(np.float32) for t in times]
        scratch = torch.empty(int(lib.ArapFlow_BlurLayersScratchBytes(W, H, N_LAYERS, S)), dtype=torch.uint8, device="cuda")
        if args.only in (None, "fused"):
            for with_bg in args.bg:
                def fused():
                    rc = lib.ArapFlow_BlurLayers(st.handle, W, H, N_LAYERS, p(d_rgb), p(d_masks), None, p(d_flows), CENTRE, SHUTTER,
                                                 S, p(d_bg) if with_bg else None, bg.shape[1], bg.shape[0], Ma, Mb, p(out_rgb),
                                                 p(out_a), p(scratch))
                    assert rc == 0, rc
                res["fused_S%d_%s" % (S, "bg" if with_bg else "nobg")] = device_us(fused)
        if args.only in (None, "warps"):
            d_mixed = [up(f) for f in mixed]

            def warps():
                for f in d_mixed:
                    rc = lib.ArapFlow_WarpLayers(st.handle, W, H, N_LAYERS, p(d_rgb), p(d_masks), p(f), p(out_rgb), p(out_a), None,
                                                 None, None, p(scr_layers))
                    assert rc == 0, rc
            res["warps_S%d" % S] = device_us(warps)
            del d_mixed
        if args.only in (None, "warps_host"):
            def warps_host():
                total, cnt = np.zeros((H, W, 3), np.uint32), np.zeros((H, W), np.uint32)
                for f in mixed:
                    d = up(f)
                    rc = lib.ArapFlow_WarpLayers(st.handle, W, H, N_LAYERS, p(d_rgb), p(d_masks), p(d), p(out_rgb), p(out_a), None,
                                                 None, None, p(scr_layers))
                    assert rc == 0, rc
                    torch.cuda.synchronize()
                    total += out_rgb.cpu().numpy()
                    cnt += out_a.cpu().numpy() != 0
                return ((2 * total + S) // (2 * S)).astype(np.uint8), ((2 * 255 * cnt + S) // (2 * S)).astype(np.uint8)
            res["warps_host_S%d" % S] = wall_us(warps_host)
    print(json.dumps(dict(what="ArapFlow_BlurLayers (fused) against S ArapFlow_WarpLayers calls (warps: device only; warps_host: "
                               "with uploads, downloads and the host mean, wall clock), microseconds per blurred frame",
                          W=W, H=H, layers=N_LAYERS, centre=CENTRE, shutter=SHUTTER, calls=ITER, us=res)))
    st.close()


if __name__ == "__main__":
    main()
