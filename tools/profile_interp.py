#!/usr/bin/env python3
"""Device time of frames from flows (profiles/interp/README.md).

ArapFlow_InterpFrames at 854x480 and 1920x1080 for K = 1, 4 and 32 times, without (`fwd`) and with (`bwd`) the backward
flow, on a smooth flow of a few pixels with a noisy tenth -- and, as context measured in the same run, a device-to-device
hipMemcpyAsync of as many bytes as the call reads and writes (`copy`: 6 bytes a pixel of frames, 8 or 16 of flows, 3 K of
output; the K key images of scratch are not counted) and K ArapFlow_Warp calls at the same size (`warp`).  Each ITER
times after WARM warm-up rounds, device times with the library's events (ArapFlow_TimerBegin / End) on the state's
stream; then one call per configuration under the per-kernel timer (ArapFlow_SetKernelTiming) for k_interp_splat and
k_interp_gather alone, without the clear of the keys.  Prints one JSON line.  For a kernel table run it under the
profiler, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/profile_interp.py --only bwd --size 854x480 --times 4
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARM, ITER = 3, 20
SIZES = ((854, 480), (1920, 1080))
TIMES = (1, 4, 32)
CONFIGS = ("fwd", "bwd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=CONFIGS, default=None)
    ap.add_argument("--size", default=None, help="WxH: that size alone")
    ap.add_argument("--times", type=int, default=None, help="that K alone")
    args = ap.parse_args()
    import torch
    from arap_flow_amd import opt
    st = opt.State()
    lib = st.lib
    own = torch.cuda.Stream()                    # the state's stream, so that the copy is between the same events
    st.set_stream(own)
    stream = C.c_void_p(own.cuda_stream)
    torch.cuda.synchronize()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    rng = np.random.default_rng(0)
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()

    def device_us(call):
        torch.cuda.synchronize()
        for _ in range(WARM):
            call()
        torch.cuda.synchronize()
        st.timer_begin()
        for _ in range(ITER):
            call()
        return 1e3 * st.timer_end() / ITER

    def kernel_us(call):
        st.set_kernel_timing(True)
        call()
        got = {k: st.kernel_time(k) for k in ("k_interp_splat", "k_interp_gather")}
        st.set_kernel_timing(False)
        return {k: None if v is None else 1e3 * v[0] for k, v in got.items()}

    res, kern, srcs = {}, {}, {}
    for W, H in SIZES:
        if args.size not in (None, "%dx%d" % (W, H)):
            continue
        N = W * H
        ys, xs = np.mgrid[0:H, 0:W]
        a = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
        b = np.roll(a, (2, 3), (0, 1))
        fwd = np.stack([3 + 2 * np.sin(xs / 40.0), 2 + np.cos(ys / 30.0)], -1)
        fwd += rng.normal(size=fwd.shape) * 3 * (rng.random((H, W, 1)) < 0.1)
        fwd = fwd.astype(np.float32)
        d_a, d_b, d_fwd, d_bwd = up(a), up(b), up(fwd), up(-fwd)
        mask = up(np.zeros((H, W), np.uint8))
        w_rgb, w_mask = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda"), torch.empty((H, W), dtype=torch.uint8, device="cuda")
        w_scratch = torch.empty(int(lib.ArapFlow_WarpScratchBytes(W, H)), dtype=torch.uint8, device="cuda")
        for K in TIMES:
            if args.times not in (None, K):
                continue
            times = (C.c_float * K)(*[(k + 1) / (K + 1.0) for k in range(K)])
            out = torch.empty((K, H, W, 3), dtype=torch.uint8, device="cuda")
            src = torch.empty((K, H, W), dtype=torch.uint8, device="cuda")
            scratch = torch.empty(int(lib.ArapFlow_InterpScratchBytes(W, H, K)), dtype=torch.uint8, device="cuda")
            moved = torch.empty(N * (22 + 3 * K), dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(moved)
            tag = "%dx%d_K%d" % (W, H, K)
            for name in CONFIGS:
                if args.only not in (None, name):
                    continue
                back = p(d_bwd) if name == "bwd" else None

                def interp(want_src=None):
                    rc = lib.ArapFlow_InterpFrames(st.handle, W, H, p(d_a), p(d_b), p(d_fwd), back, K, times, p(out), want_src, p(scratch))
                    assert rc == 0, rc
                key = "%s_%s" % (name, tag)
                res[key] = device_us(interp)
                kern[key] = kernel_us(interp)
                interp(p(src))
                torch.cuda.synchronize()
                v, c = np.unique(src.cpu().numpy(), return_counts=True)
                srcs[key] = {int(x): int(y) for x, y in zip(v, c)}
                nbytes = N * (6 + (16 if name == "bwd" else 8) + 3 * K)

                def copy():
                    rc = hip.hipMemcpyAsync(p(dst), p(moved), nbytes, 3, stream)       # 3: device to device
                    assert rc == 0, rc
                res["copy_" + key] = device_us(copy)

            def warp():
                for _ in range(K):
                    rc = lib.ArapFlow_Warp(st.handle, W, H, p(d_a), p(mask), p(d_fwd), p(w_rgb), p(w_mask), p(w_scratch))
                    assert rc == 0, rc
            if args.only is None:
                res["warp_" + tag] = device_us(warp)
    ratio = {k: res[k] / res["copy_" + k] for k in res if "copy_" + k in res}
    print(json.dumps(dict(what="ArapFlow_InterpFrames (fwd: no backward flow; bwd: with it; K times in one call) against a device-to-device "
                               "hipMemcpyAsync of the bytes the call reads and writes (copy_*) and against K ArapFlow_Warp calls "
                               "(warp_*), microseconds per call; kernel: each kernel alone, one call under the per-kernel timer; "
                               "ratio: call / copy; src: the histogram of the source map",
                          calls=ITER, us=res, kernel_us=kern, ratio=ratio, src=srcs)))
    st.close()


if __name__ == "__main__":
    main()
