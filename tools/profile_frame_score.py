#!/usr/bin/env python3
"""Device time of the frame scorer (profiles/frame_score/README.md).

ArapFlow_FrameScore at 854x480 for n = 1 and 8 pairs and at 1920x1080 for one, without optional planes (`none`) and with
occ, dist, skip and obj (`all`); a call on one 1x1 pair (`empty`), the fixed cost of the clear and the launch -- and, as the
yardstick measured in the same run, a device-to-device hipMemcpyAsync of as many bytes as the call reads (`copy_none`: 6
bytes a pixel, `copy_all`: 11), which moves every byte twice.  Each ITER times after WARM warm-up rounds, device times with
the library's events (ArapFlow_TimerBegin / End) on the state's stream; then one call per configuration under the
per-kernel timer (ArapFlow_SetKernelTiming) for k_frame_score alone, without the clear of the table.  Prints one JSON
line.  For a kernel table run it under the profiler, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/profile_frame_score.py --only all
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARM, ITER = 3, 20
SIZES = ((854, 480, 1), (854, 480, 8), (1920, 1080, 1))
CONFIGS = ("none", "all")
BYTES = dict(none=6, all=11)                 # read per pixel: two frames of 3 bytes; occ 1, dist 2, skip 1, obj 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=CONFIGS + ("copy",), default=None)
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
        got = st.kernel_time("k_frame_score")
        st.set_kernel_timing(False)
        return None if got is None else 1e3 * got[0]

    res, kern, tables = {}, {}, {}
    for W, H, n in SIZES + ((1, 1, 1),):
        tag = "empty" if W == 1 else "%dx%d_n%d" % (W, H, n)
        ref = rng.integers(0, 256, (n, H, W, 3)).astype(np.uint8)
        est = np.clip(ref.astype(np.int16) + rng.integers(-6, 7, ref.shape), 0, 255).astype(np.uint8)
        d_ref, d_est = up(ref), up(est)
        d_occ = up((rng.random((n, H, W)) < 0.1).astype(np.uint8) * 255)
        d_dist = up(rng.integers(0, 30000, (n, H, W)).astype(np.uint16).view(np.int16))
        d_skip = up((rng.random((n, H, W)) < 0.02).astype(np.uint8) * 255)
        d_obj = up((rng.random((n, H, W)) < 0.7).astype(np.uint8) * 255)
        table = torch.empty((n, 9, 7), dtype=torch.int64, device="cuda")
        src = torch.empty(n * H * W * BYTES["all"], dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        for name in CONFIGS:
            if args.only not in (None, name) or (W == 1 and name != "none"):
                continue
            planes = [None] * 4 if name == "none" else [p(d_occ), p(d_dist), p(d_skip), p(d_obj)]

            def score():
                rc = lib.ArapFlow_FrameScore(st.handle, W, H, n, p(d_ref), p(d_est), *planes, p(table), None)
                assert rc == 0, rc
            key = tag if W == 1 else "%s_%s" % (name, tag)
            res[key] = device_us(score)
            kern[key] = kernel_us(score)
            tables[key] = [int(v) for v in table.cpu().numpy().view(np.uint64).sum(axis=0)[0, [0, 1, 4, 5]]]
        if args.only in (None, "copy") and W != 1:
            for name in CONFIGS:
                def copy():
                    rc = hip.hipMemcpyAsync(p(dst), p(src), n * H * W * BYTES[name], 3, stream)       # 3: device to device
                    assert rc == 0, rc
                res["copy_%s_%s" % (name, tag)] = device_us(copy)
    ratio = {k: res[k] / res["copy_" + k] for k in res if "copy_" + k in res}
    print(json.dumps(dict(what="ArapFlow_FrameScore (none: no optional plane; all: occ, dist, skip, obj; empty: one 1x1 pair) against a "
                               "device-to-device hipMemcpyAsync of the bytes the call reads, microseconds per call; kernel: "
                               "k_frame_score alone, one call under the per-kernel timer; ratio: call / copy",
                          calls=ITER, us=res, kernel_us=kern, ratio=ratio, count_sse_windows_ssim_sum_of_all=tables)))
    st.close()


if __name__ == "__main__":
    main()
