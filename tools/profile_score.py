#!/usr/bin/env python3
"""Device time of the flow scorer (profiles/score/README.md).

ArapFlow_FlowScore at 854x480 for n = 1 and 8 pairs, without optional planes (`none`), with occ, dist and skip (`all`) and
with all three and the error map (`all_err`) -- and, as the yardstick measured in the same run, a device-to-device
hipMemcpyAsync of as many bytes as the call reads (`copy_none`: 16 bytes a pixel, `copy_all`: 20), which moves every byte
twice.  Each ITER times after WARM warm-up rounds, device times with the library's events (ArapFlow_TimerBegin / End) on
the state's stream; then one call per configuration under the per-kernel timer (ArapFlow_SetKernelTiming) for k_flow_score
alone, without the clear of the table.  Prints one JSON line.  For a kernel table run it under the profiler, in a run of
its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/profile_score.py --only all --pairs 8
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARM, ITER = 3, 20
W, H = 854, 480
CONFIGS = ("none", "all", "all_err")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=CONFIGS + ("copy",), default=None)
    ap.add_argument("--pairs", type=int, nargs="*", default=[1, 8])
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
        got = st.kernel_time("k_flow_score")
        st.set_kernel_timing(False)
        return None if got is None else 1e3 * got[0]

    res, kern, tables = {}, {}, {}
    for n in args.pairs:
        gt = (rng.normal(size=(n, H, W, 2)) * 12).astype(np.float32)
        est = (gt + rng.normal(size=gt.shape) * 1.5).astype(np.float32)
        d_gt, d_est = up(gt), up(est)
        d_occ = up((rng.random((n, H, W)) < 0.1).astype(np.uint8) * 255)
        d_dist = up(rng.integers(0, 30000, (n, H, W)).astype(np.uint16).view(np.int16))
        d_skip = up((rng.random((n, H, W)) < 0.02).astype(np.uint8) * 255)
        table = torch.empty((n, 10, 8), dtype=torch.int64, device="cuda")
        err = torch.empty((n, H, W), dtype=torch.float32, device="cuda")
        src = torch.empty(n * H * W * 20, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        for name in CONFIGS:
            if args.only not in (None, name):
                continue
            planes = [None, None, None] if name == "none" else [p(d_occ), p(d_dist), p(d_skip)]

            def score():
                rc = lib.ArapFlow_FlowScore(st.handle, W, H, n, p(d_gt), p(d_est), *planes, p(table), p(err) if name == "all_err" else None)
                assert rc == 0, rc
            res["%s_n%d" % (name, n)] = device_us(score)
            kern["%s_n%d" % (name, n)] = kernel_us(score)
            tables["%s_n%d" % (name, n)] = [int(v) for v in table.cpu().numpy().view(np.uint64).sum(axis=0)[0, :2]]
        if args.only in (None, "copy"):
            for name, per_pixel in (("copy_none", 16), ("copy_all", 20)):
                def copy():
                    rc = hip.hipMemcpyAsync(p(dst), p(src), n * H * W * per_pixel, 3, stream)       # 3: device to device
                    assert rc == 0, rc
                res["%s_n%d" % (name, n)] = device_us(copy)
    ratio = {k: res[k] / res["copy_" + ("none" if k.startswith("none") else "all") + k[k.rindex("_n"):]]
             for k in res if not k.startswith("copy") and "copy_none" + k[k.rindex("_n"):] in res}
    print(json.dumps(dict(what="ArapFlow_FlowScore (none: no optional plane; all: occ, dist, skip; all_err: and the error map) "
                               "against a device-to-device hipMemcpyAsync of the bytes the call reads, microseconds per call; "
                               "kernel: k_flow_score alone, one call under the per-kernel timer; ratio: call / copy",
                          W=W, H=H, calls=ITER, us=res, kernel_us=kern, ratio=ratio, count_and_sum_of_all=tables)))
    st.close()


if __name__ == "__main__":
    main()
