#!/usr/bin/env python3
"""Device time of the track scorer and of flow chaining (profiles/track_score/README.md).

ArapFlow_TrackScore and ArapFlow_ChainFlows (without and with bwd) at F = 5 frames (L = 4 links on 854x480 flows) for
P = 4096 and P = 854 * 480 points, and the two yardsticks measured in the same run on the same stream:
  floor   the same call at P = 1, F = 2 (L = 1): what a call costs that moves no data -- the clear of the table and one launch
  copy    a device-to-device hipMemcpyAsync of 256 MiB, whose rate (read + written bytes over time) is the achieved HBM rate
          the scorer's 18 bytes per point-frame (two positions, two flags) are set against
Each figure is the median (smallest, largest) of WINDOWS windows of ITER calls after WARM warm-up rounds, device times with
the library's events (ArapFlow_TimerBegin / End) on the state's stream; then one call per configuration under the
per-kernel timer (ArapFlow_SetKernelTiming) for the kernel alone.  Prints one JSON line.  For a kernel table run it under
the profiler, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/profile_track_score.py --only tscore --points 409920
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARM, ITER, WINDOWS = 20, 1000, 5
W, H, NF = 854, 480, 5
CONFIGS = ("tscore", "chain", "chain_bwd")
COPY_BYTES = 256 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=CONFIGS + ("copy",), default=None)
    ap.add_argument("--points", type=int, nargs="*", default=[4096, W * H])
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

    def device_us(call, iters=ITER):
        torch.cuda.synchronize()
        for _ in range(WARM):
            call()
        torch.cuda.synchronize()
        times = []
        for _ in range(WINDOWS):
            st.timer_begin()
            for _ in range(iters):
                call()
            times.append(1e3 * st.timer_end() / iters)
        times.sort()
        return dict(median=times[len(times) // 2], min=times[0], max=times[-1])

    def kernel_us(call, name):
        st.set_kernel_timing(True)
        call()
        got = st.kernel_time(name)
        st.set_kernel_timing(False)
        return None if got is None else 1e3 * got[0]

    flows = up((rng.normal(size=(NF - 1, H, W, 2)) * 3).astype(np.float32))
    bwd = up((-flows.cpu().numpy() + rng.normal(size=(NF - 1, H, W, 2)) * 0.1).astype(np.float32))
    res, kern, check = {}, {}, {}
    for P in [1] + args.points:
        nf = 2 if P == 1 else NF
        gt_pos = (rng.uniform(0, 1, (nf, P, 2)) * [W - 1, H - 1]).astype(np.float32)
        est_pos = (gt_pos + rng.normal(size=gt_pos.shape) * 3).astype(np.float32)
        d_gp, d_ep = up(gt_pos), up(est_pos)
        d_go = up((rng.random((nf, P)) < 0.15).astype(np.uint8) * 255)
        d_eo = up((rng.random((nf, P)) < 0.15).astype(np.uint8) * 255)
        table = torch.empty((nf, 3, 16), dtype=torch.int64, device="cuda")
        d_pts = up(gt_pos[0])
        pos = torch.empty((nf, P, 2), dtype=torch.float32, device="cuda")
        occ = torch.empty((nf, P), dtype=torch.uint8, device="cuda")

        def tscore():
            rc = lib.ArapFlow_TrackScore(st.handle, nf, P, p(d_gp), p(d_go), p(d_ep), p(d_eo), 1.0, 1.0, p(table))
            assert rc == 0, rc

        def chain(back=None):
            rc = lib.ArapFlow_ChainFlows(st.handle, W, H, nf - 1, p(flows), p(back), P, p(d_pts), p(pos), p(occ))
            assert rc == 0, rc
        tag = "floor" if P == 1 else "P%d" % P
        for name, call, kname in (("tscore", tscore, "k_track_score"), ("chain", chain, "k_chain_flows"),
                                  ("chain_bwd", lambda: chain(bwd), "k_chain_flows")):
            if args.only not in (None, name):
                continue
            res["%s_%s" % (name, tag)] = device_us(call)
            kern["%s_%s" % (name, tag)] = kernel_us(call, kname)
        if args.only in (None, "tscore"):
            check[tag] = [int(v) for v in table.cpu().numpy().view(np.uint64)[:, 0, 0]]      # valid points, then point-frames per frame
    out = dict(what="ArapFlow_TrackScore / ArapFlow_ChainFlows (chain_bwd: with the forward-backward check), F = %d, flows %dx%d, "
                    "microseconds per call: median, smallest and largest of %d windows of %d calls; floor: the call at P = 1; "
                    "kernel: the kernel alone, one call under the per-kernel timer" % (NF, W, H, WINDOWS, ITER),
               us=res, kernel_us=kern, count_per_frame=check)
    if args.only in (None, "copy"):
        src = torch.empty(COPY_BYTES, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)

        def copy():
            rc = hip.hipMemcpyAsync(p(dst), p(src), COPY_BYTES, 3, stream)       # 3: device to device
            assert rc == 0, rc
        t = device_us(copy, iters=50)
        rate = 2 * COPY_BYTES / (t["median"] * 1e-6)                             # bytes read + written per second
        out["copy_256MiB_us"] = t
        out["hbm_bytes_per_s"] = rate
        out["tscore_bytes_at_hbm_rate_us"] = {"P%d" % P: 18 * (NF - 1) * P / rate * 1e6 for P in args.points}
    print(json.dumps(out))
    st.close()


if __name__ == "__main__":
    main()
