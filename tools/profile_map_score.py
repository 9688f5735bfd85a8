#!/usr/bin/env python3
"""Device time of the map scorers (profiles/map_score/README.md).

At 854x480, label maps of three objects and a two-valued occlusion map, for n = 1 and 8 maps:
  hist      ArapFlow_MapScore with m = 0 -- against `copy`, a device-to-device hipMemcpyAsync of the 2 bytes a pixel it reads
            (which moves every byte twice), measured in the same run on the same stream;
  match3    ArapFlow_MapScore with m = 3 thresholds at radius 8: 3 boundary matches a map, 6 distance transforms;
  labels    ArapFlow_LabelScore with L = 3 at radius 8: the same count of matches and transforms;
  empty     ArapFlow_MapScore with m = 0 on one 1x1 map: the fixed cost of the clear and the launch.
Each ITER times after WARM warm-up rounds, device times with the library's events (ArapFlow_TimerBegin / End) on the
state's stream; then one call per configuration under the per-kernel timer (ArapFlow_SetKernelTiming): the time and the
launches of every kernel of the call, among them k_seg_cols and k_seg_rows, the distance passes of ArapFlow_SegMaps' frame-1
half (profiles/seg/), so `transform_us` = (k_seg_cols + k_seg_rows) / transforms is the yardstick of match3 and labels.
With ARAPOPT_MSCORE_PLAIN=1 in the environment `hist` runs the plain variant of k_mscore_hist, one LDS atomic per pixel and
no wave aggregation: run the tool twice, with `--only hist`, for the contention comparison.  Prints one JSON line.  For a
kernel table run it under the profiler, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/profile_map_score.py --only labels
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARM, ITER = 3, 20
W, H, L, RADIUS, THR = 854, 480, 3, 8, (64, 128, 192)
CONFIGS = ("hist", "match3", "labels")
KERNELS = ("k_mscore_hist", "k_mscore_labels", "k_mscore_sets", "k_seg_cols", "k_seg_rows", "k_mscore_hits")


def scene(n, rng):
    """three discs on the ground as labels, the estimate two pixels to the right; the union as a 0 / 255 map"""
    ys, xs = np.mgrid[0:H, 0:W]
    gt = np.zeros((n, H, W), np.uint8)
    for i in range(n):
        for k in (1, 2, 3):
            cx, cy, r = rng.integers(100, W - 100), rng.integers(100, H - 100), rng.integers(40, 90)
            gt[i][(xs - cx) ** 2 + (ys - cy) ** 2 <= r * r] = k
    est = np.roll(gt, 2, axis=2)
    return gt, est, (gt != 0).astype(np.uint8) * 255, (est != 0).astype(np.uint8) * 255


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
    thr = (C.c_uint * len(THR))(*THR)

    def device_us(call):
        torch.cuda.synchronize()
        for _ in range(WARM):
            call()
        torch.cuda.synchronize()
        st.timer_begin()
        for _ in range(ITER):
            call()
        return 1e3 * st.timer_end() / ITER

    def kernels_us(call):
        st.set_kernel_timing(True)
        call()
        torch.cuda.synchronize()
        got = {k: st.kernel_time(k) for k in KERNELS}
        st.set_kernel_timing(False)
        return {k: dict(us=1e3 * v[0], launches=int(v[1])) for k, v in got.items() if v is not None}

    res, kern, sums = {}, {}, {}
    for n in (1, 8):
        gt, est, occ, sc = (up(a) for a in scene(n, rng))
        table = torch.empty((n, L + 1, 8), dtype=torch.int64, device="cuda")
        hist = torch.empty((n, 2, 256), dtype=torch.int64, device="cuda")
        match = torch.empty((n, len(THR), 4), dtype=torch.int64, device="cuda")
        scratch = torch.empty(int(lib.ArapFlow_MapScoreScratchBytes(W, H)), dtype=torch.uint8, device="cuda")
        src = torch.empty(n * H * W * 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)

        def run_hist():
            assert lib.ArapFlow_MapScore(st.handle, W, H, n, p(occ), p(sc), None, 0, None, 0, p(hist), None, None) == 0

        def run_match3():
            assert lib.ArapFlow_MapScore(st.handle, W, H, n, p(occ), p(sc), None, len(THR), thr, RADIUS, p(hist), p(match), p(scratch)) == 0

        def run_labels():
            assert lib.ArapFlow_LabelScore(st.handle, W, H, n, L, RADIUS, p(gt), p(est), None, p(table), p(scratch)) == 0

        def copy():
            assert hip.hipMemcpyAsync(p(dst), p(src), n * H * W * 2, 3, stream) == 0       # 3: device to device
        for name, call in (("hist", run_hist), ("match3", run_match3), ("labels", run_labels)):
            if args.only not in (None, name):
                continue
            key = "%s_n%d" % (name, n)
            res[key] = device_us(call)
            kern[key] = kernels_us(call)
            torch.cuda.synchronize()
            out = table if name == "labels" else hist
            sums[key] = int(out.cpu().numpy().view(np.uint64).sum())
        if args.only in (None, "copy"):
            res["copy_n%d" % n] = device_us(copy)
    if args.only in (None, "hist"):
        one = torch.zeros(16, dtype=torch.uint8, device="cuda")
        hist1 = torch.empty((1, 2, 256), dtype=torch.int64, device="cuda")

        def run_empty():
            assert lib.ArapFlow_MapScore(st.handle, 1, 1, 1, p(one), p(one), None, 0, None, 0, p(hist1), None, None) == 0
        res["empty"] = device_us(run_empty)
    ratio = {k: res[k] / res["copy_" + k.split("_")[1]] for k in res if k.startswith("hist_") and "copy_" + k.split("_")[1] in res}
    transform = {}
    for k, v in kern.items():
        if "k_seg_cols" in v:
            transform[k] = (v["k_seg_cols"]["us"] + v["k_seg_rows"]["us"]) / v["k_seg_cols"]["launches"]
    print(json.dumps(dict(what="ArapFlow_MapScore (hist: m = 0; match3: m = 3, radius 8) and ArapFlow_LabelScore (labels: L = 3, "
                               "radius 8) at 854x480 for n = 1 and 8, microseconds per call; copy: a device-to-device "
                               "hipMemcpyAsync of the 2 bytes a pixel hist reads; empty: one 1x1 map; kernels: every kernel of one "
                               "call under the per-kernel timer; transform_us: one distance transform (k_seg_cols + k_seg_rows); "
                               "ratio: hist / copy",
                          plain=os.environ.get("ARAPOPT_MSCORE_PLAIN") == "1", calls=ITER, us=res, kernels=kern,
                          transform_us=transform, ratio=ratio, sum_of_output=sums)))
    st.close()


if __name__ == "__main__":
    main()
