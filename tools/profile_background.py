#!/usr/bin/env python3
"""Device time of the moving-background pass (profiles/bg_motion/README.md).

One ArapFlow_Background call with every output on at 854x480 over a 1200x700 picture, a 1.5 degree / 1.01 / (4, -2) px
similarity, on the outputs of one ArapFlow_WarpEx of a synthetic object; ITER calls after WARM warm-up calls, timed with
the library's device events (ArapFlow_TimerBegin / End).  Prints one JSON line: microseconds per call, the bytes the call
streams (inputs read and outputs written once, the picture's gathers not counted) and the rate that makes.  For the
kernel table run it under the profiler, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/profile_background.py

--seq (profiles/bg_seq/README.md): the sequence pass instead.  Frame 1, n = 3 in-between frames and frame 2 at 854x480
over the same picture, the camera at the fractions 4/19, 9/19, 14/19 and 1 of that similarity: ITER ArapFlow_BackgroundSeq
calls with every output on (one k_bg_seq launch each), ITER with the last frame's RGB left out, and as the yardstick ITER
rounds of n + 1 ArapFlow_Background calls for out_rgb1, flow_full and occ_full of the same links (one k_bg_frame1 launch
each, a later frame's cover handed over as a solver mask).  One JSON line with the three times.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARM, ITER = 5, 50
W, H, BW, BH = 854, 480, 1200, 700


def main():
    import torch
    from arap_flow_amd import opt
    rng = np.random.default_rng(0)
    ys, xs = np.mgrid[0:H, 0:W]
    inside = ((xs - 0.45 * W) / (0.22 * W)) ** 2 + ((ys - 0.5 * H) / (0.3 * H)) ** 2 <= 1
    mask = np.where(inside, 0, 255).astype(np.uint8)
    flow = np.stack([6.0 + 0.01 * (ys - H / 2), -3.0 + 0.01 * (xs - W / 2)], -1).astype(np.float32)
    flow[~inside] = 0
    rgb1 = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    bg = rng.integers(0, 256, (BH, BW, 3)).astype(np.uint8)
    st = opt.State()
    r = opt.warp_image_ex(st, rgb1, mask, flow)
    t = np.deg2rad(1.5)
    a, b, cx, cy = 1.01 * np.cos(t), 1.01 * np.sin(t), (W - 1) / 2.0, (H - 1) / 2.0
    M1 = (C.c_float * 6)(1, 0, 170, 0, 1, 110)
    M2 = (C.c_float * 6)(a, -b, 170 + cx - a * cx + b * cy + 4, b, a, 110 + cy - b * cx - a * cy - 2)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    ins = [up(x) for x in (rgb1, mask, r["warped_rgb"], r["warped_mask"], flow, r["occlusion"], r["backward_flow"],
                           r["occlusion_bwd"])]
    dbg = up(bg)
    outs = [torch.empty(s, dtype=d, device="cuda") for s, d in (((H, W, 3), torch.uint8), ((H, W, 3), torch.uint8),
            ((H, W, 2), torch.float32), ((H, W), torch.uint8), ((H, W, 2), torch.float32), ((H, W), torch.uint8))]
    p = lambda x: C.c_void_p(x.data_ptr())

    def call():
        rc = st.lib.ArapFlow_Background(st.handle, W, H, p(dbg), BW, BH, M1, M2, *[p(x) for x in ins], *[p(x) for x in outs])
        assert rc == 0, rc

    torch.cuda.synchronize()
    for _ in range(WARM):
        call()
    torch.cuda.synchronize()
    st.timer_begin()
    for _ in range(ITER):
        call()
    ms = st.timer_end()
    N = W * H
    streamed = N * (2 * (3 + 1 + 8 + 1) + 2 * (3 + 8 + 1))      # per domain: rgb, mask, flow, occ in; rgb, flow, occ out
    us = 1e3 * ms / ITER
    print(json.dumps(dict(what="ArapFlow_Background, every output", W=W, H=H, bg=[BW, BH], calls=ITER, us_per_call=us,
                          streamed_bytes=streamed, streamed_GBps=streamed / us * 1e-3)))
    st.close()


def similarity(tau):
    """the camera at the fraction tau of main()'s similarity, as six floats"""
    t, sc = np.deg2rad(1.5 * tau), 1.01 ** tau
    a, b, cx, cy = sc * np.cos(t), sc * np.sin(t), (W - 1) / 2.0, (H - 1) / 2.0
    return [a, -b, 170 + cx - a * cx + b * cy + 4 * tau, b, a, 110 + cy - b * cx - a * cy - 2 * tau]


def main_seq():
    import torch
    from arap_flow_amd import opt
    rng = np.random.default_rng(0)
    n = 3
    m = n + 2
    ys, xs = np.mgrid[0:H, 0:W]
    ellipse = lambda f: ((xs - 0.45 * W - 3 * f) / (0.22 * W)) ** 2 + ((ys - 0.5 * H) / (0.3 * H)) ** 2 <= 1
    mask = np.where(ellipse(0), 0, 255).astype(np.uint8)
    covers = [None] + [np.where(ellipse(f), 255, 0).astype(np.uint8) for f in range(1, m)]
    flow = np.stack([3.0 + 0.01 * (ys - H / 2), -1.0 + 0.01 * (xs - W / 2)], -1).astype(np.float32)
    flows = [np.where(ellipse(f)[..., None], flow, np.float32(0)) for f in range(m - 1)]
    rgbs = [rng.integers(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(m)]
    occs = [np.where(rng.integers(0, 2, (H, W)) != 0, 255, 0).astype(np.uint8) for _ in range(m - 1)]
    bg = rng.integers(0, 256, (BH, BW, 3)).astype(np.uint8)
    maps = np.asarray([similarity(t) for t in (0.0, 4 / 19.0, 9 / 19.0, 14 / 19.0, 1.0)], np.float32)
    st = opt.State()
    up = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_bg, d_mask = up(bg), up(mask)
    d_cov, d_rgb, d_flow, d_occ = [[up(x) for x in v] for v in (covers, rgbs, flows, occs)]
    d_own = [d_mask] + [up(np.where(c != 0, 0, 255).astype(np.uint8)) for c in covers[1:-1]]     # the yardstick's own masks
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device="cuda")
    o_rgb = [new((H, W, 3), torch.uint8) for _ in range(m)]
    o_flow = [new((H, W, 2), torch.float32) for _ in range(m - 1)]
    o_occ = [new((H, W), torch.uint8) for _ in range(m - 1)]
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    arr = lambda ts: (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])
    mp = maps.ctypes.data_as(C.POINTER(C.c_float))
    m6 = lambda f: (C.c_float * 6)(*maps[f].tolist())

    def seq(out_rgb):
        rc = st.lib.ArapFlow_BackgroundSeq(st.handle, W, H, p(d_bg), BW, BH, m, mp, p(d_mask), arr(d_cov), arr(d_rgb), arr(d_flow),
                                           arr(d_occ), arr(out_rgb), arr(o_flow), arr(o_occ))
        assert rc == 0, rc

    def pairs():
        for f in range(m - 1):
            rc = st.lib.ArapFlow_Background(st.handle, W, H, p(d_bg), BW, BH, m6(f), m6(f + 1), p(d_rgb[f]), p(d_own[f]), None,
                                            p(d_cov[f + 1]), p(d_flow[f]), p(d_occ[f]), None, None, p(o_rgb[f]), None,
                                            p(o_flow[f]), p(o_occ[f]), None, None)
            assert rc == 0, rc

    def timed(fn):
        torch.cuda.synchronize()
        for _ in range(WARM):
            fn()
        torch.cuda.synchronize()
        st.timer_begin()
        for _ in range(ITER):
            fn()
        return 1e3 * st.timer_end() / ITER

    pairs()
    torch.cuda.synchronize()
    ref = [t.clone() for t in o_rgb[:-1] + o_flow + o_occ]
    for t in o_rgb + o_flow + o_occ:
        t.zero_()
    seq(o_rgb)
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(ref, o_rgb[:-1] + o_flow + o_occ)), \
        "the sequence pass and the pair passes differ"
    N = W * H
    print(json.dumps(dict(what="ArapFlow_BackgroundSeq, n = 3", W=W, H=H, bg=[BW, BH], frames=m, calls=ITER,
                          us_seq_every_output=timed(lambda: seq(o_rgb)),
                          us_seq_without_last_rgb=timed(lambda: seq(o_rgb[:-1] + [None])),
                          us_pair_passes=timed(pairs), pair_passes_per_round=m - 1,
                          streamed_bytes_seq=N * ((m - 1) * (3 + 1 + 8 + 1 + 3 + 8 + 1) + (3 + 1 + 3)))))
    st.close()


if __name__ == "__main__":
    main_seq() if "--seq" in sys.argv[1:] else main()
