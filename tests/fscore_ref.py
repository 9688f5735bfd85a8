"""The numpy twin of ArapFlow_FrameScore (DESIGN.md "Frame scoring"): integer pixel terms, integer window sums by
cumulative sums (and, as a check of those, by a plain loop over a window's 64 pixels), the SSIM quotient float32 operator by
operator, an integer table.  Test helper; no GPU."""
import numpy as np

from arap_flow_amd import pipeline

F = np.float32
ROWS, FIELDS = len(pipeline.FSCORE_ROWS), len(pipeline.FSCORE_FIELDS)
ONE = 1 << 21                       # q of identical windows: s = 1 in units of 2^-20, offset by 1
C1, C2 = 416, 235963


def luma(rgb):
    """Y = (77 R + 150 G + 29 B + 128) >> 8, int64"""
    c = np.asarray(rgb, np.uint8).astype(np.int64)
    return (77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8


def window_sums(a, b):
    """(s1, s2, ss, s12) int64[..., H-7, W-7] of every 8 x 8 window of the lumas a, b [..., H, W], by cumulative sums"""
    def box(v):
        c = np.zeros(v.shape[:-2] + (v.shape[-2] + 1, v.shape[-1] + 1), np.int64)
        c[..., 1:, 1:] = v.cumsum(axis=-2).cumsum(axis=-1)
        return c[..., 8:, 8:] - c[..., :-8, 8:] - c[..., 8:, :-8] + c[..., :-8, :-8]
    return box(a), box(b), box(a * a + b * b), box(a * b)


def window_sums_direct(a, b):
    """the same by a loop over the 64 pixels of a window"""
    H, W = a.shape[-2:]
    out = [np.zeros(a.shape[:-2] + (H - 7, W - 7), np.int64) for _ in range(4)]
    for dy in range(8):
        for dx in range(8):
            pa, pb = a[..., dy:dy + H - 7, dx:dx + W - 7], b[..., dy:dy + H - 7, dx:dx + W - 7]
            for o, v in zip(out, (pa, pb, pa * pa + pb * pb, pa * pb)):
                o += v
    return tuple(out)


def ssim_terms(s1, s2, ss, s12):
    """(s float32, q uint32) of windows from their four sums; asserts that the four integers fit int32"""
    var, covar = 64 * ss - s1 * s1 - s2 * s2, 64 * s12 - s1 * s2
    A, B, C, D = 2 * s1 * s2 + C1, 2 * covar + C2, s1 * s1 + s2 * s2 + C1, var + C2
    for v in (A, B, C, D):
        assert v.size == 0 or (np.abs(v).max() < 1 << 31), "an SSIM integer beyond int32"
    assert A.size == 0 or (A.min() > 0 and C.min() > 0 and D.min() > 0)
    fa, fb, fc, fd = (v.astype(np.int32).astype(F) for v in (A, B, C, D))
    s = (fa * fb) / (fc * fd)
    t = np.maximum(s + F(1), F(0))
    q = (t * F(1048576) + F(0.5)).astype(np.uint32)              # truncation
    assert s.dtype == t.dtype == F and (q.size == 0 or q.max() <= ONE)
    return s, q


def fscore_ref(ref, est, occ=None, dist=None, skip=None, obj=None, sums=window_sums):
    """opt.frame_score's twin: ref, est u8[H,W,3] or [n,H,W,3]; occ u8, dist u16, skip u8, obj u8 of ref's shape without its
    last axis, or None -> dict(table u64[n,9,7], ssim f32[n,H,W], q u32[n,H-7,W-7] or None)"""
    ref, est = np.asarray(ref, np.uint8), np.asarray(est, np.uint8)
    if ref.ndim == 3:
        ref, est = ref[None], est[None]
    n, H, W = shape = ref.shape[:3]
    plane = lambda a, dt: None if a is None else np.asarray(a, dt).reshape(shape).astype(np.int64)
    occ, dist, skip, obj = plane(occ, np.uint8), plane(dist, np.uint16), plane(skip, np.uint8), plane(obj, np.uint8)
    d = np.abs(ref.astype(np.int64) - est.astype(np.int64))
    sse, sad, mx = (d * d).sum(axis=-1), d.sum(axis=-1), d.max(axis=-1)
    skipped = np.zeros(shape, bool) if skip is None else skip != 0
    none = np.zeros(shape, bool)
    on = lambda a, test: none if a is None else ~skipped & test(a)
    cls = [~skipped, on(occ, lambda a: a == 0), on(occ, lambda a: a != 0), on(dist, lambda a: a < 100),
           on(dist, lambda a: (a >= 100) & (a < 3600)), on(dist, lambda a: (a >= 3600) & (a < 19600)),
           on(obj, lambda a: a == 0), on(obj, lambda a: a != 0)]
    table = np.zeros((n, ROWS, FIELDS), np.uint64)
    total = lambda v: v.sum(axis=(1, 2)).astype(np.uint64)
    peak = lambda v: v.max(axis=(1, 2), initial=0).astype(np.uint64)
    ssim = np.full(shape, F(-2), F)
    q = None
    if W >= 8 and H >= 8:
        s, q = ssim_terms(*sums(luma(ref), luma(est)))
        at = lambda v: v[:, 3:H - 4, 3:W - 4]                   # a plane at the anchors of the windows, in the windows' order
        ssim[:, 3:H - 4, 3:W - 4] = np.where(at(skipped), F(-2), s)
    for r, m in enumerate(cls):
        table[:, r, 0], table[:, r, 1], table[:, r, 2] = total(m), total(np.where(m, sse, 0)), total(np.where(m, sad, 0))
        table[:, r, 3] = peak(np.where(m, mx, 0))
        if q is not None:
            w = at(m)
            table[:, r, 4], table[:, r, 5] = total(w), total(np.where(w, q, 0).astype(np.uint64))
            table[:, r, 6] = peak(np.where(w, ONE - q.astype(np.int64), 0))
    table[:, ROWS - 1, 0] = total(skipped)
    if q is not None:
        table[:, ROWS - 1, 1] = total(at(skipped))
    return dict(table=table, ssim=ssim, q=q)
