"""numpy twin of DESIGN.md "Motion blur" (arap_flow_amd/csrc/arap_blur.h), built on occ_layers_ref and bg_ref.

`blur_ref` is vectorised: the schedule in Python double rounded to float32, per sample occ_layers_ref.layers_ref on the
positions of the flow u*a + t*b (float32, one operation per operator), bg_ref's bilinear sample behind the samples that
leave a pixel uncovered, integer sums and the two rounding formulas.  `blur_brute` is a plain sequential Python statement
of the same definitions for tiny grids, built on occ_layers_ref.layers_brute.
"""
import numpy as np

import bg_ref
import occ_layers_ref
from occ_ref import F

MAX_SAMPLES = 32


def times(centre, shutter, samples):
    """t_k = c + e ((k + 0.5) / S - 0.5): double arithmetic on the float32 values of c and e, rounded once to float32"""
    c, e = float(F(centre)), float(F(shutter))
    return np.array([F(c + e * ((k + 0.5) / samples - 0.5)) for k in range(samples)], F)


def maps(ts, Ma, Mb):
    """the sampling map of every sample: u Ma + t Mb per coefficient in float32; Ma itself when Ma and Mb are bit-equal"""
    Ma, Mb = np.asarray(Ma, F), np.asarray(Mb, F)
    if Ma.tobytes() == Mb.tobytes():
        return np.stack([Ma] * len(ts))
    return np.stack([(F(1.0) - t) * Ma + t * Mb for t in np.asarray(ts, F)]).astype(F)


def mix(flows_a, flows_b, t):
    """the flow of the sample at time t: u a + t b, u = 1 - t, float32; flows_a None: zeros"""
    flows_b = np.asarray(flows_b, F)
    a = np.zeros_like(flows_b) if flows_a is None else np.asarray(flows_a, F)
    t = F(t)
    with np.errstate(all="ignore"):
        return ((F(1.0) - t) * a + t * flows_b).astype(F)


def mean_rgb(total, S):
    """round half up of total / S, in integers"""
    return ((2 * np.asarray(total, np.int64) + S) // (2 * S)).astype(np.uint8)


def mean_alpha(cnt, S):
    return ((2 * 255 * np.asarray(cnt, np.int64) + S) // (2 * S)).astype(np.uint8)


def _blur(render, rgb, masks, flows_b, centre, shutter, samples, flows_a, bg, Ma, Mb, sample_bg, cache=None):
    masks = np.asarray(masks)
    n, H, W = masks.shape
    ts = times(centre, shutter, samples)
    Ms = maps(ts, Ma, Mb) if bg is not None else None
    total, cnt = np.zeros((H, W, 3), np.int64), np.zeros((H, W), np.int64)
    for k, t in enumerate(ts):
        r = None if cache is None else cache.get(t.tobytes())
        if r is None:
            r = render(rgb, masks, occ_layers_ref.fields_from_flows(mix(flows_a, flows_b, t)))
            r = dict(warped_mask=r["warped_mask"], warped_rgb=r["warped_rgb"])
            if cache is not None:
                cache[t.tobytes()] = r
        cov = r["warped_mask"] != 0
        colour = np.where(cov[..., None], r["warped_rgb"], 0).astype(np.int64)
        if bg is not None:
            colour = np.where(cov[..., None], colour, sample_bg(bg, Ms[k], W, H))
        total += colour
        cnt += cov
    return mean_rgb(total, samples), mean_alpha(cnt, samples)


def blur_ref(rgb, masks, flows_b, centre, shutter, samples, flows_a=None, bg=None, Ma=bg_ref.IDENTITY, Mb=bg_ref.IDENTITY,
             cache=None):
    """-> (out_rgb u8[H,W,3], out_alpha u8[H,W]).  `cache`: a dict the caller keeps for ONE (rgb, masks, flows_a, flows_b):
    the render of a sample time is computed once and shared between calls (with and without bg, other sample counts)"""
    return _blur(occ_layers_ref.layers_ref, rgb, masks, flows_b, centre, shutter, samples, flows_a, bg, Ma, Mb,
                 lambda bg, M, W, H: bg_ref.sample(bg, *bg_ref.apply_map(M, W, H)).astype(np.int64), cache)


def _sample_bg_seq(bg, M, W, H):
    """bg_ref.sample pixel by pixel, each pixel on its own"""
    out = np.zeros((H, W, 3), np.int64)
    M = np.asarray(M, F)
    for y in range(H):
        for x in range(W):
            bx = bg_ref.fma(M[0], F(x), bg_ref.fma(M[1], F(y), M[2]))
            by = bg_ref.fma(M[3], F(x), bg_ref.fma(M[4], F(y), M[5]))
            out[y, x] = bg_ref.sample(bg, bx, by)
    return out


def blur_brute(rgb, masks, flows_b, centre, shutter, samples, flows_a=None, bg=None, Ma=bg_ref.IDENTITY, Mb=bg_ref.IDENTITY):
    """the sequential statement: layers_brute per sample, the picture sampled pixel by pixel; tiny grids only"""
    return _blur(occ_layers_ref.layers_brute, rgb, masks, flows_b, centre, shutter, samples, flows_a, bg, Ma, Mb,
                 _sample_bg_seq)
