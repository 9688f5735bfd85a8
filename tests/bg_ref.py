"""Vectorised float32 numpy twin of DESIGN.md "Moving background" (arap_flow_amd/csrc/arap_bg.h): the same float32
operations in the same order.  An fmaf is a float64 product and sum rounded once to float32: the product of two float32
is exact in float64, and so is the sum wherever it matters here (coordinates are integers below 2^24, colours integers
below 2^8, coefficients float32) -- tests/test_bg_host.py checks the twin against an exactly rounded per-pixel statement.
The point maps G / Ginv are an input: the tests take them from ArapFlow_BackgroundMaps (or maps_f64 below, its float64
statement, on the CPU), so the inversion is stated once."""
import numpy as np

F = np.float32
OUTPUTS = ("out_rgb1", "out_rgb2", "flow_full", "occ_full", "bwd_full", "occ_bwd_full")
IDENTITY = np.array([1, 0, 0, 0, 1, 0], F)


def fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def apply_map(m, W, H):
    """(px, py) float32 [H, W] of the six-float map m at every pixel"""
    m = np.asarray(m, F)
    ys, xs = np.mgrid[0:H, 0:W]
    xs, ys = xs.astype(F), ys.astype(F)
    return fma(m[0], xs, fma(m[1], ys, m[2])), fma(m[3], xs, fma(m[4], ys, m[5]))


def sample(bg, bx, by):
    """S(bg, b): bilinear, clamp to edge, round half up -> u8 [..., 3]"""
    bh, bw = bg.shape[:2]
    bx = np.minimum(np.maximum(bx, F(0)), F(bw - 1))
    by = np.minimum(np.maximum(by, F(0)), F(bh - 1))
    x0, y0 = np.floor(bx).astype(np.int64), np.floor(by).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, bw - 1), np.minimum(y0 + 1, bh - 1)
    fx, fy = (bx - x0.astype(F))[..., None], (by - y0.astype(F))[..., None]
    c = bg.astype(F)
    c00, c01, c10, c11 = c[y0, x0], c[y0, x1], c[y1, x0], c[y1, x1]
    top, bot = fma(fx, c01 - c00, c00), fma(fx, c11 - c10, c10)
    v = fma(fy, bot - top, top)
    return (v + F(0.5)).astype(np.uint8)


def hidden(px, py, hides, W, H):
    """background occlusion: the target leaves the frame (NaN counts as outside) or `hides` is set at its nearest pixel"""
    inside = (px >= 0) & (px <= F(W - 1)) & (py >= 0) & (py <= F(H - 1))
    nx = np.where(inside, np.floor(px + F(0.5)), 0).astype(np.int64)
    ny = np.where(inside, np.floor(py + F(0.5)), 0).astype(np.int64)
    return ~inside | hides[ny, nx]


def background(bg, M1, M2, G, Ginv, rgb1, mask_red, rgb2, cover2, flow=None, occ=None, bwd=None, occ_bwd=None):
    """every output of ArapFlow_Background whose input is given, {name: array}"""
    H, W = mask_red.shape
    obj1, obj2 = mask_red == 0, cover2 != 0
    ys, xs = np.mgrid[0:H, 0:W]
    grid = np.stack([xs, ys], -1).astype(F)
    out = {}
    if rgb1 is not None:
        out["out_rgb1"] = np.where(obj1[..., None], rgb1, sample(bg, *apply_map(M1, W, H)))
    if rgb2 is not None:
        out["out_rgb2"] = np.where(obj2[..., None], rgb2, sample(bg, *apply_map(M2, W, H)))
    px, py = apply_map(G, W, H)
    if flow is not None:
        out["flow_full"] = np.where(obj1[..., None], flow, np.stack([px, py], -1) - grid).astype(F)
    if occ is not None:
        out["occ_full"] = np.where(obj1, occ, np.where(hidden(px, py, obj2, W, H), 255, 0)).astype(np.uint8)
    qx, qy = apply_map(Ginv, W, H)
    if bwd is not None:
        out["bwd_full"] = np.where(obj2[..., None], bwd, np.stack([qx, qy], -1) - grid).astype(F)
    if occ_bwd is not None:
        out["occ_bwd_full"] = np.where(obj2, occ_bwd, np.where(hidden(qx, qy, obj1, W, H), 255, 0)).astype(np.uint8)
    return out


def affine3(m):
    m = np.asarray(m, np.float64)
    return np.array([[m[0], m[1], m[2]], [m[3], m[4], m[5]], [0, 0, 1]])


def maps_f64(M1, M2):
    """float64 numpy statement of G = M2^-1 o M1 and Ginv = M1^-1 o M2 (six numbers each, not rounded to float32)"""
    A, B = affine3(np.asarray(M1, F)), affine3(np.asarray(M2, F))
    return (np.linalg.inv(B) @ A)[:2].ravel(), (np.linalg.inv(A) @ B)[:2].ravel()


def similarity(deg, scale, shift, centre):
    """the six float32 of the similarity about `centre`: rotate by deg, scale, then shift"""
    t = np.deg2rad(deg)
    a, b = scale * np.cos(t), scale * np.sin(t)
    cx, cy = centre
    return np.array([a, -b, cx - a * cx + b * cy + shift[0], b, a, cy - b * cx - a * cy + shift[1]], F)


def compose(A, B):
    """A o B (first B, then A), float64 arithmetic, rounded once to float32"""
    return (affine3(A) @ affine3(B))[:2].ravel().astype(F)


def ellipse_case(W, H, bw, bh, seed=0):
    """a frame pair for the tests: random rgb1 and bg, an elliptic object, a small synthetic flow that is 0 off the object"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    inside = ((xs - 0.45 * W) / (0.22 * W)) ** 2 + ((ys - 0.5 * H) / (0.3 * H)) ** 2 <= 1
    mask_red = np.where(inside, 0, 255).astype(np.uint8)
    flow = np.stack([2.25 + 0.02 * (ys - H / 2), -0.75 + 0.03 * (xs - W / 2)], -1).astype(F)
    flow[~inside] = 0
    return dict(rgb1=rng.integers(0, 256, (H, W, 3)).astype(np.uint8), bg=rng.integers(0, 256, (bh, bw, 3)).astype(np.uint8),
                mask_red=mask_red, flow=flow)
