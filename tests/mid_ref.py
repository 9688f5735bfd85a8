"""float32 numpy restatement of `step` (DESIGN.md "In-between frames"): the flow from the warp of a deformation state a
to a second state b, in the domain of the warped frame.  On top of tests/occ_ref.py (its triangles, cell ranges and
`_bary`); the ramp of the frame solver composed from the oracle's pieces (`ramp_states`) lives here too.

`step_ref` is vectorised; `step_brute` is a plain sequential Python statement of the definition, for tiny grids only.
Both evaluate every float expression in the kernel's order, one IEEE float32 operation at a time.
"""
import numpy as np

import occ_ref

F = np.float32


def grid_field(W, H):
    ys, xs = np.mgrid[0:H, 0:W]
    return np.stack([xs, ys], -1).astype(F)


def winners(mask, field):
    """T(q) per pixel (the largest index of a triangle drawn there, -1 if none) and the triangle table of occ_ref"""
    H, W = mask.shape
    field = np.ascontiguousarray(field, F)
    t, corners, (pa, pb, pc) = occ_ref._triangles(field, mask)
    xa, ya, nx, ny = occ_ref._cell_ranges(W, H, pa, pb, pc)
    k, x, y = occ_ref._pairs(xa, ya, nx, ny)
    ok = occ_ref._bary(pa[k, 0], pa[k, 1], pb[k, 0], pb[k, 1], pc[k, 0], pc[k, 1], x.astype(F), y.astype(F))[0]
    win = np.full(W * H, -1, np.int64)
    np.maximum.at(win, (x + W * y)[ok], t[k[ok]])
    return win, t, corners, (pa, pb, pc)


def step_ref(mask, field_a, field_b):
    """step f32[H,W,2]: per pixel q with winner T(q) under field a, corners c0 c1 c2 and barycentrics (b0, b1, b2) of
    a(c0), a(c1), a(c2) at q:  (b(c0) * b0 + b(c1) * b1) + b(c2) * b2 - q;  (0, 0) where nothing is drawn"""
    H, W = mask.shape
    win, t, (ax, ay, bx, by, cx, cy), (pa, pb, pc) = winners(mask, field_a)
    Pb = np.ascontiguousarray(field_b, F).reshape(-1, 2)
    q = np.flatnonzero(win >= 0)
    r = np.searchsorted(t, win[q])
    qx, qy = (q % W).astype(F), (q // W).astype(F)
    ok, b0, b1, b2 = occ_ref._bary(pa[r, 0], pa[r, 1], pb[r, 0], pb[r, 1], pc[r, 0], pc[r, 1], qx, qy)
    assert ok.all()
    d0, d1, d2 = Pb[ax[r] + W * ay[r]], Pb[bx[r] + W * by[r]], Pb[cx[r] + W * cy[r]]
    out = np.zeros((W * H, 2), F)
    for c, s in ((0, qx), (1, qy)):
        out[q, c] = ((d0[:, c] * b0 + d1[:, c] * b1) + d2[:, c] * b2) - s
    return out.reshape(H, W, 2)


def step_brute(mask, field_a, field_b):
    """the definition, sequentially: the quad loop with later triangles winning, then every pixel on its own"""
    H, W = mask.shape
    A, B = np.ascontiguousarray(field_a, F), np.ascontiguousarray(field_b, F)
    one = F(1.0)

    def bary(p0, p1, p2, sx, sy):
        with np.errstate(all="ignore"):
            X0, X1, X2 = p0[0] - sx * one, p1[0] - sx * one, p2[0] - sx * one
            Y0, Y1, Y2 = p0[1] - sy * one, p1[1] - sy * one, p2[1] - sy * one
            d01, d12, d20 = X0 * Y1 - Y0 * X1, X1 * Y2 - Y1 * X2, X2 * Y0 - Y2 * X0
            if d01 < 0 and d12 < 0 and d20 < 0:
                return None
            ood = one / ((d01 + d12) + d20)
            d01, d12, d20 = d01 * ood, d12 * ood, d20 * ood
        if not (d01 >= 0 and d12 >= 0 and d20 >= 0):
            return None
        return d12, d20, d01

    def visits(p, x, y):
        xs, ys = [c[0] for c in p], [c[1] for c in p]
        if any(np.isnan(v) for v in xs + ys):
            return False
        mnx, mny = np.floor(min(xs)), np.floor(min(ys))      # clamped as floats first: +-Inf has no int
        xa = 0 if mnx < 0 else W if mnx > W else int(mnx)
        ya = 0 if mny < 0 else H if mny > H else int(mny)
        return xa <= x < W and x <= np.ceil(max(xs)) and ya <= y < H and y <= np.ceil(max(ys))

    out = np.zeros((H, W, 2), F)
    win = {}
    for uy in range(H - 1):
        for ux in range(W - 1):
            if not all(mask[y, x] == 0 for x, y in ((ux, uy), (ux + 1, uy), (ux, uy + 1), (ux + 1, uy + 1))):
                continue
            for cs in ([(ux, uy), (ux + 1, uy), (ux, uy + 1)], [(ux, uy + 1), (ux + 1, uy), (ux + 1, uy + 1)]):
                p = [A[gy, gx] for gx, gy in cs]
                for y in range(H):
                    for x in range(W):
                        if visits(p, x, y) and bary(*p, F(x), F(y)) is not None:
                            win[(x, y)] = cs                 # later triangles overwrite
    for (x, y), cs in win.items():
        b = bary(*[A[gy, gx] for gx, gy in cs], F(x), F(y))
        d = [B[gy, gx] for gx, gy in cs]
        for c in range(2):
            out[y, x, c] = ((d[0][c] * b[0] + d[1][c] * b[1]) + d[2][c] * b[2]) - F((x, y)[c])
    return out


def smooth_flow(W, H, seed, amp):
    """a smooth random flow: a coarse normal lattice, bilinearly enlarged"""
    rng = np.random.default_rng(seed)
    gh, gw = H // 8 + 2, W // 8 + 2
    c = rng.normal(size=(gh, gw, 2)) * amp
    ys, xs = np.mgrid[0:H, 0:W]
    fy, fx = ys / 8.0, xs / 8.0
    y0, x0 = fy.astype(int), fx.astype(int)
    ty, tx = (fy - y0)[..., None], (fx - x0)[..., None]
    f = (c[y0, x0] * (1 - ty) * (1 - tx) + c[y0, x0 + 1] * (1 - ty) * tx + c[y0 + 1, x0] * ty * (1 - tx) +
         c[y0 + 1, x0 + 1] * ty * tx)
    return f.astype(F)


def holes_mask(W, H, seed, frac=0.15):
    """object everywhere but random single-pixel and block holes"""
    rng = np.random.default_rng(seed + 1000)
    m = np.where(rng.random((H, W)) < frac * 0.3, 255, 0).astype(np.uint8)
    for _ in range(3):
        y, x = rng.integers(0, H - 3), rng.integers(0, W - 3)
        m[y:y + rng.integers(2, 6), x:x + rng.integers(2, 6)] = 255
    return m


def two_state_case(W, H, seed, kind):
    """(rgb, mask, flow_a, flow_b): two deformations of one frame.  kind "smooth": smooth random fields on a mask with
    holes; "folded": a pair of occ_ref.folded_case flows (triangles overlap and flip)"""
    if kind == "folded":
        rgb, mask, fa = occ_ref.folded_case(W, H, 1.5, seed=seed)
        fb = occ_ref.folded_case(W, H, 2.5, seed=seed + 77)[2]
        fb[mask != 0] = 0
        return rgb, mask, fa, fb
    rgb = np.random.default_rng(seed).integers(0, 256, (H, W, 3)).astype(np.uint8)
    mask = holes_mask(W, H, seed)
    fa, fb = smooth_flow(W, H, seed, 2.0), smooth_flow(W, H, seed + 1, 3.0)
    fa[mask != 0] = 0
    fb[mask != 0] = 0
    return rgb, mask, fa, fb


def ramp_states(oracle, mask_red, cons, num_iter, n_iter, l_iter):
    """the frame solver's ramp composed from the oracle's pieces: reset, then per ramp step i the constraint image at
    alpha_i = (float)i / (float)num_iter and one solve warm-started from the previous step.  Returns the lists
    [Offset_1 .. Offset_numIter], [Angle_1 ..]: the states S_i."""
    mask_red = np.ascontiguousarray(mask_red, np.uint8)
    H, W = mask_red.shape
    allc = np.concatenate([np.asarray(cons, np.int32).reshape(-1, 4), oracle.border_pins(W, H)])
    U = grid_field(W, H)
    O, A = U.copy(), np.zeros((H, W), F)
    M = mask_red.astype(F)
    wf, wr = np.sqrt(F(100.0)), np.sqrt(F(0.01))
    Os, As = [], []
    for i in range(1, num_iter + 1):
        alpha = F(i) / F(num_iter)
        Cn = oracle.constraint_image(mask_red, allc, alpha)
        O, A, _ = oracle.solve(O, A, U, Cn, M, wf, wr, n_iter, l_iter, dtype=np.float32, mode=1, trig=1)
        Os.append(O)
        As.append(A)
    return Os, As


def exact_flow(state):
    """where flow = state - grid loses no bit of the state: (state - grid) + grid == state, per value"""
    H, W = state.shape[:2]
    grid = grid_field(W, H)
    return ((state - grid) + grid) == state


SOLVER_CASE = dict(W=96, H=72, schedule=(4, 2, 40), snapshots=(1, 3, 4))
_solver_case = {}


def solver_case(oracle):
    """the frame-solver case of the in-between tests, computed once: three synthetic frames with uneven masks and, per
    frame, the states S_1 .. S_numIter of the composed oracle loop"""
    if not _solver_case:
        from arap_flow_amd import synth
        W, H = SOLVER_CASE["W"], SOLVER_CASE["H"]
        frames = []
        for seed, K, area in ((31, 1, 0.12), (32, 2, 0.25), (33, 1, 0.4)):
            labels = synth.make_labels(W, H, K, seed, area_frac=area)
            f = dict(rgb=synth.make_rgb(W, H, seed), mask_red=np.where(labels != 0, 0, 255).astype(np.uint8),
                     constraints=synth.make_constraints(labels, seed, fd=3))
            f["states"] = ramp_states(oracle, f["mask_red"], f["constraints"], *SOLVER_CASE["schedule"])[0]
            frames.append(f)
        _solver_case["frames"] = frames
    return _solver_case["frames"]
