"""Masks and handles of tests/test_gpu_resident_cells.py (its own copy of the builders: the other resident tests keep
theirs).  A frame is dict(mask_red, constraints): mask_red == 0 marks the active vertices, a constraint row is
(x, y, target x, target y).  Tiles are 32 x 8, in bands of 8 rows that start at the band's first active column."""
import numpy as np

from arap_flow_amd import synth

W, H = 160, 96


def frame_from_labels(labels, seed, extra=()):
    cons = synth.make_constraints(labels, seed)
    if len(extra):
        cons = np.concatenate([cons.reshape(-1, 4), np.asarray(extra, np.int32)]).astype(np.int32)
    return dict(mask_red=np.where(labels != 0, 0, 255).astype(np.uint8), constraints=cons)


def frames_160x96():
    """full (60 tiles on all four image borders, the last column tile of 160 = 5 x 32 exact), rows88 (a band cut at row 87:
    55 tiles, seven to a workgroup when eight share them), thin (a blob with a one-vertex-wide stripe) and holes:
    one-vertex-wide vertical and horizontal stripes, a block with single-vertex holes, isolated vertices -- degrees 0 .. 4,
    excluded neighbours on every side of an active vertex (cells that are never written), bands that start at x = 8, and
    handles on corners and on each border of its tiles next to the lattice ones."""
    ys, xs = np.mgrid[0:H, 0:W]
    thin = (((xs - 50) / 30.0) ** 2 + ((ys - 48) / 25.0) ** 2 <= 1.0).astype(np.int32)
    thin[10:71, 100] = 1
    rows88 = (ys < 88).astype(np.int32)
    holes = np.zeros((H, W), np.int32)
    holes[4:45, 8:72] = (xs[4:45, 8:72] % 2 == 0)                                       # vertical stripes: 2 edges, 1 at the ends
    holes[50:65, 8:72] = (ys[50:65, 8:72] % 2 == 0)                                     # horizontal stripes
    holes[4:61, 72:151] = ~((xs[4:61, 72:151] % 5 == 0) & (ys[4:61, 72:151] % 4 == 0))  # block with holes: 3 and 4 edges
    holes[70:91, 8:150] = (xs[70:91, 8:150] % 3 == 2) & (ys[70:91, 8:150] % 3 == 1)     # isolated vertices: no edge
    # tile corners (8, 8), (40, 8), (103, 15), (104, 16), (135, 23); borders: left (104, 20), bottom (120, 23), top (91, 8),
    # right (103, 19)
    extra = [(x, y, x + 3, y + 2) for x, y in [(8, 8), (40, 8), (103, 15), (104, 16), (135, 23), (104, 20), (120, 23), (91, 8),
                                               (103, 19)]]
    assert all(holes[y, x] for x, y, _, _ in extra)
    deg = sum(np.roll(holes, s, a) for s, a in [(1, 0), (-1, 0), (1, 1), (-1, 1)]) * holes
    assert all(((deg == d) & (holes != 0)).any() for d in range(5))
    for dy, dx in [(0, 1), (0, -1), (1, 0), (-1, 0)]:                                   # an excluded neighbour on every side
        assert ((holes != 0) & (np.roll(holes, (-dy, -dx), (0, 1)) == 0))[1:-1, 1:-1].any()
    return dict(full=frame_from_labels(np.ones((H, W), np.int32), 1), rows88=frame_from_labels(rows88, 5),
                thin=frame_from_labels(thin, 3), holes=frame_from_labels(holes, 4, extra))


def frame_150x90():
    """full 150 x 90: the right tiles are 22 columns wide (150 = 4 x 32 + 22), the last band 2 rows high (90 = 11 x 8 + 2):
    their cells beyond the image must read as zeros.  Handles on the last column and in the last band as well."""
    extra = [(149, 40, 146, 42), (127, 87, 130, 85), (128, 88, 131, 86), (140, 89, 137, 87)]
    return dict(w=150, h=90, frame=frame_from_labels(np.ones((90, 150), np.int32), 6, extra))


def frame_64x64():
    return dict(w=64, h=64, frame=frame_from_labels(np.ones((64, 64), np.int32), 2))


def frame_seven_tiles():
    """64 x 64, a 64 x 24 block and a 32 x 8 one below it: 7 tiles that one workgroup can hold (both neighbours of a shared
    border are then slots of the same workgroup).  Handles inside tiles, on a tile corner (32, 24) and on a left (32, 28),
    top (20, 24), right (31, 36) and bottom (10, 39) border."""
    mask = np.full((64, 64), 255, np.uint8)
    mask[16:40, :] = 0
    mask[40:48, :32] = 0
    cons = np.asarray([(16, 20, 19, 22), (48, 20, 45, 23), (16, 44, 19, 41), (40, 36, 43, 38), (32, 24, 34, 27), (32, 28, 29, 30),
                       (20, 24, 22, 21), (31, 36, 33, 34), (10, 39, 12, 42)], np.int32)
    assert all(mask[y, x] == 0 for x, y, _, _ in cons)
    return dict(w=64, h=64, frame=dict(mask_red=mask, constraints=cons))
