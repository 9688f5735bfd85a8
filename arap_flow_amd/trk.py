"""Track files (DESIGN.md "Point tracks"): little-endian, the bytes `ATRK`, then int32 version = 1, W, H, F, P, then
float32 pos[F][P][2], then uint8 occ[F][P] (255 = hidden in that frame).  Frame 0 of a written track file holds the
query points themselves; a points file is the same format with F = 1.  host/trk_io.h is the C++ twin."""
import struct

import numpy as np

MAGIC = b"ATRK"
VERSION = 1
_HEAD = struct.Struct("<4s5i")


def in_frame(points, W, H):
    """the kernels' in_frame: NaN counts as outside"""
    p = np.asarray(points, np.float32)
    with np.errstate(invalid="ignore"):
        return (p[..., 0] >= 0) & (p[..., 0] <= np.float32(W - 1)) & (p[..., 1] >= 0) & (p[..., 1] <= np.float32(H - 1))


def write(path, W, H, pos, occ=None):
    """pos f32[F,P,2] (or [P,2]: one frame), occ u8[F,P]; without `occ` it is 0 / 255 by in_frame"""
    pos = np.ascontiguousarray(pos, "<f4")
    if pos.ndim == 2:
        pos = pos[None]
    if pos.ndim != 3 or pos.shape[2] != 2 or pos.shape[0] < 1 or pos.shape[1] < 1:
        raise ValueError("trk.write: pos [F,P,2] expected")
    if occ is None:
        occ = np.where(in_frame(pos, W, H), 0, 255)
    occ = np.ascontiguousarray(occ, np.uint8)
    if occ.shape != pos.shape[:2]:
        raise ValueError("trk.write: occ [F,P] expected")
    with open(path, "wb") as f:
        f.write(_HEAD.pack(MAGIC, VERSION, W, H, pos.shape[0], pos.shape[1]))
        f.write(pos.tobytes())
        f.write(occ.tobytes())


def read(path):
    """-> dict(W, H, pos f32[F,P,2], occ u8[F,P]); a ValueError names what is wrong with the file"""
    with open(path, "rb") as f:
        raw = f.read()
    if len(raw) < _HEAD.size:
        raise ValueError("%s: truncated track file (%d bytes of header)" % (path, len(raw)))
    magic, version, W, H, F, P = _HEAD.unpack_from(raw)
    if magic != MAGIC:
        raise ValueError("%s: not a track file (magic %r)" % (path, magic))
    if version != VERSION:
        raise ValueError("%s: track file version %d, %d expected" % (path, version, VERSION))
    if W < 1 or H < 1 or F < 1 or P < 1:
        raise ValueError("%s: bad track file sizes W=%d H=%d F=%d P=%d" % (path, W, H, F, P))
    want = _HEAD.size + 9 * F * P
    if len(raw) != want:
        raise ValueError("%s: %s track file, %d bytes where %d are expected" %
                         (path, "truncated" if len(raw) < want else "mis-sized", len(raw), want))
    pos = np.frombuffer(raw, "<f4", 2 * F * P, _HEAD.size).reshape(F, P, 2).astype(np.float32)
    occ = np.frombuffer(raw, np.uint8, F * P, _HEAD.size + 8 * F * P).reshape(F, P).copy()
    return dict(W=W, H=H, pos=pos, occ=occ)
