"""numpy restatement of rotation-robust detection ("Rotation-robust detection"): a helper, not a test.

A frame is detected as it is (pass 0) and turned by one, two and three quarter turns counter-clockwise (pass k is np.rot90(F, k)).
Every face is moved into source-frame pixels with one fp32 multiply per coordinate by the frame scale of the PASS's own shape, and one
fp32 subtract where a coordinate flips; the landmarks keep their index.  The faces of all passes are merged by the flip-TTA merge
(tests/tta_ref.py) with g = k * max_det + j, k the rotation.  The kernels (retinaface_amd/csrc/kernels.hip rotate_frames_kernel,
pass_gather_kernel<RotMap>, vote_merge_kernel), retinaface_amd/csrc/rot.h and the host entry points rf_rot_map_face / rf_rot_merge_host /
rf_rotate_host are checked byte for byte against this file.
"""
import numpy as np

import tta_ref
from tile_ref import frame_scale

f32 = np.float32
f64 = np.float64


def rot_list(rots):
    """the rotations a mask runs, ascending; 0 = all four"""
    return [k for k in range(4) if (rots or 15) >> k & 1]


def rotate(frame, k):
    """pass k of a frame"""
    return np.ascontiguousarray(np.rot90(frame, k))


def pass_shape(k, rows, cols):
    return (cols, rows) if k & 1 else (rows, cols)


def map_point(k, rows, cols, x, y):
    """a point (x', y') of pass k (float32, already scaled) in the rows x cols source frame"""
    c, r = f32(cols - 1), f32(rows - 1)
    if k == 0:
        return x, y
    if k == 1:
        return c - y, x
    if k == 2:
        return c - x, r - y
    return y, r - x


def map_face(face, k, rows, cols, net_h, net_w):
    """the mapping of one face (15 float32: score, box, 5 x, 5 y) of pass k"""
    f = np.asarray(face, np.float32).copy()
    f[1:] = f[1:] * frame_scale(*pass_shape(k, rows, cols), net_h, net_w)
    if k == 0:
        return f
    out = f.copy()
    ax, ay = map_point(k, rows, cols, f[1], f[2])
    bx, by = map_point(k, rows, cols, f[3], f[4])
    out[1], out[3] = (ax, bx) if k == 3 else (bx, ax)          # the corner that flipped carries the larger source coordinate
    out[2], out[4] = (ay, by) if k == 1 else (by, ay)
    for i in range(5):
        out[5 + i], out[10 + i] = map_point(k, rows, cols, f[5 + i], f[10 + i])
    return out


def unmap_face(face, k, rows, cols):
    """the face of pass k that maps to `face` at scale 1 (exact on quarter-pixel coordinates): the mapping of pass (4 - k) % 4 of the
    PASS's frame"""
    pr, pc = pass_shape(k, rows, cols)
    return map_face(face, (4 - k) % 4, pr, pc, 1 << 20, 1 << 20)


def candidates(rows, cols, passes, net_h, net_w, max_det, rots=0):
    """the mapped faces of all passes of one frame: (rows (c, 15) float32, g (c,) int64) with g = k * max_det + j"""
    out, gs = [], []
    ks = rot_list(rots)
    assert len(passes) == len(ks)
    for k, faces in zip(ks, passes):
        faces = np.asarray(faces, np.float32).reshape(-1, 15)[:max_det]
        for j, f in enumerate(faces):
            out.append(map_face(f, k, rows, cols, net_h, net_w))
            gs.append(k * max_det + j)
    return (np.stack(out) if out else np.zeros((0, 15), np.float32)), np.array(gs, np.int64)


def orientation(faces, src_rot):
    """(frame_rot, rot_score (4,) float32) of the emitted heads of one frame, in merge order"""
    total = [f64(0)] * 4
    seen = [False] * 4
    for f, k in zip(faces, src_rot):
        total[k] = total[k] + f64(f[0])
        seen[k] = True
    best = -1
    for k in range(4):
        if seen[k] and (best < 0 or total[k] > total[best]):
            best = k
    return best, np.array(total, f64).astype(f32)


def merge(rows, cols, passes, net_h, net_w, nms_threshold, max_det, vote_on=False, max_faces=0, rots=0, cap=None):
    """one frame: (faces (k, 15) float32 in merge order, k = min(count, max_faces); count: the true number of heads; votes (k,) int32;
    src_rot (k,) int32; the number of candidates; frame_rot; rot_score (4,) float32 -- the last two over the first min(k, cap) heads).
    passes[p]: the result of the p-th rotation of `rots`, at most max_det faces in score order."""
    cand, g = candidates(rows, cols, passes, net_h, net_w, max_det, rots)
    faces, count, votes, src = tta_ref.merge_candidates(cand, g, nms_threshold, max_det, vote_on, max_faces)
    lim = len(faces) if cap is None else min(len(faces), cap)
    return (faces, count, votes, src, len(cand)) + orientation(faces[:lim], src[:lim])
