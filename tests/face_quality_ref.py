"""numpy restatement of face quality records and quality-gated face batches ("Face quality"): a helper, not a test.

The crop is align_ref's, untouched.  Every image statistic is an integer sum over its luma (Python / int64 integers, so the order
does not matter); every landmark number is IEEE double with + - * / only in the order written below (numpy never contracts into
FMA).  The kernels (retinaface_amd/csrc/kernels.hip: face_quality_kernel, face_gate_scan_kernel), rf_face_pose and
rf_face_gate_eval are checked byte for byte against this file.
"""
import numpy as np

import align_ref
import face_batch_ref

DTYPE = np.dtype([("flags", "<i4"), ("covered", "<i4"), ("sum_luma", "<i8"), ("sum_lap", "<i8"), ("sum_lap2", "<i8"),
                  ("sharpness", "<f8"), ("iod2", "<f8"), ("yaw", "<f8"), ("sin2_roll", "<f8")])
INVALID, SHARPNESS, IOD, YAW, ROLL, COVERED, DARK, BRIGHT = 1, 2, 4, 8, 16, 32, 64, 128
GATE_FIELDS = ("min_sharpness", "min_iod", "max_abs_yaw", "max_sin2_roll", "min_covered", "min_luma", "max_luma")


def luma(crop):
    """(S, S, 3) u8 BGR -> (S, S) int64"""
    c = np.asarray(crop).astype(np.int64)
    return (29 * c[..., 0] + 150 * c[..., 1] + 77 * c[..., 2] + 128) >> 8


def pose(face, cs=1.0, size=112):
    """(valid, iod2, yaw, sin2_roll) as float64; zeros for an invalid face"""
    f = np.asarray(face, np.float32)
    ok, fwd, _ = align_ref.estimate(f, cs, size)
    zero = np.float64(0.0)
    if not ok:
        return False, zero, zero, zero
    c = np.float64(np.float32(cs))
    two = np.float64(2.0)
    with np.errstate(all="ignore"):
        p0x, p0y = np.float64(f[5]) * c, np.float64(f[10]) * c
        p1x, p1y = np.float64(f[6]) * c, np.float64(f[11]) * c
        p2x, p2y = np.float64(f[7]) * c, np.float64(f[12]) * c
        ex = p1x - p0x
        ey = p1y - p0y
        iod2 = ex * ex + ey * ey
        mx = (p0x + p1x) / two
        my = (p0y + p1y) / two
        yaw = ((p2x - mx) * ex + (p2y - my) * ey) / iod2
        s2 = fwd[3] * fwd[3] / (fwd[0] * fwd[0] + fwd[3] * fwd[3])
    return True, iod2, yaw, s2


def covered(frame, face, cs=1.0, size=112):
    """crop pixels whose in-range test holds and whose rounded top-left tap (x0, y0) is a pixel of the frame"""
    S = int(size)
    ok, _, inv = align_ref.estimate(face, cs, S)
    if not ok:
        return 0
    ia, ib, mpx, mpy, mqx, mqy = inv
    rows, cols = frame.shape[:2]
    with np.errstate(all="ignore"):
        du = np.arange(S, dtype=np.float64)[None, :] - mqx
        dv = np.arange(S, dtype=np.float64)[:, None] - mqy
        x = (ia * du - ib * dv) + mpx
        y = (ib * du + ia * dv) + mpy
        inside = (x > -2) & (x < np.float64(cols + 1)) & (y > -2) & (y < np.float64(rows + 1))
        X = np.floor(np.where(inside, x, 0.0) * 1024.0 + 0.5).astype(np.int64)
        Y = np.floor(np.where(inside, y, 0.0) * 1024.0 + 0.5).astype(np.int64)
    x0, y0 = X >> 10, Y >> 10
    return int((inside & (x0 >= 0) & (x0 < cols) & (y0 >= 0) & (y0 < rows)).sum())


def sums(crop):
    """(sum_luma, sum_lap, sum_lap2) of an (S, S, 3) u8 crop, Python integers"""
    y = luma(crop)
    lap = 4 * y[1:-1, 1:-1] - y[1:-1, :-2] - y[1:-1, 2:] - y[:-2, 1:-1] - y[2:, 1:-1]
    return int(y.sum()), int(lap.sum()), int((lap * lap).sum())


def sharpness(sum_lap, sum_lap2, size):
    n = (int(size) - 2) ** 2
    num = n * int(sum_lap2) - int(sum_lap) * int(sum_lap)
    assert -2 ** 63 <= num < 2 ** 63
    return np.float64(num) / (np.float64(n) * np.float64(n))          # int -> float64 rounds to nearest even, as the conversion does


def quality(frame, face, cs=1.0, size=112):
    """the record of one face, flags = INVALID or 0 (no gate applied), as a DTYPE scalar"""
    q = np.zeros((), DTYPE)
    ok, iod2, yaw, s2 = pose(face, cs, size)
    if not ok:
        q["flags"] = INVALID
        return q
    crop, _ = align_ref.crop(frame, face, cs, size)
    sl, sa, sb = sums(crop)
    q["covered"] = covered(frame, face, cs, size)
    q["sum_luma"], q["sum_lap"], q["sum_lap2"] = sl, sa, sb
    q["sharpness"] = sharpness(sa, sb, size)
    q["iod2"], q["yaw"], q["sin2_roll"] = iod2, yaw, s2
    return q


def gate_flags(q, gate, size=112):
    """flags of record q (its INVALID bit marks an invalid face) under `gate`: None, or a dict of GATE_FIELDS (absent / 0 = off)"""
    if gate is None:
        return 0
    g = {k: np.float64(np.float32(gate.get(k, 0.0))) for k in GATE_FIELDS}
    area = np.float64(int(size) * int(size))
    f = INVALID if int(q["flags"]) & INVALID else 0
    sh, iod2, yaw, s2 = (np.float64(q[k]) for k in ("sharpness", "iod2", "yaw", "sin2_roll"))
    cov, sl = np.float64(int(q["covered"])), np.float64(int(q["sum_luma"]))
    with np.errstate(all="ignore"):
        if g["min_sharpness"] != 0 and not sh >= g["min_sharpness"]:
            f |= SHARPNESS
        if g["min_iod"] != 0 and not iod2 >= g["min_iod"] * g["min_iod"]:
            f |= IOD
        if g["max_abs_yaw"] != 0 and not (yaw >= -g["max_abs_yaw"] and yaw <= g["max_abs_yaw"]):
            f |= YAW
        if g["max_sin2_roll"] != 0 and not s2 <= g["max_sin2_roll"]:
            f |= ROLL
        if g["min_covered"] != 0 and not cov >= g["min_covered"] * area:
            f |= COVERED
        if g["min_luma"] != 0 and not sl >= g["min_luma"] * area:
            f |= DARK
        if g["max_luma"] != 0 and not sl <= g["max_luma"] * area:
            f |= BRIGHT
    return f


def records(frames, faces, gate=None, *, size=112, max_faces=4096, scales=None):
    """per image the DTYPE array of its considered faces (k < min(len, max_faces); none for an empty frame), flags from `gate`"""
    out = []
    for i, fr in enumerate(frames):
        rows = np.asarray(faces[i], np.float32).reshape(-1, 15)[:max_faces]
        if fr is None:
            rows = rows[:0]
        rec = np.zeros(len(rows), DTYPE)
        for k, r in enumerate(rows):
            rec[k] = quality(fr, r, 1.0 if scales is None else scales[i], size)
            rec[k]["flags"] = gate_flags(rec[k], gate, size)
        out.append(rec)
    return out


def gated_batch(frames, faces, fmt, gate, *, size=112, rgb=0, mean=None, scale=None, max_faces=4096, capacity=None, scales=None):
    """face_batch_ref.batch over the faces whose flags are 0.  Returns (tensor, matrices, offsets -- the true numbers --, records)."""
    recs = records(frames, faces, gate, size=size, max_faces=max_faces, scales=scales)
    kept = []
    for i, rec in enumerate(recs):
        rows = np.asarray(faces[i], np.float32).reshape(-1, 15)[:len(rec)]
        kept.append(rows[rec["flags"] == 0])
    t, m, off = face_batch_ref.batch(frames, kept, fmt, size=size, rgb=rgb, mean=mean, scale=scale, max_faces=max_faces, capacity=capacity,
                                     scales=scales)
    return t, m, off, recs
