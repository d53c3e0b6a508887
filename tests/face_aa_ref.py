"""numpy restatement of antialiased face crops ("Antialiased face crops"): a helper, not a test.

The transform is align_ref's, untouched.  A face whose source footprint is larger than its crop is supersampled: k x k sub-samples
per crop pixel (k a power of two chosen per face from the inverse similarity), each one sampled exactly as align_ref.crop samples a
pixel centre up to its unshifted integer sum, the sums added and shifted once.  Everything real is IEEE double with + - * / only, in
the order written below; everything after the sample coordinates is integer.  The batch and quality restatements are those of
face_batch_ref / face_quality_ref with this crop in place of align_ref.crop.  The kernels (retinaface_amd/csrc/kernels.hip:
align_sample_aa and the AA instances of face_batch_kernel / face_quality_kernel) and rf_face_aa_factor are checked byte for byte
against this file.
"""
import numpy as np

import align_ref
import face_batch_ref
import face_quality_ref

TEMPLATE_X, TEMPLATE_Y = align_ref.TEMPLATE_X, align_ref.TEMPLATE_Y


def build_face(f, rot=0.0, ox=0.0, oy=0.0, size=112):
    """a face row (15 float32) whose landmarks are the template of crop size `size`, scaled by f, rotated by rot, moved by (ox, oy)"""
    x = np.asarray(TEMPLATE_X, np.float64) * size / 112 * f
    y = np.asarray(TEMPLATE_Y, np.float64) * size / 112 * f
    row = np.zeros(15, np.float32)
    row[0] = 0.9
    row[5:10] = (np.cos(rot) * x - np.sin(rot) * y + ox).astype(np.float32)
    row[10:15] = (np.sin(rot) * x + np.cos(rot) * y + oy).astype(np.float32)
    row[1:5] = (row[5:10].min(), row[10:15].min(), row[5:10].max(), row[10:15].max())
    return row


def _factor(inv, aa_max):
    ia, ib = np.float64(inv[0]), np.float64(inv[1])
    with np.errstate(all="ignore"):
        R = ia * ia + ib * ib
    k = 1
    while k < aa_max and np.float64(k * k) * np.float64(2.0) < R:
        k *= 2
    return k


def aa_factor(face, cs=1.0, size=112, aa_max=4):
    """the supersampling factor per axis of a face: 1, 2, 4 or 8 (<= aa_max); 1 for an invalid face"""
    assert aa_max in (1, 2, 4, 8)
    ok, _, inv = align_ref.estimate(face, cs, size)
    return _factor(inv, aa_max) if ok else 1


def crop_aa(frame, face, cs=1.0, size=112, aa_max=4):
    """frame: H x W x 3 uint8.  Returns (size x size x 3 uint8 antialiased crop, fwd[6] float64)."""
    assert aa_max in (1, 2, 4, 8)
    S = int(size)
    out = np.zeros((S, S, 3), np.uint8)
    ok, fwd, inv = align_ref.estimate(face, cs, S)
    if not ok:
        return out, fwd
    ia, ib, mpx, mpy, mqx, mqy = inv
    k = _factor(inv, aa_max)
    m = k.bit_length() - 1
    rows, cols = frame.shape[:2]
    total = np.zeros((S, S, 3), np.int64)
    for j in range(k):
        for i in range(k):
            ou = np.float64(2 * i + 1 - k) / np.float64(2 * k)
            ov = np.float64(2 * j + 1 - k) / np.float64(2 * k)
            with np.errstate(all="ignore"):
                du = (np.arange(S, dtype=np.float64)[None, :] + ou) - mqx
                dv = (np.arange(S, dtype=np.float64)[:, None] + ov) - mqy
                x = (ia * du - ib * dv) + mpx
                y = (ib * du + ia * dv) + mpy
                inside = (x > -2) & (x < np.float64(cols + 1)) & (y > -2) & (y < np.float64(rows + 1))
                X = np.floor(np.where(inside, x, 0.0) * 1024.0 + 0.5).astype(np.int64)
                Y = np.floor(np.where(inside, y, 0.0) * 1024.0 + 0.5).astype(np.int64)
            x0, fx = X >> 10, X & 1023
            y0, fy = Y >> 10, Y & 1023
            for dy, wy in ((0, 1024 - fy), (1, fy)):
                for dx, wx in ((0, 1024 - fx), (1, fx)):
                    xx, yy = x0 + dx, y0 + dy
                    tap = inside & (xx >= 0) & (xx < cols) & (yy >= 0) & (yy < rows)
                    pix = frame[np.where(tap, yy, 0), np.where(tap, xx, 0)].astype(np.int64)
                    total += np.where(tap, wx * wy, 0)[:, :, None] * pix
    out[:] = ((total + (1 << (19 + 2 * m))) >> (20 + 2 * m)).astype(np.uint8)
    return out, fwd


def crops_aa(frame, faces, cs=1.0, size=112, aa_max=4):
    """(k, size, size, 3) antialiased crops and (k, 6) matrices of the rows of `faces`"""
    faces = np.asarray(faces, np.float32).reshape(-1, 15)
    cr = np.zeros((len(faces), size, size, 3), np.uint8)
    ms = np.zeros((len(faces), 6), np.float64)
    for i, f in enumerate(faces):
        cr[i], ms[i] = crop_aa(frame, f, cs, size, aa_max)
    return cr, ms


def batch(frames, faces, fmt, *, size=112, rgb=0, mean=None, scale=None, max_faces=4096, capacity=None, scales=None, aa_max=4):
    """face_batch_ref.batch with the antialiased crop: (tensor [min(total, capacity), ...], matrices, offsets -- the true numbers)"""
    per_c, per_m, counts = [], [], []
    for i, f in enumerate(frames):
        rows = np.asarray(faces[i], np.float32).reshape(-1, 15)[:max_faces]
        if f is None:
            rows = rows[:0]
        counts.append(len(rows))
        cr, ms = crops_aa(f, rows, 1.0 if scales is None else scales[i], size, aa_max) if len(rows) else (
            np.zeros((0, size, size, 3), np.uint8), np.zeros((0, 6), np.float64))
        per_c.append(cr)
        per_m.append(ms)
    off = face_batch_ref.offsets(counts, max_faces)
    cr = np.concatenate(per_c) if per_c else np.zeros((0, size, size, 3), np.uint8)
    ms = np.concatenate(per_m) if per_m else np.zeros((0, 6), np.float64)
    keep = int(off[-1]) if capacity is None else min(int(off[-1]), int(capacity))
    return face_batch_ref.convert(cr[:keep], fmt, rgb, mean, scale), ms[:keep], off


def quality(frame, face, cs=1.0, size=112, aa_max=4):
    """face_quality_ref.quality with the luma sums of the antialiased crop; covered and the landmark numbers are unchanged"""
    q = np.zeros((), face_quality_ref.DTYPE)
    ok, iod2, yaw, s2 = face_quality_ref.pose(face, cs, size)
    if not ok:
        q["flags"] = face_quality_ref.INVALID
        return q
    crop, _ = crop_aa(frame, face, cs, size, aa_max)
    sl, sa, sb = face_quality_ref.sums(crop)
    q["covered"] = face_quality_ref.covered(frame, face, cs, size)
    q["sum_luma"], q["sum_lap"], q["sum_lap2"] = sl, sa, sb
    q["sharpness"] = face_quality_ref.sharpness(sa, sb, size)
    q["iod2"], q["yaw"], q["sin2_roll"] = iod2, yaw, s2
    return q


def records(frames, faces, gate=None, *, size=112, max_faces=4096, scales=None, aa_max=4):
    """face_quality_ref.records with the antialiased crop"""
    out = []
    for i, fr in enumerate(frames):
        rows = np.asarray(faces[i], np.float32).reshape(-1, 15)[:max_faces]
        if fr is None:
            rows = rows[:0]
        rec = np.zeros(len(rows), face_quality_ref.DTYPE)
        for k, r in enumerate(rows):
            rec[k] = quality(fr, r, 1.0 if scales is None else scales[i], size, aa_max)
            rec[k]["flags"] = face_quality_ref.gate_flags(rec[k], gate, size)
        out.append(rec)
    return out


def gated_batch(frames, faces, fmt, gate, *, size=112, rgb=0, mean=None, scale=None, max_faces=4096, capacity=None, scales=None,
                aa_max=4):
    """batch() over the faces whose flags are 0.  Returns (tensor, matrices, offsets -- the true numbers --, records)."""
    recs = records(frames, faces, gate, size=size, max_faces=max_faces, scales=scales, aa_max=aa_max)
    kept = []
    for i, rec in enumerate(recs):
        rows = np.asarray(faces[i], np.float32).reshape(-1, 15)[:len(rec)]
        kept.append(rows[rec["flags"] == 0])
    t, m, off = batch(frames, kept, fmt, size=size, rgb=rgb, mean=mean, scale=scale, max_faces=max_faces, capacity=capacity,
                      scales=scales, aa_max=aa_max)
    return t, m, off, recs
