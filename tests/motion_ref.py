"""numpy restatement of motion-predicted face tracks ("Motion-predicted tracks"): a helper, not a test.

A stream with motion keeps one MOTION record per track slot: a velocity of the box centre, smoothed over the matches.  The frame step is
track_ref's with two changes: a face is matched against the track's PREDICTED box, and a matched track updates its velocity before its
`last` face is overwritten.  Redaction coasts at the predicted box.  All arithmetic is float32 with one rounding per operation
(np.float32 scalars never contract).  The kernels (retinaface_amd/csrc/kernels.hip track_motion_kernel and the coasting variant of
redact_regions_kernel), retinaface_amd/csrc/motion.h and the host entry points rf_track_step_motion / rf_track_predict are checked byte
for byte against this file: the records below have the C layout.
"""
import numpy as np

import track_ref as tr
from track_ref import FACE, TAG, TRACK, f32

MOTION = np.dtype([("vx", "<f4"), ("vy", "<f4"), ("samples", "<i4"), ("reserved", "<i4")])
assert MOTION.itemsize == 16
MAX_SAMPLES = 1 << 30
MAX_HORIZON = 65536
XS = (1, 3, 5, 6, 7, 8, 9)            # the x coordinates of a 15-float face row; the other 7 coordinates are y's
YS = (2, 4, 10, 11, 12, 13, 14)


class Spec:
    """rf_motion_spec's defaults: 0 = default; a negative horizon never extrapolates (kept as 0)"""

    def __init__(self, alpha=0.0, horizon=0):
        if not (np.isfinite(alpha) and 0.0 <= alpha <= 1.0):
            raise ValueError("alpha must be finite and in (0, 1]")
        if horizon > MAX_HORIZON:
            raise ValueError("horizon must be in [1, 65536]")
        self.alpha = f32(alpha) if f32(alpha) != 0 else f32(0.5)
        self.horizon = 8 if horizon == 0 else max(horizon, 0)


class Stream(tr.Stream):
    """track_ref.Stream + the motion records and their spec"""

    def __init__(self, spec, mspec=None):
        super().__init__(spec)
        self.mspec = mspec or Spec()
        self.motion = np.zeros(spec.max_tracks, MOTION)


def frames_ahead(missed, ahead, horizon):
    return min(int(missed) + ahead, horizon)


def predict_row(last_row, rec, h):
    """the predicted face (15 float32) of a track whose `last` is last_row, h frames ahead.  samples == 0 or h == 0: the same bytes."""
    out = np.array(last_row, np.float32).copy()
    if rec["samples"] == 0 or h == 0:
        return out
    with np.errstate(all="ignore"):
        dx, dy = f32(rec["vx"]) * f32(h), f32(rec["vy"]) * f32(h)
        for i in XS:
            out[i] = out[i] + dx
        for i in YS:
            out[i] = out[i] + dy
    return out


def predict(track, rec, ahead, mspec):
    """rf_track_predict: the predicted face of a live track for h = min(missed + ahead, horizon)"""
    row = np.frombuffer(np.asarray(track["last"]).tobytes(), np.float32)
    return predict_row(row, rec, frames_ahead(track["missed"], ahead, mspec.horizon))


def predicted_table(stream, ahead=0):
    """a copy of the stream's table whose `last` faces are the predicted ones: what redaction coasts at (ahead 0)"""
    table = stream.table.copy()
    for s in range(len(table)):
        if table[s]["id"] != 0:
            table[s]["last"] = predict(stream.table[s], stream.motion[s], ahead, stream.mspec).view(FACE)[0]
    return table


def _update_velocity(rec, box, last, missed, alpha):
    with np.errstate(all="ignore"):
        dt = f32(int(missed) + 1)
        half = f32(0.5)
        rx = ((box[0] + box[2]) * half - (last[0] + last[2]) * half) / dt
        ry = ((box[1] + box[3]) * half - (last[1] + last[3]) * half) / dt
        if rec["samples"] == 0:
            vx, vy = rx, ry
        else:
            vx = f32(rec["vx"]) + alpha * (rx - f32(rec["vx"]))
            vy = f32(rec["vy"]) + alpha * (ry - f32(rec["vy"]))
    if not (np.isfinite(vx) and np.isfinite(vy)):
        return np.zeros((), MOTION)
    out = np.zeros((), MOTION)
    out["vx"], out["vy"], out["samples"] = vx, vy, min(int(rec["samples"]) + 1, MAX_SAMPLES)
    return out


def step(stream, faces, coord_scale=1.0, quality=None, max_faces=tr.MAX_FACES):
    """one frame step with motion; arguments and results as track_ref.step"""
    sp, ms = stream.spec, stream.mspec
    faces = tr.rows_of(tr.faces_array(faces) if not (isinstance(faces, np.ndarray) and faces.dtype == FACE) else faces)
    count = len(faces)
    m = min(count, max_faces, tr.MAX_FACES)
    tags = np.zeros(count, TAG)
    for k in range(m, count):
        tags[k] = tr._untracked()
    f = stream.frames
    stream.frames = f + 1
    mapped = faces[:m].copy()
    with np.errstate(all="ignore"):
        mapped[:, 1:] = mapped[:, 1:] * f32(coord_scale)
    table, motion = stream.table, stream.motion
    T = sp.max_tracks
    # the predicted boxes, taken once at the start of the step
    pred = np.zeros((T, 4), np.float32)
    for s in range(T):
        if table[s]["id"] != 0:
            pred[s] = predict(table[s], motion[s], 1, ms)[1:5]
    claimed = np.zeros(T, bool)
    slot_of = [-1] * m
    for k in range(m):
        best_iou, best_slot = None, -1
        for s in range(T):
            if table[s]["id"] == 0 or claimed[s]:
                continue
            v = tr.iou(mapped[k, 1:5], pred[s])
            if not v >= sp.min_iou:
                continue
            if best_slot < 0 or v > best_iou:          # strict: ties stay with the lowest slot
                best_iou, best_slot = v, s
        if best_slot < 0:
            continue
        s = best_slot
        claimed[s] = True
        slot_of[k] = s
        t = table[s]
        last = np.array([t["last"]["x1"], t["last"]["y1"], t["last"]["x2"], t["last"]["y2"]], np.float32)
        motion[s] = _update_velocity(motion[s], mapped[k, 1:5], last, t["missed"], ms.alpha)
        t["last"] = mapped[k].view(FACE)[0]
        t["last_frame"] = f
        t["hits"] += 1
        t["missed"] = 0
        if t["hits"] >= sp.min_hits:
            t["flags"] |= tr.CONFIRMED
        b = tr._best(t, mapped[k], f, quality[k] if quality is not None else None)
        tags[k] = tr._tag(t, s, f, sp.min_hits, b)
    ended = []
    for s in range(T):
        if table[s]["id"] == 0 or claimed[s]:
            continue
        table[s]["missed"] += 1
        if table[s]["missed"] > sp.max_missed:
            ended.append(table[s].copy())
            table[s] = np.zeros((), TRACK)
            motion[s] = np.zeros((), MOTION)
    overflow = False
    for k in range(m):
        if slot_of[k] >= 0:
            continue
        if not mapped[k, 0] >= sp.new_score:
            tags[k] = tr._untracked()
            continue
        free = np.nonzero(table["id"] == 0)[0]
        if len(free) == 0:
            tags[k] = tr._untracked(tr.OVERFLOW)
            overflow = True
            continue
        s = int(free[0])
        t = table[s]
        t["id"] = stream.next_id
        stream.next_id += 1
        t["first_frame"] = t["last_frame"] = f
        t["best_frame"] = -1
        t["hits"], t["missed"] = 1, 0
        t["flags"] = tr.CONFIRMED if 1 >= sp.min_hits else 0
        t["last"] = mapped[k].view(FACE)[0]
        motion[s] = np.zeros((), MOTION)
        b = tr._best(t, mapped[k], f, quality[k] if quality is not None else None)
        tags[k] = tr._tag(t, s, f, sp.min_hits, tr.NEW | b)
    return tags, (np.array(ended, TRACK) if ended else np.zeros(0, TRACK)), overflow


def update(streams, stream_of_image, faces, counts, cap_per_image, coord_scale=None, quality=None, max_faces=tr.MAX_FACES, cap_ended=0):
    """rf_track_update_device on a motion tracker: track_ref.update with the step above"""
    n = len(stream_of_image)
    tags = np.zeros((n, cap_per_image), TAG)
    ended = np.zeros((n, max(cap_ended, 0)), TRACK)
    ended_counts = np.zeros(n, np.int32)
    truncated = False
    for i in range(n):
        s = int(stream_of_image[i])
        if s < 0:
            continue
        c = int(counts[i])
        have = min(c, cap_per_image)
        q = quality[i, :min(have, max_faces)] if quality is not None else None
        t, e, over = step(streams[s], faces[i, :have], 1.0 if coord_scale is None else coord_scale[i], q, min(max_faces, cap_per_image))
        tags[i, :have] = t
        ended_counts[i] = len(e)
        ended[i, :min(len(e), cap_ended)] = e[:cap_ended]
        truncated = truncated or over or len(e) > cap_ended
    return tags, ended, ended_counts, truncated


def flush(stream):
    """rf_tracker_flush on a motion tracker: the freed slots' records become zero"""
    out = tr.flush(stream)
    stream.motion[:] = np.zeros((), MOTION)
    return out


# ---- coverage, in pixels.  A box (x1, y1, x2, y2) CONSISTS of the pixels floor(x1) .. floor(x2) by floor(y1) .. floor(y2) inside the
# frame -- the rectangle rf_redact_region gives it with no margin.  It is covered by a list of RECT regions when every one of those
# pixels lies in some region's clipped rectangle [cx0, cx1) x [cy0, cy1).
def box_pixels(box, rows, cols):
    x0, y0 = max(int(np.floor(box[0])), 0), max(int(np.floor(box[1])), 0)
    x1, y1 = min(int(np.floor(box[2])) + 1, cols), min(int(np.floor(box[3])) + 1, rows)
    return x0, y0, x1, y1


def coverage(box, regions, rows, cols):
    """(covered pixels, pixels) of a box under RECT regions given as rows [ux0, uy0, ux1, uy1, cx0, cy0, cx1, cy1, c]"""
    x0, y0, x1, y1 = box_pixels(box, rows, cols)
    hit = np.zeros((max(y1 - y0, 0), max(x1 - x0, 0)), bool)
    for r in regions:
        cx0, cy0, cx1, cy1 = (int(v) for v in r[4:8])
        hit[max(cy0 - y0, 0):max(cy1 - y0, 0), max(cx0 - x0, 0):max(cx1 - x0, 0)] = True
    return int(hit.sum()), hit.size
