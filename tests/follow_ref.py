"""numpy restatement of followed face tracks ("Followed tracks"): a helper, not a test.

A stream with follow keeps, next to its track table (tests/track_ref.py), one 32 x 32 template of luma cell means and one FOLLOW record
per slot.  A key step is the plain frame step plus "retake the template of every face the step tagged"; a follow step searches every
live slot's template in the new frame and moves the track's last box by whole cells.  All arithmetic is integer except the one float32
add per moved coordinate.  retinaface_amd/csrc/follow.h, the three follow kernels and the host entry points are checked byte for byte
against this file, which is written from the definition -- whole cell planes by gather and reshape, candidates as array slices -- and
shares no structure with the C code.
"""
import numpy as np

import track_ref as tr

f32 = np.float32
G = 32
FOLLOW = np.dtype([(k, "<i4") for k in ("valid", "run", "q", "ox", "oy", "sad", "dx", "dy")])
assert FOLLOW.itemsize == 32
FOLLOWED = 32


class FollowSpec:
    """the spec's defaults: 0 = default"""

    def __init__(self, radius=0, max_mad=0, max_run=0):
        if not (0 <= radius <= 16 and 0 <= max_mad <= 255 and 0 <= max_run <= 65536):
            raise ValueError("radius 1..16, max_mad 1..255, max_run 1..65536 (0 = default)")
        self.radius = radius or 8
        self.max_mad = max_mad or 16
        self.max_run = max_run or 8


class Stream(tr.Stream):
    """track_ref's stream plus the follow state"""

    def __init__(self, spec, fspec=None):
        super().__init__(spec)
        self.fspec = fspec or FollowSpec()
        self.records = np.zeros(spec.max_tracks, FOLLOW)
        self.templates = np.zeros((spec.max_tracks, G, G), np.uint8)


def luma(frame):
    """the Y plane (int64) of a (rows, cols, 3) u8 BGR frame"""
    p = frame.astype(np.int64)
    return (29 * p[..., 0] + 150 * p[..., 1] + 77 * p[..., 2] + 128) >> 8


def geometry(box):
    """(q, ox, oy) of a box (x1, y1, x2, y2), or None"""
    b = np.asarray(box, np.float32)
    if not np.all(np.isfinite(b)):
        return None
    ix1, iy1, ix2, iy2 = (int(v) for v in np.floor(np.clip(b.astype(np.float64), -4096.0, 8192.0)))
    W, H = ix2 - ix1 + 1, iy2 - iy1 + 1
    if W < 1 or H < 1:
        return None
    q = max(1, (max(W, H) + G - 1) // G)
    return q, (ix1 + ix2 + 1 - G * q) // 2, (iy1 + iy2 + 1 - G * q) // 2


def cell_plane(Y, cx, cy, q, nx, ny):
    """the (ny, nx) u8 cell values whose first cell has its origin at (cx, cy); the border is replicated"""
    rows, cols = Y.shape
    xs = np.clip(cx + np.arange(nx * q), 0, cols - 1)
    ys = np.clip(cy + np.arange(ny * q), 0, rows - 1)
    sums = Y[np.ix_(ys, xs)].reshape(ny, q, nx, q).sum(axis=(1, 3))
    return ((sums + (q * q) // 2) // (q * q)).astype(np.uint8)


def template(frame, q, ox, oy):
    return cell_plane(luma(frame), ox, oy, q, G, G)


def search(frame, tpl, q, ox, oy, R):
    """(state, sad, du, dv): state 1 = no eligible candidate (sad -1), 2 = the winner"""
    Y = luma(frame)
    rows, cols = Y.shape
    n = G + 2 * R
    win = cell_plane(Y, ox - R * q, oy - R * q, q, n, n).astype(np.int64)
    t = np.asarray(tpl, np.uint8).reshape(G, G).astype(np.int64)
    best = None
    for dv in range(-R, R + 1):
        for du in range(-R, R + 1):
            mx, my = ox + du * q + 16 * q, oy + dv * q + 16 * q
            if not (0 <= mx < cols and 0 <= my < rows):
                continue
            sad = int(np.abs(t - win[dv + R:dv + R + G, du + R:du + R + G]).sum())
            key = (sad << 32) | ((du * du + dv * dv) << 16) | ((dv + R) * (2 * R + 1) + du + R)
            if best is None or key < best[0]:
                best = (key, sad, du, dv)
    return (1, -1, 0, 0) if best is None else (2,) + best[1:]


def empty(frame):
    return frame is None or frame.size == 0


def key_step(stream, frame, faces, coord_scale=1.0, quality=None, max_faces=tr.MAX_FACES):
    """the plain frame step, then the keep rule.  Returns track_ref.step's (tags, ended, overflow); a frame without pixels has no faces."""
    if empty(frame):
        faces = np.zeros((0, 15), np.float32)
    tags, ended, over = tr.step(stream, faces, coord_scale, quality, max_faces)
    stream.records[stream.table["id"] == 0] = np.zeros((), FOLLOW)
    for g in tags:
        s = int(g["slot"])
        if s < 0 or g["flags"] & tr.UNTRACKED:
            continue
        last = stream.table[s]["last"]
        geo = geometry([last["x1"], last["y1"], last["x2"], last["y2"]])
        rec = np.zeros((), FOLLOW)
        if geo is not None:
            rec["valid"], rec["q"], rec["ox"], rec["oy"] = 1, geo[0], geo[1], geo[2]
            stream.templates[s] = template(frame, *geo)
        else:
            stream.templates[s] = 0
        stream.records[s] = rec
    return tags, ended, over


def follow_step(stream, frame):
    """one follow step.  Returns (faces (k,) FACE, tags (k,) TAG -- the accepted slots ascending --, ended (e,) TRACK in slot order)."""
    sp, fs = stream.spec, stream.fspec
    f = stream.frames
    stream.frames = f + 1
    out, tags, ended = [], [], []
    for s in range(sp.max_tracks):
        t, rec = stream.table[s], stream.records[s]
        if t["id"] == 0:
            continue
        res = (0, -1, 0, 0)
        if rec["valid"] and rec["run"] < fs.max_run and not empty(frame):
            res = search(frame, stream.templates[s], int(rec["q"]), int(rec["ox"]), int(rec["oy"]), fs.radius)
        if res[0] == 2 and res[1] <= fs.max_mad * G * G:
            mx, my = res[2] * int(rec["q"]), res[3] * int(rec["q"])
            last = t["last"]
            for name in ("x1", "x2", "px"):
                last[name] = last[name] + f32(mx)
            for name in ("y1", "y2", "py"):
                last[name] = last[name] + f32(my)
            rec["ox"] += mx
            rec["oy"] += my
            rec["run"] += 1
            rec["sad"], rec["dx"], rec["dy"] = res[1], mx, my
            out.append(t["last"].copy())
            tags.append(tr._tag(t, s, f, sp.min_hits, FOLLOWED))
            continue
        rec["sad"], rec["dx"], rec["dy"] = (res[1] if res[0] == 2 else -1), 0, 0
        t["missed"] += 1
        if t["missed"] > sp.max_missed:
            ended.append(t.copy())
            stream.table[s] = np.zeros((), tr.TRACK)
            stream.records[s] = np.zeros((), FOLLOW)
    return (np.array(out, tr.FACE) if out else np.zeros(0, tr.FACE), np.array(tags, tr.TAG) if tags else np.zeros(0, tr.TAG),
            np.array(ended, tr.TRACK) if ended else np.zeros(0, tr.TRACK))


def read_templates(stream):
    """what rf_tracker_read_follow returns for templates: zeros where the record is not valid"""
    out = stream.templates.copy()
    out[stream.records["valid"] == 0] = 0
    return out
