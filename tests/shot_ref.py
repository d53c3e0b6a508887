"""numpy restatement of the best-shot gallery ("Best-shot gallery"): a helper, not a test.

A tracker with a gallery keeps, per track slot, the face-batch crop of the track's best shot and an rf_shot record.  The frame step is
track_ref's, untouched; two rules are added.  Keep: a face whose tag carries BEST sets its track's slot -- the entry becomes the bytes
the face batch writes for that face of that image (face_batch_ref / face_aa_ref, untouched), the record {id, frame, matrix}.  Deliver:
every ended track that makes it into the image's ended list gets the entry and record of its slot, zeros when it never had a best shot.
Within a frame the order is the tracker's: age (which ends tracks), then open.  The kernels (retinaface_amd/csrc/kernels.hip
shot_deliver_kernel / shot_keep_kernel), retinaface_amd/csrc/shot.h and the host entry point rf_shot_resolve are checked byte for byte
against this file: the records below have the C layout.
"""
import numpy as np

import face_aa_ref
import face_batch_ref
import track_ref

SHOT = np.dtype([("id", "<i8"), ("frame", "<i8"), ("matrix", "<f8", 6)])
assert SHOT.itemsize == 64
NONE, STORED, LAUNCH = 0, 1, 2
BEST, NEW = track_ref.BEST, track_ref.NEW


class Gallery:
    """a tracker with a gallery: n_streams track_ref.Stream objects, their entries and records"""

    def __init__(self, spec, n_streams, fmt=face_batch_ref.U8_HWC, *, size=112, rgb=0, mean=None, scale=None, max_faces=256, antialias=0,
                 aa_max=4):
        self.spec = spec
        self.streams = [track_ref.Stream(spec) for _ in range(n_streams)]
        self.fmt, self.size, self.rgb, self.mean, self.scale = fmt, size, rgb, mean, scale
        self.max_faces, self.antialias, self.aa_max = max_faces, antialias, aa_max
        self.bytes_per_face = 3 * size * size * np.dtype(face_batch_ref.DTYPES[fmt]).itemsize
        self.entries = np.zeros((n_streams, spec.max_tracks, self.bytes_per_face), np.uint8)
        self.records = np.zeros((n_streams, spec.max_tracks), SHOT)

    def face_bytes(self, frame, row, cs=1.0):
        """one face's tensor of rf_face_batch_device as bytes, and its matrix"""
        kw = dict(size=self.size, rgb=self.rgb, mean=self.mean, scale=self.scale, scales=[np.float32(cs)])
        rows = [np.asarray(row, np.float32).reshape(1, 15)]
        if self.antialias:
            t, m, _ = face_aa_ref.batch([frame], rows, self.fmt, aa_max=self.aa_max, **kw)
        else:
            t, m, _ = face_batch_ref.batch([frame], rows, self.fmt, **kw)
        return np.ascontiguousarray(t[0]).view(np.uint8).reshape(-1), m[0]

    def step(self, s, frame, faces, coord_scale=1.0, quality=None, cap_ended=0):
        """one image of stream s.  frame: H x W x 3 u8 or None (a frame with no faces); faces: (count, 15) rows.
        Returns (tags, ended (all of them), overflow, shots (min(e, cap_ended), bytes_per_face) u8, info (same,) SHOT)."""
        st = self.streams[s]
        rows = np.asarray(faces, np.float32).reshape(-1, 15)
        if frame is None:
            rows = rows[:0]
        f = st.frames
        tags, ended, over = track_ref.step(st, rows, coord_scale, quality, min(self.max_faces, track_ref.MAX_FACES))

        def keep(k):
            slot = int(tags[k]["slot"])
            self.entries[s, slot], m = self.face_bytes(frame, rows[k], coord_scale)
            self.records[s, slot] = (tags[k]["id"], f, m)

        for k in range(len(tags)):                                  # matched faces: before the step ages and ends tracks
            if tags[k]["flags"] & BEST and not tags[k]["flags"] & NEW:
                keep(k)
        ne = min(len(ended), cap_ended)
        shots = np.zeros((ne, self.bytes_per_face), np.uint8)
        info = np.zeros(ne, SHOT)
        for e in range(ne):
            t = ended[e]
            if t["best_frame"] < 0:
                continue
            hit = np.nonzero((self.records[s]["id"] == t["id"]) & (self.records[s]["frame"] == t["best_frame"]))[0]
            assert len(hit) == 1
            shots[e], info[e] = self.entries[s, hit[0]], self.records[s, hit[0]]
        for k in range(len(tags)):                                  # new tracks: a slot freed in this frame is theirs now
            if tags[k]["flags"] & BEST and tags[k]["flags"] & NEW:
                keep(k)
        return tags, ended, over, shots, info

    def update(self, frames, stream_of_image, faces, counts, cap_per_image, coord_scale=None, quality=None, cap_ended=0):
        """rf_track_shots_device.  faces: (n, cap_per_image, 15) float32 or (n, cap_per_image) FACE; quality: None or (n, max_faces).
        Returns (tags (n, cap_per_image), ended (n, cap_ended), ended_counts, truncated, shots (n, cap_ended, bytes_per_face), info
        (n, cap_ended), delivered (n,): how many of each image's shots and records are written)."""
        n = len(stream_of_image)
        faces = track_ref.rows_of(np.ascontiguousarray(faces)).reshape(n, cap_per_image, 15) if n else np.zeros((0, cap_per_image, 15), np.float32)
        tags = np.zeros((n, cap_per_image), track_ref.TAG)
        ended = np.zeros((n, max(cap_ended, 0)), track_ref.TRACK)
        ended_counts = np.zeros(n, np.int32)
        shots = np.zeros((n, max(cap_ended, 0), self.bytes_per_face), np.uint8)
        info = np.zeros((n, max(cap_ended, 0)), SHOT)
        delivered = np.zeros(n, np.int32)
        truncated = False
        for i in range(n):
            s = int(stream_of_image[i])
            if s < 0:
                continue
            have = min(int(counts[i]), cap_per_image)
            q = quality[i, :min(have, self.max_faces)] if quality is not None else None
            t, e, over, sh, inf = self.step(s, frames[i], faces[i, :have], 1.0 if coord_scale is None else coord_scale[i], q, cap_ended)
            tags[i, :len(t)] = t
            if frames[i] is None:
                tags[i] = np.zeros((), track_ref.TAG)
            ended_counts[i] = len(e)
            delivered[i] = len(sh)
            ended[i, :len(sh)] = e[:cap_ended]
            shots[i, :len(sh)], info[i, :len(sh)] = sh, inf
            truncated = truncated or over or len(e) > cap_ended
        return tags, ended, ended_counts, truncated, shots, info, delivered

    def read(self, s):
        """rf_tracker_read_shots: (entries, records) of stream s; zeros where the slot holds no shot"""
        tb = self.streams[s].table
        ok = (tb["id"] != 0) & (tb["best_frame"] >= 0) & (self.records[s]["id"] == tb["id"]) & (self.records[s]["frame"] == tb["best_frame"])
        ent, rec = self.entries[s].copy(), self.records[s].copy()
        ent[~ok] = 0
        rec[~ok] = np.zeros((), SHOT)
        return ent, rec

    def flush(self, s):
        """rf_tracker_flush_shots: (ended, shots, info) slot-ascending"""
        ent, rec = self.read(s)
        live = self.streams[s].table["id"] != 0
        ended = track_ref.flush(self.streams[s])
        self.records[s] = np.zeros((), SHOT)
        return ended, ent[live], rec[live]

    def reset(self, s):
        self.streams[s] = track_ref.Stream(self.spec)
        self.records[s] = np.zeros((), SHOT)


def resolve(max_tracks, tags, counts, ended, ended_counts, first_frame, records, matrices=None):
    """rf_shot_resolve for one stream's n images of one launch.  tags: (n, cap_per_image) TAG; ended: (n, cap_ended) TRACK; records:
    (max_tracks,) SHOT before the launch; matrices: None (zero matrices) or (n, cap_per_image, 6) float64.
    Returns (delivered, source (n, cap_ended, 3) int32, owner (max_tracks, 2) int32, records after)."""
    n, cap = tags.shape
    cap_ended = ended.shape[1]
    before = records.copy()
    rec = records.copy()
    now = {}                                                        # slot -> (id, frame, image, face)
    source = np.full((n, cap_ended, 3), -1, np.int32)
    delivered = 0
    for i in range(n):
        m = min(int(counts[i]), cap, track_ref.MAX_FACES)
        g = tags[i]

        def keep(k):
            if 0 <= g[k]["slot"] < max_tracks:
                now[int(g[k]["slot"])] = (int(g[k]["id"]), first_frame + i, i, k)

        for k in range(m):
            if g[k]["flags"] & BEST and not g[k]["flags"] & NEW and g[k]["id"] != 0:
                keep(k)
        for e in range(min(int(ended_counts[i]), cap_ended)):
            t = ended[i, e]
            tid, bf = int(t["id"]), int(t["best_frame"])
            src = (NONE, 0, 0)
            if 0 <= bf < first_frame:
                hit = [s for s in range(max_tracks) if tid != 0 and before[s]["id"] == tid and before[s]["frame"] == bf]
                if hit:
                    src = (STORED, hit[0], 0)
            elif bf >= first_frame and bf - first_frame < n:
                a = bf - first_frame
                ma = min(int(counts[a]), cap, track_ref.MAX_FACES)
                hit = [k for k in range(ma) if tid != 0 and tags[a, k]["id"] == tid and tags[a, k]["flags"] & BEST]
                if hit:
                    src = (LAUNCH, a, hit[0])
            source[i, e] = src
            delivered += 1
            for s in range(max_tracks):
                if s in now and now[s][0] == tid:
                    del now[s]
                if rec[s]["id"] == tid:
                    rec[s] = np.zeros((), SHOT)
        for k in range(m):
            if g[k]["flags"] & BEST and g[k]["flags"] & NEW and g[k]["id"] != 0:
                keep(k)
    owner = np.full((max_tracks, 2), -1, np.int32)
    for s, (tid, fr, i, k) in now.items():
        owner[s] = (i, k)
        rec[s] = (tid, fr, np.zeros(6) if matrices is None else matrices[i, k])
    return delivered, source, owner, rec
