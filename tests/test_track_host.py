"""Face tracks on the host: rf_track_step (retinaface_amd/csrc/track.h, the code the kernel runs) against tests/track_ref.py, byte for byte."""
import ctypes as C

import numpy as np
import pytest

import track_ref as tr
from retinaface_amd import _lib

f32 = np.float32
SCORES = (np.arange(31, dtype=np.float32) + f32(1)) / f32(32)        # 31 values: ties abound


def _spec(**kw):
    s = _lib.rf_track_spec()
    s.struct_size = C.sizeof(_lib.rf_track_spec)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class HostStream:
    """a caller-held table driven through rf_track_step"""

    def __init__(self, lib, max_tracks=64, **kw):
        self.lib, self.spec = lib, _spec(max_tracks=max_tracks, **kw)
        self.table = np.zeros(max_tracks or 64, tr.TRACK)
        self.frames, self.next_id = C.c_int64(0), C.c_int64(1)

    def step(self, faces, scale=1.0, quality=None, max_faces=256, cap_ended=8):
        faces = np.ascontiguousarray(faces)
        count = len(faces)
        tags = np.zeros(max(count, 1), tr.TAG)
        ended = np.zeros(max(cap_ended, 1), tr.TRACK)
        ne = C.c_int(-1)
        rc = self.lib.rf_track_step(C.byref(self.spec), _ptr(self.table, _lib.rf_track), C.byref(self.frames), C.byref(self.next_id),
                                    _ptr(faces, _lib.rf_face), count, scale, _ptr(quality, _lib.rf_face_quality) if quality is not None else None,
                                    max_faces, _ptr(tags, _lib.rf_track_tag), _ptr(ended, _lib.rf_track), cap_ended, C.byref(ne))
        return rc, tags[:count], ended[:min(max(ne.value, 0), cap_ended)], ne.value


def face(score, x, y, w, h=None):
    h = w if h is None else h
    r = np.zeros(15, np.float32)
    r[0], r[1], r[2], r[3], r[4] = score, x, y, x + w, y + h
    r[5:10] = x + np.array([0.3, 0.7, 0.5, 0.35, 0.65], np.float32) * f32(w)
    r[10:15] = y + np.array([0.4, 0.4, 0.6, 0.8, 0.8], np.float32) * f32(h)
    return r


def by_score(rows):
    rows = np.asarray(rows, np.float32).reshape(-1, 15)
    return tr.faces_array(rows[np.argsort(-rows[:, 0], kind="stable")])


def sequence(seed, n_frames, n_people, max_missed):
    """seeded frames of boxes that drift, appear, vanish for 1 .. max_missed + 2 frames and cross each other"""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0, 600, (n_people, 2)).astype(np.float32)
    vel = rng.uniform(-14, 14, (n_people, 2)).astype(np.float32)
    size = rng.uniform(24, 90, n_people).astype(np.float32)
    hidden = np.zeros(n_people, int)
    start = rng.integers(0, max(n_frames // 2, 1), n_people)
    frames = []
    for t in range(n_frames):
        rows = []
        for p in range(n_people):
            pos[p] += vel[p]
            if t < start[p]:
                continue
            if hidden[p] == 0 and rng.random() < 0.12:
                hidden[p] = int(rng.integers(1, max_missed + 3))
            if hidden[p] > 0:
                hidden[p] -= 1
                continue
            rows.append(face(SCORES[rng.integers(0, 31)], pos[p, 0], pos[p, 1], size[p], size[p] * f32(1.2)))
        frames.append(by_score(rows) if rows else np.zeros(0, tr.FACE))
    return frames


def test_struct_sizes():
    assert C.sizeof(_lib.rf_track) == 176 == tr.TRACK.itemsize
    assert C.sizeof(_lib.rf_track_tag) == 24 == tr.TAG.itemsize
    assert C.sizeof(_lib.rf_track_spec) == 24


@pytest.mark.parametrize("seed,max_tracks,max_missed,min_hits,new_score,n_people", [
    (1, 64, 2, 3, 0.0, 12), (2, 8, 1, 2, 0.0, 14), (3, 256, 4, 1, 0.25, 40), (4, 5, -1, -1, 0.0, 9), (5, 0, 0, 0, 0.5, 20)])
def test_sequences_match_the_reference(built_lib, seed, max_tracks, max_missed, min_hits, new_score, n_people):
    spec = tr.Spec(max_tracks, 0.0, max_missed, min_hits, new_score)
    ref = tr.Stream(spec)
    got = HostStream(built_lib, max_tracks, max_missed=max_missed, min_hits=min_hits, new_score=new_score)
    seen, last_id, any_end, any_over = set(), 0, False, False
    for faces in sequence(seed, 40, n_people, spec.max_missed):
        tags, ended, over = tr.step(ref, faces, 1.0)
        rc, gtags, gended, ne = got.step(faces, cap_ended=4)
        assert gtags.tobytes() == tags.tobytes()
        assert ne == len(ended) and gended.tobytes() == ended[:4].tobytes()
        assert rc == (_lib.RF_ERR_TRUNCATED if over or len(ended) > 4 else 0)
        assert got.table.tobytes() == ref.table.tobytes()
        assert (got.frames.value, got.next_id.value) == (ref.frames, ref.next_id)
        for g in gtags[(gtags["flags"] & tr.NEW) != 0]:            # ids are unique and increase
            assert g["id"] > last_id and g["id"] not in seen
            last_id = int(g["id"]); seen.add(last_id)
        any_end, any_over = any_end or len(ended) > 0, any_over or over
    assert any_end and len(seen) > 3
    if max_tracks in (5, 8):
        assert any_over


def test_equal_overlap_goes_to_the_lower_slot(built_lib):
    s = HostStream(built_lib, 8)
    s.step(by_score([face(0.9, 100, 100, 40), face(0.8, 120, 100, 40)]))           # slots 0 and 1
    mid = by_score([face(0.7, 110, 100, 40)])                                       # the same overlap with both
    a = tr.iou(tr.rows_of(mid)[0, 1:5], np.array([100, 100, 140, 140], np.float32))
    b = tr.iou(tr.rows_of(mid)[0, 1:5], np.array([120, 100, 160, 140], np.float32))
    assert a == b and a > 0.3
    _, tags, _, _ = s.step(mid)
    assert tags[0]["slot"] == 0 and tags[0]["id"] == 1


def test_overlap_equal_to_min_iou_matches_one_ulp_below_does_not(built_lib):
    box0 = np.array([100, 100, 140, 140], np.float32)
    probe = by_score([face(0.9, 118, 100, 40)])
    v = tr.iou(tr.rows_of(probe)[0, 1:5], box0)
    assert 0 < v < 1
    for min_iou, want_match in ((v, True), (np.nextafter(v, f32(2)), False), (np.nextafter(v, f32(0)), True)):
        s = HostStream(built_lib, 4, min_iou=float(min_iou))
        s.step(by_score([face(0.9, 100, 100, 40)]))
        _, tags, _, _ = s.step(probe)
        assert (tags[0]["id"] == 1) == want_match, (min_iou, tags)
        assert bool(tags[0]["flags"] & tr.NEW) == (not want_match)


def test_a_track_ends_when_missed_first_exceeds_max_missed(built_lib):
    s = HostStream(built_lib, 4, max_missed=2)
    s.step(by_score([face(0.9, 10, 10, 30)]))
    for missed in (1, 2):
        rc, _, ended, ne = s.step(np.zeros(0, tr.FACE))
        assert (rc, ne) == (0, 0) and s.table[0]["missed"] == missed and s.table[0]["id"] == 1
    rc, _, ended, ne = s.step(np.zeros(0, tr.FACE))
    assert ne == 1 and ended[0]["id"] == 1 and ended[0]["missed"] == 3 and s.table[0]["id"] == 0
    assert s.table.tobytes() == bytes(4 * 176)


def test_a_slot_freed_in_a_frame_is_reused_in_that_frame(built_lib):
    s = HostStream(built_lib, 1, max_missed=-1)
    s.step(by_score([face(0.9, 10, 10, 30)]))
    rc, tags, ended, ne = s.step(by_score([face(0.9, 400, 400, 30)]))
    assert rc == 0 and ne == 1 and ended[0]["id"] == 1
    assert tags[0]["id"] == 2 and tags[0]["slot"] == 0 and tags[0]["flags"] & tr.NEW


def test_full_table_overflows_and_truncates(built_lib):
    s = HostStream(built_lib, 2)
    rc, tags, _, _ = s.step(by_score([face(0.9, 10, 10, 30), face(0.8, 100, 10, 30), face(0.7, 200, 10, 30)]))
    assert rc == _lib.RF_ERR_TRUNCATED
    assert [int(t["id"]) for t in tags] == [1, 2, 0]
    assert tags[2]["flags"] == tr.UNTRACKED | tr.OVERFLOW and tags[2]["slot"] == -1
    rc, _, ended, ne = HostStream(built_lib, 4, max_missed=-1).step(np.zeros(0, tr.FACE), cap_ended=0)
    assert (rc, ne) == (0, 0)


def test_cut_ended_list_truncates(built_lib):
    s = HostStream(built_lib, 4, max_missed=-1)
    s.step(by_score([face(0.9, 10, 10, 30), face(0.8, 100, 10, 30), face(0.7, 200, 10, 30)]))
    rc, _, ended, ne = s.step(np.zeros(0, tr.FACE), cap_ended=1)
    assert rc == _lib.RF_ERR_TRUNCATED and ne == 3 and len(ended) == 1 and ended[0]["id"] == 1


def test_new_score_holds_faces_back(built_lib):
    s = HostStream(built_lib, 4, new_score=0.5)
    _, tags, _, _ = s.step(by_score([face(0.75, 10, 10, 30), face(0.5, 100, 10, 30), face(0.25, 200, 10, 30)]))
    assert [int(t["id"]) for t in tags] == [1, 2, 0] and tags[2]["flags"] == tr.UNTRACKED
    _, tags, _, _ = s.step(by_score([face(0.25, 10, 10, 30)]))             # a track once open is matched by any score
    assert tags[0]["id"] == 1


def test_best_shot_tie_keeps_the_earlier_frame(built_lib):
    s = HostStream(built_lib, 4)
    _, t0, _, _ = s.step(by_score([face(0.5, 10, 10, 30)]))
    _, t1, _, _ = s.step(by_score([face(0.5, 11, 10, 30)]))
    _, t2, _, _ = s.step(by_score([face(0.75, 12, 10, 30)]))
    assert t0[0]["flags"] & tr.BEST and not t1[0]["flags"] & tr.BEST and t2[0]["flags"] & tr.BEST
    assert s.table[0]["best_frame"] == 2 and s.table[0]["best"]["x1"] == 12
    s = HostStream(built_lib, 4)
    s.step(by_score([face(0.5, 10, 10, 30)]))
    s.step(by_score([face(0.5, 11, 10, 30)]))
    assert s.table[0]["best_frame"] == 0 and s.table[0]["best"]["x1"] == 10


def test_a_face_that_fails_its_gate_is_never_the_best_shot(built_lib):
    s, ref = HostStream(built_lib, 4), tr.Stream(tr.Spec(4))
    sharp = [(5.0, 2), (9.0, 0), (7.0, 0), (9.0, 0), (99.0, 16)]
    for t, (v, flags) in enumerate(sharp):
        q = np.zeros(1, tr.QUALITY)
        q["sharpness"], q["flags"] = v, flags
        faces = by_score([face(0.9, 10 + t, 10, 30)])
        _, tags, _, _ = s.step(faces, quality=q)
        rtags, _, _ = tr.step(ref, faces, 1.0, q)
        assert tags.tobytes() == rtags.tobytes() and s.table.tobytes() == ref.table.tobytes()
        assert bool(tags[0]["flags"] & tr.BEST) == (t in (1,))
        assert s.table[0]["best_frame"] == (-1 if t == 0 else 1)
    assert s.table[0]["best_value"] == 9.0


def test_nan_face_matches_nothing_and_opens_a_track(built_lib):
    s, ref = HostStream(built_lib, 4), tr.Stream(tr.Spec(4))
    for rows in ([face(0.9, 10, 10, 30)], [face(0.9, 10, 10, 30) * np.array([1] + [np.nan] * 14, np.float32), face(0.8, 11, 10, 30)],
                 [face(0.9, 12, 10, 30)]):
        faces = by_score(rows)
        _, tags, _, _ = s.step(faces)
        rtags, _, _ = tr.step(ref, faces)
        assert tags.tobytes() == rtags.tobytes() and s.table.tobytes() == ref.table.tobytes()
    assert s.next_id.value == 3 and s.table[1]["id"] == 2 and np.isnan(s.table[1]["last"]["x1"]) and s.table[1]["missed"] == 1
    assert s.table[0]["hits"] == 3


def test_scale_maps_every_coordinate_once(built_lib):
    s, ref = HostStream(built_lib, 4), tr.Stream(tr.Spec(4))
    faces = by_score([face(0.9, 10.3, 10.7, 30.1)])
    sc = float(f32(1280) / f32(448))
    s.step(faces, scale=sc)
    tr.step(ref, faces, sc)
    assert s.table.tobytes() == ref.table.tobytes()
    assert s.table[0]["last"]["x1"] == f32(10.3) * f32(sc) and s.table[0]["last"]["score"] == f32(0.9)


def test_max_faces_leaves_the_rest_untracked(built_lib):
    s = HostStream(built_lib, 8)
    _, tags, _, _ = s.step(by_score([face(0.9, 10, 10, 30), face(0.8, 100, 10, 30), face(0.7, 200, 10, 30)]), max_faces=2)
    assert [int(t["id"]) for t in tags] == [1, 2, 0]
    assert tags[2].tobytes() == np.array((0, -1, 0, 0, tr.UNTRACKED), tr.TAG).tobytes()


def test_refusals(built_lib):
    s = HostStream(built_lib, 4)
    faces = by_score([face(0.9, 10, 10, 30)])
    before = s.table.tobytes()

    def rc_with(**kw):
        s.spec = _spec(**kw)
        return s.step(faces)[0]

    assert rc_with(max_tracks=4) == 0
    s = HostStream(built_lib, 4); s.spec.struct_size = 20
    assert s.step(faces)[0] == _lib.RF_ERR_INVALID_ARG and s.table.tobytes() == before and s.frames.value == 0
    for bad in (dict(max_tracks=257), dict(max_tracks=-1), dict(min_iou=float("nan")), dict(min_iou=-0.1), dict(min_iou=1.5),
                dict(min_iou=float("inf")), dict(new_score=-1.0), dict(new_score=float("nan"))):
        s = HostStream(built_lib, 4)
        s.spec = _spec(**bad)
        assert s.step(faces)[0] == _lib.RF_ERR_INVALID_ARG, bad
        assert s.table.tobytes() == before and (s.frames.value, s.next_id.value) == (0, 1)
    d = HostStream(built_lib, 0)                        # max_tracks 0 = 64; a NULL spec is all defaults
    assert len(d.table) == 64 and d.step(faces)[0] == 0 and d.table[0]["id"] == 1
    assert d.step(faces, max_faces=0)[0] == _lib.RF_ERR_INVALID_ARG
    # n_streams is checked before the handle is looked at: no GPU needed
    out = C.c_void_p()
    for n_streams in (0, -1, 1025):
        assert built_lib.rf_tracker_create(None, None, n_streams, C.byref(out)) == _lib.RF_ERR_INVALID_ARG and not out.value
