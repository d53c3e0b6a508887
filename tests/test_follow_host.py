"""Followed tracks on the host: rf_follow_geometry / rf_follow_template / rf_follow_search and the two whole steps
rf_track_step_follow_key / rf_track_step_follow (retinaface_amd/csrc/follow.h, the code the kernels run) against tests/follow_ref.py,
byte for byte; the refusals; the behaviour cases; the claim on real pixels (a pan over the base frame, boxes from the fp32 oracle on
the key frames only); and the stand-alone sanitizer program."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import follow_ref as fr
import track_ref as tr
from conftest import ROOT, STEMS
from retinaface_amd import _lib
from test_track_host import _ptr, _spec, by_score, face

f32 = np.float32
EMPTY = np.zeros(0, tr.FACE)


def _fspec(**kw):
    s = _lib.rf_follow_spec()
    s.struct_size = C.sizeof(_lib.rf_follow_spec)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def strided(img, pad=11, offset=1):
    """the same pixels in a buffer whose row step is larger than cols * 3 and whose base address is odd"""
    rows, cols = img.shape[:2]
    step = cols * 3 + pad
    buf = np.full(rows * step + offset + 8, 0xEE, np.uint8)
    out = np.ndarray((rows, cols, 3), np.uint8, buffer=buf, offset=offset, strides=(step, 3, 1))
    out[...] = img
    assert out.ctypes.data % 2 == 1 or offset % 2 == 0
    return out


def canvas(rows, cols, seed):
    """seeded smooth noise with blobs, u8 BGR"""
    rng = np.random.default_rng(seed)
    low = rng.uniform(40, 200, (rows // 8 + 2, cols // 8 + 2, 3))
    img = np.kron(low, np.ones((8, 8, 1)))[:rows, :cols]
    for _ in range(3):                                          # a cheap blur: the noise becomes smooth
        img = (img + np.roll(img, 3, 0) + np.roll(img, 3, 1) + np.roll(img, -3, 0) + np.roll(img, -3, 1)) / 5
    yy, xx = np.mgrid[0:rows, 0:cols]
    for _ in range(12):
        cy, cx, r = rng.uniform(0, rows), rng.uniform(0, cols), rng.uniform(4, 18)
        img += rng.uniform(-70, 70, 3) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))[..., None]
    img += rng.uniform(-2, 2, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def window(big, rows, cols, x0, y0):
    return strided(big[y0:y0 + rows, x0:x0 + cols])


def frame_args(frame):
    if frame is None:
        return None, 0, 0, 0
    return frame.ctypes.data, frame.shape[0], frame.shape[1], frame.strides[0]


class FollowHost:
    """a caller-held table, records and templates driven through the two host steps"""

    def __init__(self, lib, max_tracks=8, radius=0, max_mad=0, max_run=0, **kw):
        self.lib, self.spec, self.fspec = lib, _spec(max_tracks=max_tracks, **kw), _fspec(radius=radius, max_mad=max_mad, max_run=max_run)
        T = max_tracks or 64
        self.table = np.zeros(T, tr.TRACK)
        self.records = np.zeros(T, fr.FOLLOW)
        self.templates = np.zeros((T, 32, 32), np.uint8)
        self.frames, self.next_id = C.c_int64(0), C.c_int64(1)

    def key(self, frame, faces, scale=1.0, cap_ended=8):
        faces = np.ascontiguousarray(faces)
        count = len(faces)
        tags = np.zeros(max(count, 1), tr.TAG)
        ended = np.zeros(max(cap_ended, 1), tr.TRACK)
        ne = C.c_int(-1)
        rc = self.lib.rf_track_step_follow_key(C.byref(self.spec), _ptr(self.table, _lib.rf_track), _ptr(self.records, _lib.rf_track_follow),
                                               self.templates.ctypes.data, C.byref(self.frames), C.byref(self.next_id), *frame_args(frame),
                                               _ptr(faces, _lib.rf_face), count, scale, None, 256, _ptr(tags, _lib.rf_track_tag),
                                               _ptr(ended, _lib.rf_track), cap_ended, C.byref(ne))
        return rc, tags[:count if frame is not None else 0], ended[:min(max(ne.value, 0), cap_ended)], ne.value

    def follow(self, frame, cap=None, cap_ended=8):
        cap = len(self.table) if cap is None else cap
        out = np.zeros(max(cap, 1), tr.FACE)
        tags = np.zeros(max(cap, 1), tr.TAG)
        ended = np.zeros(max(cap_ended, 1), tr.TRACK)
        cnt, ne = C.c_int(-1), C.c_int(-1)
        rc = self.lib.rf_track_step_follow(C.byref(self.spec), C.byref(self.fspec), _ptr(self.table, _lib.rf_track),
                                           _ptr(self.records, _lib.rf_track_follow), self.templates.ctypes.data, C.byref(self.frames),
                                           *frame_args(frame), _ptr(out, _lib.rf_face), _ptr(tags, _lib.rf_track_tag), cap, C.byref(cnt),
                                           _ptr(ended, _lib.rf_track), cap_ended, C.byref(ne))
        k = min(max(cnt.value, 0), cap)
        return rc, out[:k], tags[:k], cnt.value, ended[:min(max(ne.value, 0), cap_ended)], ne.value

    def masked_templates(self):
        t = self.templates.copy()
        t[self.records["valid"] == 0] = 0
        return t


def pair(lib, max_tracks=8, radius=0, max_mad=0, max_run=0, **kw):
    spec = tr.Spec(max_tracks, kw.get("min_iou", 0.0), kw.get("max_missed", 0), kw.get("min_hits", 0), kw.get("new_score", 0.0))
    return FollowHost(lib, max_tracks, radius, max_mad, max_run, **kw), fr.Stream(spec, fr.FollowSpec(radius, max_mad, max_run))


def same_state(got, ref, where=""):
    assert got.table.tobytes() == ref.table.tobytes(), where
    assert got.records.tobytes() == ref.records.tobytes(), (where, got.records, ref.records)
    assert got.masked_templates().tobytes() == fr.read_templates(ref).tobytes(), where
    assert (got.frames.value, got.next_id.value) == (ref.frames, ref.next_id), where


def key_both(got, ref, frame, faces, **kw):
    rc, tags, ended, ne = got.key(frame, faces, **kw)
    rtags, rended, rover = fr.key_step(ref, frame, faces)
    assert tags.tobytes() == rtags.tobytes() and ne == len(rended)
    same_state(got, ref, "key")
    return rc, tags


def follow_both(got, ref, frame, cap=None, cap_ended=8):
    rc, out, tags, cnt, ended, ne = got.follow(frame, cap, cap_ended)
    rout, rtags, rended = fr.follow_step(ref, frame)
    cap = len(got.table) if cap is None else cap
    assert cnt == len(rout) and ne == len(rended)
    assert out.tobytes() == rout[:cap].tobytes() and tags.tobytes() == rtags[:cap].tobytes()
    assert ended.tobytes() == rended[:cap_ended].tobytes()
    assert rc == (_lib.RF_ERR_TRUNCATED if cnt > cap or ne > cap_ended else 0)
    same_state(got, ref, "follow")
    return rc, out, tags, ended


# boxes (x, y, w, h) for a rows x cols frame: q = 1 (20 and 32 px), q = 2 (33 px), a 130 px box, one larger than the frame, one over each
# edge and over a corner
def boxes_for(rows, cols):
    return [(30.3, 40.6, 19, 19), (50, 30, 31, 31), (20.5, 10.2, 32, 32), (8, 8, 129, 80), (-20, -30, cols + 60, rows + 50),
            (-12, 40, 30, 30), (cols - 14, 30, 28, 28), (40, -9, 26, 26), (60, rows - 10, 24, 24), (cols - 8, rows - 6, 40, 40)]


def test_struct_sizes():
    assert C.sizeof(_lib.rf_follow_spec) == 20
    assert C.sizeof(_lib.rf_track_follow) == 32 == fr.FOLLOW.itemsize
    assert _lib.RF_TRACK_FOLLOWED == 32 == fr.FOLLOWED


@pytest.mark.parametrize("rows,cols,seed", [(96, 128, 1), (200, 240, 2)])
def test_geometry_template_and_search_match_the_reference(built_lib, rows, cols, seed):
    big = canvas(rows + 40, cols + 40, seed)
    key, nxt = window(big, rows, cols, 20, 20), window(big, rows, cols, 23, 18)          # the content moves by (-3, +2)
    out3, out4 = (C.c_int32 * 3)(), (C.c_int32 * 4)()
    for (x, y, w, h) in boxes_for(rows, cols):
        box = np.array([x, y, x + w, y + h], np.float32)
        geo = fr.geometry(box)
        assert built_lib.rf_follow_geometry(_ptr(box, C.c_float), out3) == 1 and tuple(out3) == geo, (box, tuple(out3), geo)
        q, ox, oy = geo
        tpl = np.zeros((32, 32), np.uint8)
        assert built_lib.rf_follow_template(*frame_args(key), q, ox, oy, tpl.ctypes.data) == 0
        assert tpl.tobytes() == fr.template(key, q, ox, oy).tobytes(), box
        for R in (1, 8, 16):
            assert built_lib.rf_follow_search(*frame_args(nxt), tpl.ctypes.data, q, ox, oy, R, out4) == 0
            assert tuple(out4) == fr.search(nxt, tpl, q, ox, oy, R), (box, R)
    # q = 1 and 2 inside the frame: the shift is found exactly / to the nearest cell
    for (x, y, w, h), want in (((50, 30, 31, 31), (-3, 2)), ((20.5, 10.2, 32, 32), (-1, 1))):
        q, ox, oy = fr.geometry(np.array([x, y, x + w, y + h], np.float32))
        st, sad, du, dv = fr.search(nxt, fr.template(key, q, ox, oy), q, ox, oy, 8)
        assert st == 2 and (du, dv) in ((want[0], want[1]), (want[0] - (q == 2), want[1])), (q, du, dv)


def test_invalid_geometries(built_lib):
    out3 = (C.c_int32 * 3)()
    for box in ([np.nan, 0, 10, 10], [0, np.inf, 10, 10], [0, 0, -np.inf, 10], [10, 10, 8.5, 20], [10, 10, 20, 8.9]):
        b = np.array(box, np.float32)
        assert fr.geometry(b) is None
        assert built_lib.rf_follow_geometry(_ptr(b, C.c_float), out3) == 0 and tuple(out3) == (0, 0, 0)
    for box in ([10, 10, 10, 10], [10.2, 10.2, 10.9, 10.9], [-1e9, -1e9, 1e9, 1e9], [-5000, 0, -4090, 10]):      # zero size: one pixel; clamped
        b = np.array(box, np.float32)
        assert built_lib.rf_follow_geometry(_ptr(b, C.c_float), out3) == 1 and tuple(out3) == fr.geometry(b), box
    assert fr.geometry([-1e9, -1e9, 1e9, 1e9])[0] == 385
    assert built_lib.rf_follow_geometry(None, out3) == _lib.RF_ERR_INVALID_ARG


def test_spec_defaults_and_refusals(built_lib):
    frame = strided(canvas(96, 128, 3))
    faces = by_score([face(0.9, 40, 30, 31)])
    # defaults: a NULL follow spec and an all-zero one are radius 8, max_mad 16, max_run 8
    for use_null in (True, False):
        got, ref = pair(built_lib, 4)
        key_both(got, ref, frame, faces)
        if use_null:
            out, tags, ended = np.zeros(4, tr.FACE), np.zeros(4, tr.TAG), np.zeros(4, tr.TRACK)
            cnt, ne = C.c_int(), C.c_int()
            assert built_lib.rf_track_step_follow(C.byref(got.spec), None, _ptr(got.table, _lib.rf_track), _ptr(got.records, _lib.rf_track_follow),
                                                  got.templates.ctypes.data, C.byref(got.frames), *frame_args(frame), _ptr(out, _lib.rf_face),
                                                  _ptr(tags, _lib.rf_track_tag), 4, C.byref(cnt), _ptr(ended, _lib.rf_track), 4, C.byref(ne)) == 0
            fr.follow_step(ref, frame)
            same_state(got, ref)
        else:
            follow_both(got, ref, frame)
        assert got.records[0]["run"] == 1
    # bad follow specs change nothing
    for bad in (dict(struct_size=16), dict(reserved=1), dict(radius=17), dict(radius=-1), dict(max_mad=256), dict(max_mad=-1),
                dict(max_run=65537), dict(max_run=-1)):
        got, ref = pair(built_lib, 4)
        key_both(got, ref, frame, faces)
        before = (got.table.tobytes(), got.records.tobytes(), got.frames.value)
        for k, v in bad.items():
            setattr(got.fspec, k, v)
        assert got.follow(frame)[0] == _lib.RF_ERR_INVALID_ARG, bad
        assert (got.table.tobytes(), got.records.tobytes(), got.frames.value) == before
    for ok in (dict(radius=16), dict(radius=1), dict(max_mad=255), dict(max_run=65536)):
        got, ref = pair(built_lib, 4, **ok)
        key_both(got, ref, frame, faces)
        follow_both(got, ref, frame)
    # bad track spec, bad frames, NULL state
    got, _ = pair(built_lib, 4)
    got.spec = _spec(max_tracks=257)
    assert got.key(frame, faces)[0] == _lib.RF_ERR_INVALID_ARG and got.follow(frame)[0] == _lib.RF_ERR_INVALID_ARG
    got, _ = pair(built_lib, 4)
    tags, ended, ne, cnt = np.zeros(1, tr.TAG), np.zeros(1, tr.TRACK), C.c_int(0), C.c_int(0)
    tail = (_ptr(faces, _lib.rf_face), 1, 1.0, None, 256, _ptr(tags, _lib.rf_track_tag), _ptr(ended, _lib.rf_track), 1, C.byref(ne))
    state = (_ptr(got.table, _lib.rf_track), _ptr(got.records, _lib.rf_track_follow), got.templates.ctypes.data)
    for fa in ((frame.ctypes.data, 96, 128, 128 * 3 - 1), (frame.ctypes.data, -1, 128, 400), (frame.ctypes.data, 96, -1, 400)):
        assert built_lib.rf_track_step_follow_key(C.byref(got.spec), *state, C.byref(got.frames), C.byref(got.next_id), *fa, *tail) == _lib.RF_ERR_INVALID_ARG
    for st in ((None, state[1], state[2]), (state[0], None, state[2]), (state[0], state[1], None)):
        assert built_lib.rf_track_step_follow_key(C.byref(got.spec), *st, C.byref(got.frames), C.byref(got.next_id), *frame_args(frame), *tail) == _lib.RF_ERR_INVALID_ARG
        assert built_lib.rf_track_step_follow(C.byref(got.spec), None, *st, C.byref(got.frames), *frame_args(frame), None, None, 0, C.byref(cnt),
                                              None, 0, C.byref(ne)) == _lib.RF_ERR_INVALID_ARG
    assert got.frames.value == 0 and not got.table["id"].any()
    # the pieces
    tpl, out4 = np.zeros((32, 32), np.uint8), (C.c_int32 * 4)()
    assert built_lib.rf_follow_template(None, 0, 0, 0, 1, 0, 0, tpl.ctypes.data) == _lib.RF_ERR_INVALID_ARG
    assert built_lib.rf_follow_template(*frame_args(frame), 0, 0, 0, tpl.ctypes.data) == _lib.RF_ERR_INVALID_ARG
    assert built_lib.rf_follow_template(*frame_args(frame), 386, 0, 0, tpl.ctypes.data) == _lib.RF_ERR_INVALID_ARG
    for R in (0, 17):
        assert built_lib.rf_follow_search(*frame_args(frame), tpl.ctypes.data, 1, 0, 0, R, out4) == _lib.RF_ERR_INVALID_ARG
    # the tracker calls refuse a NULL tracker / handle without a GPU
    assert built_lib.rf_tracker_enable_follow(None, None) == _lib.RF_ERR_INVALID_ARG
    assert built_lib.rf_tracker_read_follow(None, 0, None, None, 0) == _lib.RF_ERR_INVALID_ARG
    assert built_lib.rf_follow_last_launch_ms(None, None) == _lib.RF_ERR_INVALID_ARG


@pytest.mark.parametrize("rows,cols,seed,radius", [(96, 128, 11, 1), (96, 128, 12, 8), (200, 240, 13, 8), (200, 240, 14, 16)])
def test_key_and_follow_steps_match_the_reference(built_lib, rows, cols, seed, radius):
    """every box shape in one table: key step, three follow steps on frames that drift, a key step with some faces gone, follows again"""
    big = canvas(rows + 60, cols + 60, seed)
    got, ref = pair(built_lib, 16, radius=radius, max_mad=40, max_run=4, max_missed=2)
    rowsf = [face(0.9 - 0.01 * i, x, y, w, h) for i, (x, y, w, h) in enumerate(boxes_for(rows, cols))]
    rowsf.append(face(0.5, np.nan, 10, 20))                   # a face without a geometry opens a track and gets the zero record
    faces = by_score(rowsf)
    x0, y0 = 30, 30
    key_both(got, ref, window(big, rows, cols, x0, y0), faces)
    assert got.records["valid"].sum() == len(faces) - 1
    moved = 0
    for step in range(3):
        x0, y0 = x0 + 2, y0 - 1
        _, out, tags, _ = follow_both(got, ref, window(big, rows, cols, x0, y0))
        moved += len(out)
        assert all(g["flags"] & fr.FOLLOWED for g in tags) and list(tags["slot"]) == sorted(tags["slot"])
    assert moved > 0
    key_both(got, ref, window(big, rows, cols, x0, y0), faces[::2])
    for step in range(6):                                      # past max_run: the unkeyed tracks age and end
        x0, y0 = x0 - 3, y0 + 2
        follow_both(got, ref, window(big, rows, cols, x0, y0))
    follow_both(got, ref, None)                                # no pixels: every live track ages


def test_flat_frame_answers_did_not_move(built_lib):
    flat = strided(np.full((96, 128, 3), 77, np.uint8))
    got, ref = pair(built_lib, 4)
    key_both(got, ref, flat, by_score([face(0.9, 40, 30, 31), face(0.8, -10, 60, 30)]))
    _, out, tags, _ = follow_both(got, ref, flat)
    assert len(out) == 2
    assert [(int(r["sad"]), int(r["dx"]), int(r["dy"]), int(r["run"])) for r in got.records[:2]] == [(0, 0, 0, 1)] * 2
    assert out.tobytes() == got.table["last"][:2].tobytes()


def test_equal_minima_resolve_by_the_key(built_lib):
    """a pattern of period 4 pixels seen 2 pixels further: du = -2 and du = +2 both give SAD 0; the same motion, so raster order decides"""
    xx = np.arange(160)
    stripes = np.repeat((40 + 50 * (xx % 4))[None, :, None], 96, 0).repeat(3, 2).astype(np.uint8)
    key, nxt = strided(stripes[:, 10:138]), strided(stripes[:, 12:140])
    got, ref = pair(built_lib, 4)
    key_both(got, ref, key, by_score([face(0.9, 48, 30, 31)]))
    assert got.records[0]["q"] == 1
    st = fr.search(nxt, ref.templates[0], 1, int(ref.records[0]["ox"]), int(ref.records[0]["oy"]), 8)
    assert st[:2] == (2, 0) and st[2] == -2 and st[3] == 0
    follow_both(got, ref, nxt)
    assert (int(got.records[0]["dx"]), int(got.records[0]["dy"]), int(got.records[0]["sad"])) == (-2, 0, 0)
    # and on the key frame itself the smaller motion wins over du = +-4
    got, ref = pair(built_lib, 4)
    key_both(got, ref, key, by_score([face(0.9, 48, 30, 31)]))
    follow_both(got, ref, key)
    assert (int(got.records[0]["dx"]), int(got.records[0]["sad"])) == (0, 0)


def test_max_run_is_reached(built_lib):
    frame = strided(canvas(96, 128, 5))
    got, ref = pair(built_lib, 4, max_run=2, max_missed=5)
    key_both(got, ref, frame, by_score([face(0.9, 40, 30, 31)]))
    for want_run, want_missed, want_n in ((1, 0, 1), (2, 0, 1), (2, 1, 0), (2, 2, 0)):
        _, out, _, _ = follow_both(got, ref, frame)
        assert (int(got.records[0]["run"]), int(got.table[0]["missed"]), len(out)) == (want_run, want_missed, want_n)
    assert got.records[0]["sad"] == -1
    key_both(got, ref, frame, by_score([face(0.9, 41, 30, 31)]))                       # the next key step starts a new run
    assert (int(got.records[0]["run"]), int(got.table[0]["missed"])) == (0, 0)
    assert len(follow_both(got, ref, frame)[1]) == 1


def test_rejection_ages_ends_and_frees_the_slot(built_lib):
    a, b = strided(canvas(96, 128, 6)), strided(canvas(96, 128, 7))
    got, ref = pair(built_lib, 2, max_mad=1, max_missed=1)
    key_both(got, ref, a, by_score([face(0.9, 40, 30, 31), face(0.8, 80, 50, 25)]))
    _, out, _, ended = follow_both(got, ref, b)                                        # other pixels: rejected, the winner's SAD is kept
    assert len(out) == 0 and len(ended) == 0 and all(got.records["sad"] > 1024) and list(got.table["missed"]) == [1, 1]
    _, out, _, ended = follow_both(got, ref, b)
    assert len(ended) == 2 and list(ended["id"]) == [1, 2] and not got.table["id"].any() and got.records.tobytes() == bytes(64)
    _, tags = key_both(got, ref, a, by_score([face(0.9, 10, 10, 31)]))                 # the freed slot is taken by the next key step
    assert (int(tags[0]["slot"]), int(tags[0]["id"]), int(got.records[0]["valid"])) == (0, 3, 1)


def test_cut_lists_truncate(built_lib):
    frame, other = strided(canvas(96, 128, 8)), strided(canvas(96, 128, 9))
    faces = by_score([face(0.9, 10, 10, 31), face(0.8, 60, 10, 31), face(0.7, 10, 50, 31)])
    got, ref = pair(built_lib, 4, max_missed=-1, max_mad=1)
    key_both(got, ref, frame, faces)
    rc, out, tags, _ = follow_both(got, ref, frame, cap=2)                             # three accepted, room for two
    assert rc == _lib.RF_ERR_TRUNCATED and len(out) == 2 and list(tags["slot"]) == [0, 1]
    rc, out, _, ended = follow_both(got, ref, other, cap_ended=1)                      # three end, room for one
    assert rc == _lib.RF_ERR_TRUNCATED and len(ended) == 1 and not got.table["id"].any()


# ---------------------------------------------------------------------------------------------- the claim, on real pixels
PAN = (3, 4)                                                   # the window moves by this much a frame: the faces by its negative


def pan_windows(base_frame, n=8):
    return [np.ascontiguousarray(base_frame[48 + PAN[1] * t:496 + PAN[1] * t, 420 + PAN[0] * t:868 + PAN[0] * t]) for t in range(n)]


def test_followed_boxes_stay_on_the_faces_between_key_frames(built_lib, oracles, base_frame):
    """448 x 448 windows panning over the base frame, a key frame every fourth frame with the fp32 oracle's boxes, follow steps in
    between.  The pan was chosen with tests/follow_ref.py alone: both faces have q = 5, every followed centre is within 2 pixels per
    axis (the bound is q) of the key box moved by the true pan, at a mean absolute difference of 7.3 to 8.0.  (Pans of (7, 3), (6, 3)
    and (4, 2) land between cells so that one face reaches 18 > max_mad = 16 on a frame and is not followed there: the reference says
    so as well, it is the definition's sub-cell limit at the default max_mad, not the code's.)  The plain tracker's `last` stays where
    the key frame left it."""
    wins = pan_windows(base_frame)
    got, ref = pair(built_lib, 8)
    plain_last = None
    for t, w in enumerate(wins):
        if t % 4 == 0:
            truth = tr.faces_array(oracles[STEMS[0]].detect(w, 0.5, 0.4, net_hw=(448, 448)).rows())
            assert len(truth) == 2
            _, tags = key_both(got, ref, w, truth)
            key_centres = {int(g["slot"]): ((r[1] + r[3]) / 2, (r[2] + r[4]) / 2) for g, r in zip(tags, tr.rows_of(truth))}
            plain_last = got.table["last"].copy()
            continue
        _, out, tags, _ = follow_both(got, ref, w)
        assert len(out) == 2
        k = t % 4
        for g, r in zip(tags, tr.rows_of(out)):
            s = int(g["slot"])
            q = int(got.records[s]["q"])
            cx, cy = (r[1] + r[3]) / 2, (r[2] + r[4]) / 2
            wx, wy = key_centres[s][0] - PAN[0] * k, key_centres[s][1] - PAN[1] * k
            print("frame", t, "slot", s, "q", q, "off", cx - wx, cy - wy, "sad/1024", got.records[s]["sad"] / 1024)
            assert abs(cx - wx) <= q and abs(cy - wy) <= q, (t, s, q, cx - wx, cy - wy)
            px = (plain_last[s]["x1"] + plain_last[s]["x2"]) / 2                       # what a tracker without follow still holds
            assert abs(px - wx) == pytest.approx(PAN[0] * k, abs=1e-3)


# ---------------------------------------------------------------------------------------------- the sanitizer program
def test_host_steps_under_address_and_ub_sanitizers(tmp_path):
    """tests/csrc/test_follow_host.cpp: a few hundred random key and follow steps into exactly-sized heap buffers, host code only, built
    with -fsanitize=address,undefined.  No GPU and no library: follow.h is compiled into the program."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    clang = os.path.join(rocm, "llvm", "bin", "clang++")                   # the compiler the library is built with
    clang = clang if os.path.exists(clang) else shutil.which("clang++")
    assert clang, "no clang++ next to hipcc"
    exe = str(tmp_path / "test_follow_host")
    subprocess.check_call([clang, "-O1", "-g", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "csrc", "test_follow_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])
