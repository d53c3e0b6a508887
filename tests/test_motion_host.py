"""Motion-predicted tracks on the host: rf_track_step_motion and rf_track_predict (retinaface_amd/csrc/motion.h, the code the kernels
run) against tests/motion_ref.py, byte for byte; the negative-horizon equivalence with rf_track_step; the refusals; the vertical pan
with three dropped frames through the CPU oracle; and the stand-alone sanitizer program."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import motion_ref as mr
import track_ref as tr
from conftest import ROOT, STEMS
from retinaface_amd import _lib
from test_track_host import SCORES, HostStream, _ptr, _spec, by_score, face, sequence

f32 = np.float32
EMPTY = np.zeros(0, tr.FACE)


def _mspec(**kw):
    s = _lib.rf_motion_spec()
    s.struct_size = C.sizeof(_lib.rf_motion_spec)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


class MotionStream(HostStream):
    """a caller-held table and its motion records driven through rf_track_step_motion"""

    def __init__(self, lib, max_tracks=64, alpha=0.0, horizon=0, **kw):
        super().__init__(lib, max_tracks, **kw)
        self.mspec = _mspec(alpha=alpha, horizon=horizon)
        self.motion = np.zeros(len(self.table), mr.MOTION)

    def step(self, faces, scale=1.0, quality=None, max_faces=256, cap_ended=8):
        faces = np.ascontiguousarray(faces)
        count = len(faces)
        tags = np.zeros(max(count, 1), tr.TAG)
        ended = np.zeros(max(cap_ended, 1), tr.TRACK)
        ne = C.c_int(-1)
        rc = self.lib.rf_track_step_motion(C.byref(self.spec), C.byref(self.mspec), _ptr(self.table, _lib.rf_track),
                                           _ptr(self.motion, _lib.rf_track_motion), C.byref(self.frames), C.byref(self.next_id),
                                           _ptr(faces, _lib.rf_face), count, scale,
                                           _ptr(quality, _lib.rf_face_quality) if quality is not None else None, max_faces,
                                           _ptr(tags, _lib.rf_track_tag), _ptr(ended, _lib.rf_track), cap_ended, C.byref(ne))
        return rc, tags[:count], ended[:min(max(ne.value, 0), cap_ended)], ne.value


def crowd(rng, m, t, jitter=3.0):
    """test_track_gpu.py's crowd: m faces on a 16 x 16 grid of 40-pixel cells that drifts 2 pixels per frame"""
    ids = np.sort(rng.permutation(256)[:m])
    rows = [face(SCORES[rng.integers(0, 31)], 40.0 * (j % 16) + 2.0 * t + rng.uniform(0, jitter), 40.0 * (j // 16) + rng.uniform(0, jitter), 30.0)
            for j in ids]
    return by_score(rows) if rows else EMPTY


def gapped_crowd(seed, max_tracks, n_frames=16):
    """crowd frames with frames of 0 faces in between, so that missed reaches 1, 2 and 3 before the faces come back"""
    rng = np.random.default_rng(seed)
    sizes = (1, 64, 65, 256, 40, 200)
    gaps = {2: 1, 5: 2, 9: 3}                       # after frame t: that many empty frames
    frames = []
    for t in range(n_frames):
        frames.append(crowd(rng, min(sizes[t % len(sizes)], 2 * max_tracks + 1), len(frames)))
        frames += [EMPTY] * gaps.get(t, 0)
    return frames


def pair(lib, max_tracks, alpha, horizon, **kw):
    spec = tr.Spec(max_tracks, kw.get("min_iou", 0.0), kw.get("max_missed", 0), kw.get("min_hits", 0), kw.get("new_score", 0.0))
    return MotionStream(lib, max_tracks, alpha, horizon, **kw), mr.Stream(spec, mr.Spec(alpha, horizon))


def check_step(got, ref, faces, scale=1.0, cap_ended=4):
    tags, ended, over = mr.step(ref, faces, scale)
    rc, gtags, gended, ne = got.step(faces, scale=scale, cap_ended=cap_ended)
    assert gtags.tobytes() == tags.tobytes()
    assert ne == len(ended) and gended.tobytes() == ended[:cap_ended].tobytes()
    assert rc == (_lib.RF_ERR_TRUNCATED if over or len(ended) > cap_ended else 0)
    assert got.table.tobytes() == ref.table.tobytes()
    assert got.motion.tobytes() == ref.motion.tobytes()
    assert (got.frames.value, got.next_id.value) == (ref.frames, ref.next_id)
    return tags, ended


def test_struct_sizes():
    assert C.sizeof(_lib.rf_motion_spec) == 16
    assert C.sizeof(_lib.rf_track_motion) == 16 == mr.MOTION.itemsize
    assert C.sizeof(_lib.rf_track) == 176 and C.sizeof(_lib.rf_track_tag) == 24


@pytest.mark.parametrize("max_tracks,alpha,horizon,scale", [
    (1, 1.0, 8, 1.0), (64, 0.5, 8, 1.0), (65, 0.3, 1, float(f32(1280) / f32(448))), (256, 0.5, -1, 1.0), (64, 0.0, 0, 2.5), (65, 1.0, 2, 1.0),
    (256, 0.3, 8, 0.75)])
def test_gapped_crowd_matches_the_reference(built_lib, max_tracks, alpha, horizon, scale):
    got, ref = pair(built_lib, max_tracks, alpha, horizon, max_missed=3, min_hits=2)
    rematched = moving = 0
    for faces in gapped_crowd(max_tracks, max_tracks):
        missed_before = ref.table["missed"].copy()
        tags, _ = check_step(got, ref, faces, scale)
        slots = tags["slot"][(tags["id"] != 0) & ((tags["flags"] & tr.NEW) == 0)]
        rematched += int((missed_before[slots] > 0).sum())
        moving += int((ref.motion["samples"] > 1).sum())
    if max_tracks > 1:                                          # (one slot seldom meets its face again in a random crowd)
        assert rematched > 0 and moving > 0                     # tracks were re-matched after a gap, velocities were smoothed


@pytest.mark.parametrize("seed,max_tracks,max_missed,alpha,horizon,n_people", [
    (1, 64, 2, 0.5, 8, 12), (2, 8, 1, 1.0, 1, 14), (3, 256, 4, 0.3, 8, 40), (4, 5, -1, 0.5, 3, 9), (5, 0, 0, 0.0, 0, 20)])
def test_walkers_match_the_reference(built_lib, seed, max_tracks, max_missed, alpha, horizon, n_people):
    """test_track_host.py's walkers: they move up to 14 pixels a frame, vanish for a few frames, cross each other; tracks end, slots are
    reused (max_missed -1: a track that ends and one that opens in the same slot in the same frame), tables overflow"""
    got, ref = pair(built_lib, max_tracks, alpha, horizon, max_missed=max_missed)
    any_end = reopened = False
    for faces in sequence(seed, 40, n_people, ref.spec.max_missed):
        tags, ended = check_step(got, ref, faces)
        any_end = any_end or len(ended) > 0
        new_slots = set(tags["slot"][(tags["flags"] & tr.NEW) != 0].tolist())
        if len(ended) and new_slots:
            reopened = True
            for s in new_slots:
                assert got.motion[s].tobytes() == bytes(16)
    assert any_end and reopened


def test_a_slot_that_ends_and_reopens_in_one_frame_gets_the_zero_record(built_lib):
    got, ref = pair(built_lib, 1, 0.5, 8, max_missed=-1)
    for t in range(3):
        check_step(got, ref, by_score([face(0.9, 10 + 6 * t, 10, 30)]))
    assert got.motion[0]["samples"] == 2 and got.motion[0]["vx"] == 6
    tags, ended = check_step(got, ref, by_score([face(0.9, 400, 400, 30)]))
    assert len(ended) == 1 and ended[0]["id"] == 1 and tags[0]["id"] == 2 and tags[0]["slot"] == 0
    assert got.motion[0].tobytes() == bytes(16)


def test_prediction_keeps_a_fast_face_that_the_plain_rule_loses(built_lib):
    got, ref = pair(built_lib, 4, 0.5, 8)
    plain = HostStream(built_lib, 4)
    frames = [by_score([face(0.9, 10 + 20 * t, 10, 40)]) if t not in (3, 4, 5) else EMPTY for t in range(9)]
    for faces in frames:
        check_step(got, ref, faces)
        plain.step(faces)
    assert got.next_id.value == 2 and plain.next_id.value == 3
    assert got.table[0]["hits"] == 6 and got.motion[0]["vx"] == 20


def test_horizon_caps_the_extrapolation(built_lib):
    got, ref = pair(built_lib, 4, 1.0, 2, max_missed=8)
    for t in range(3):
        check_step(got, ref, by_score([face(0.9, 10 + 20 * t, 10, 40)]))
    for _ in range(5):
        check_step(got, ref, EMPTY)
    # missed 5, horizon 2: the box is expected 2 frames ahead of x = 50, not 6
    tags, _ = check_step(got, ref, by_score([face(0.9, 50 + 20 * 6, 10, 40), face(0.8, 50 + 20 * 2, 10, 40)]))
    assert [int(g["id"]) for g in tags] == [2, 1]
    r = f32(40) / f32(6)                                         # the newest sample: 40 pixels over 6 frames
    assert got.motion[0]["vx"] == f32(20) + f32(1) * (r - f32(20))   # alpha 1 is still a subtract, a multiply and an add


def test_nonfinite_faces_zero_the_record_and_the_next_step_runs(built_lib):
    # huge finite boxes that overlap: x1 + x2 overflows to inf, so the velocity sample is not finite
    big = lambda x1, x2: np.array([0.9, x1, 0, x2, 0] + [0] * 10, np.float32)
    got, ref = pair(built_lib, 4, 0.5, 8)
    check_step(got, ref, by_score([big(1.0e38, 1.5e38)]))
    check_step(got, ref, by_score([big(1.05e38, 1.55e38)]))
    assert got.motion[0]["samples"] == 1 and got.motion[0]["vx"] > 1e36
    tags, _ = check_step(got, ref, by_score([big(1.2e38, 2.4e38)]))
    assert tags[0]["id"] == 1 and got.motion[0].tobytes() == bytes(16)
    tags, _ = check_step(got, ref, by_score([big(1.2e38, 2.4e38)]))
    assert tags[0]["id"] == 1 and got.motion[0].tobytes() == bytes(16) and got.table[0]["hits"] == 4
    # NaN and inf in a box: such a face matches nothing and opens a track; the tracks beside it go on
    got, ref = pair(built_lib, 8, 0.5, 8)
    nan = face(0.9, 10, 10, 30) * np.array([1] + [np.nan] * 14, np.float32)
    inf = face(0.85, 300, 10, 30)
    inf[3] = np.inf
    for rows in ([face(0.8, 100, 10, 30)], [face(0.8, 104, 10, 30)], [nan, inf, face(0.8, 108, 10, 30)], [face(0.8, 112, 10, 30), inf],
                 [face(0.8, 116, 10, 30)]):
        check_step(got, ref, by_score(rows))
    assert got.table[0]["hits"] == 5 and got.motion[0]["vx"] == 4 and got.next_id.value == 5
    # an inf coordinate scale maps every box to inf
    check_step(got, ref, by_score([face(0.8, 120, 10, 30)]), scale=float("inf"))
    check_step(got, ref, by_score([face(0.8, 120, 10, 30)]))


@pytest.mark.parametrize("seed,max_tracks,max_missed,alpha", [(1, 64, 2, 0.5), (2, 8, 1, 1.0), (4, 5, -1, 0.3), (3, 256, 4, 0.0)])
def test_negative_horizon_is_the_plain_tracker(built_lib, seed, max_tracks, max_missed, alpha):
    got = MotionStream(built_lib, max_tracks, alpha, -1, max_missed=max_missed)
    plain = HostStream(built_lib, max_tracks, max_missed=max_missed)
    smoothed = 0
    for faces in sequence(seed, 40, 14, max(max_missed, 0)) + gapped_crowd(seed, max_tracks, 6):
        a, b = got.step(faces, cap_ended=4), plain.step(faces, cap_ended=4)
        assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and a[3] == b[3]
        assert got.table.tobytes() == plain.table.tobytes()
        assert (got.frames.value, got.next_id.value) == (plain.frames.value, plain.next_id.value)
        smoothed = max(smoothed, int(got.motion["samples"].max()))
    assert smoothed > 1                                          # only the records differ


@pytest.mark.parametrize("alpha,horizon", [(0.0, 0), (1.0, 1), (0.3, 65536)])
def test_steady_faces_get_the_plain_trackers_tags(built_lib, alpha, horizon):
    """nobody is ever missed and every face overlaps only its own track's last and predicted box: any spec gives the plain tags"""
    got = MotionStream(built_lib, 64, alpha, horizon)
    plain = HostStream(built_lib, 64)
    rng = np.random.default_rng(11)
    cells = np.sort(rng.permutation(256)[:48])
    for t in range(12):
        rows = [face(SCORES[rng.integers(0, 31)], 40.0 * (j % 16) + 2.0 * t + rng.uniform(0, 3), 40.0 * (j // 16) + rng.uniform(0, 3), 30.0)
                for j in cells]
        a, b = got.step(by_score(rows)), plain.step(by_score(rows))
        assert a[1].tobytes() == b[1].tobytes() and got.table.tobytes() == plain.table.tobytes()
    assert got.table["hits"][:48].tolist() == [12] * 48 and got.motion["samples"][:48].tolist() == [11] * 48


def predict(lib, mspec, track, rec, ahead):
    t = _lib.rf_track.from_buffer_copy(np.asarray(track, tr.TRACK).tobytes())
    m = _lib.rf_track_motion.from_buffer_copy(np.asarray(rec, mr.MOTION).tobytes())
    out = _lib.rf_face()
    rc = lib.rf_track_predict(C.byref(mspec) if mspec is not None else None, C.byref(t), C.byref(m), ahead, C.byref(out))
    return rc, bytes(out)


def test_predict_equals_the_reference(built_lib):
    import retinaface_amd as rfa
    got, ref = pair(built_lib, 4, 0.5, 3, max_missed=9)
    rows = face(0.9, 10.3, 20.7, 33.1)
    rows[5] = -0.0                                               # a landmark at -0.0
    check_step(got, ref, by_score([rows]))
    for missed in range(0, 6):
        for ahead in (0, 1):
            for horizon in (3, -1, 0, 1):
                want = mr.predict(ref.table[0], ref.motion[0], ahead, mr.Spec(0.5, horizon))
                rc, out = predict(built_lib, _mspec(alpha=0.5, horizon=horizon), got.table[0], got.motion[0], ahead)
                assert rc == 0 and out == want.tobytes(), (missed, ahead, horizon)
                if ref.motion[0]["samples"] == 0 or horizon < 0 or missed + ahead == 0:
                    assert out == got.table[0]["last"].tobytes()          # nothing is added: the same bytes, -0.0 included
        if missed == 0:                                          # the second match gives the track a velocity; then it coasts
            assert np.signbit(np.frombuffer(predict(built_lib, None, got.table[0], got.motion[0], 1)[1], f32)[5])
            check_step(got, ref, by_score([face(0.9, 13.9, 18.2, 33.1)]))
            assert got.motion[0]["samples"] == 1 and got.table[0]["missed"] == 0
        else:
            check_step(got, ref, EMPTY)
        if missed < 5:
            assert got.table[0]["missed"] == missed
    # h is capped by the horizon: 5 missed frames and 3 predict the same face, and the Python wrapper returns those bytes
    want = mr.predict_row(np.frombuffer(got.table[0]["last"].tobytes(), f32), got.motion[0], 3)
    assert predict(built_lib, _mspec(alpha=0.5, horizon=3), got.table[0], got.motion[0], 1)[1] == want.tobytes()
    assert rfa.track_predict(got.table[0], got.motion[0], 1, dict(alpha=0.5, horizon=3)).tobytes() == want.tobytes()
    assert want[1] != got.table[0]["last"]["x1"]


def test_python_track_step_with_motion(built_lib):
    import retinaface_amd as rfa
    table, motion = np.zeros(8, rfa.TRACK_DTYPE), np.zeros(8, rfa.MOTION_DTYPE)
    ref = mr.Stream(tr.Spec(8), mr.Spec(0.3, 2))
    frames, next_id = 0, 1
    for t in range(5):
        faces = by_score([face(0.9, 10 + 9 * t, 10, 30)]) if t != 2 else EMPTY
        tags, ended, frames, next_id, cut = rfa.track_step(table, frames, next_id, tr.rows_of(faces), motion=motion, mspec=dict(alpha=0.3, horizon=2),
                                                           max_tracks=8)
        want, _, _ = mr.step(ref, faces)
        assert tags.tobytes() == want.tobytes() and table.tobytes() == ref.table.tobytes() and motion.tobytes() == ref.motion.tobytes()
    assert next_id == 2


def test_refusals(built_lib):
    faces = by_score([face(0.9, 10, 10, 30)])
    before = MotionStream(built_lib, 4)
    for bad in (dict(struct_size=12), dict(reserved=1), dict(alpha=float("nan")), dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float("inf")),
                dict(horizon=65537)):
        s = MotionStream(built_lib, 4)
        for k, v in bad.items():
            setattr(s.mspec, k, v)
        assert s.step(faces)[0] == _lib.RF_ERR_INVALID_ARG, bad
        assert s.table.tobytes() == before.table.tobytes() and s.motion.tobytes() == bytes(64) and (s.frames.value, s.next_id.value) == (0, 1)
        live = np.zeros((), tr.TRACK)
        live["id"] = 1
        assert predict(built_lib, s.mspec, live, np.zeros((), mr.MOTION), 1)[0] == _lib.RF_ERR_INVALID_ARG, bad
    s = MotionStream(built_lib, 4)
    s.spec = _spec(max_tracks=257)
    assert s.step(faces)[0] == _lib.RF_ERR_INVALID_ARG
    for ok in (dict(horizon=65536), dict(horizon=-5), dict(alpha=1.0)):
        s = MotionStream(built_lib, 4, **ok)
        assert s.step(faces)[0] == 0 and s.table[0]["id"] == 1
    # a NULL motion spec is all defaults; a NULL record array is refused
    s = MotionStream(built_lib, 4)
    tags, ended, ne = np.zeros(1, tr.TAG), np.zeros(1, tr.TRACK), C.c_int(0)
    args = (_ptr(faces, _lib.rf_face), 1, 1.0, None, 256, _ptr(tags, _lib.rf_track_tag), _ptr(ended, _lib.rf_track), 1, C.byref(ne))
    assert built_lib.rf_track_step_motion(C.byref(s.spec), None, _ptr(s.table, _lib.rf_track), None, C.byref(s.frames), C.byref(s.next_id),
                                          *args) == _lib.RF_ERR_INVALID_ARG and s.frames.value == 0
    assert built_lib.rf_track_step_motion(C.byref(s.spec), None, _ptr(s.table, _lib.rf_track), _ptr(s.motion, _lib.rf_track_motion),
                                          C.byref(s.frames), C.byref(s.next_id), *args) == 0 and s.table[0]["id"] == 1
    # rf_track_predict: a free slot, another `ahead`
    assert predict(built_lib, None, np.zeros((), tr.TRACK), np.zeros((), mr.MOTION), 1)[0] == _lib.RF_ERR_INVALID_ARG
    for ahead in (-1, 2):
        assert predict(built_lib, None, s.table[0], s.motion[0], ahead)[0] == _lib.RF_ERR_INVALID_ARG
    assert predict(built_lib, None, s.table[0], s.motion[0], 0)[0] == 0
    # the tracker calls refuse a NULL tracker without a GPU
    assert built_lib.rf_tracker_enable_motion(None, None) == _lib.RF_ERR_INVALID_ARG
    assert built_lib.rf_tracker_read_motion(None, 0, None, 0) == _lib.RF_ERR_INVALID_ARG


# ---------------------------------------------------------------------------------------------- the pan, through the CPU oracle
DROPPED = (3, 4, 5)


def pan_windows(base_frame):
    """a vertical pan of 24 pixels a frame over the two large faces of the base frame, which stay inside every window"""
    return [np.ascontiguousarray(base_frame[48 + 24 * t:496 + 24 * t, 420:868]) for t in range(9)]


@pytest.mark.parametrize("stem", STEMS)
def test_pan_with_dropped_frames_keeps_ids_and_coverage(built_lib, oracles, base_frame, stem):
    import retinaface_amd as rfa
    wins = pan_windows(base_frame)
    truth = [tr.faces_array(oracles[stem].detect(w, 0.5, 0.4, net_hw=(448, 448)).rows()) for w in wins]
    assert [len(f) for f in truth] == [2] * 9
    got = MotionStream(built_lib, 64)
    plain = HostStream(built_lib, 64)
    ids, plain_ids = set(), set()
    uncovered_plain = {}
    for t in range(9):
        faces = EMPTY if t in DROPPED else truth[t]
        _, tags, _, _ = got.step(faces)
        _, ptags, _, _ = plain.step(faces)
        ids |= {int(g["id"]) for g in tags}
        plain_ids |= {int(g["id"]) for g in ptags}
        if t not in DROPPED:
            continue
        live = [s for s in range(64) if got.table[s]["id"] != 0 and got.table[s]["missed"] >= 1]
        assert len(live) == 2 and all(got.table[s]["missed"] == t - 2 for s in live)
        coast = [np.frombuffer(predict(built_lib, None, got.table[s], got.motion[s], 0)[1], f32) for s in live]
        regions = [rfa.redact_region(f, 448, 448)[1] for f in coast]
        last = [rfa.redact_region(np.frombuffer(plain.table[s]["last"].tobytes(), f32), 448, 448)[1] for s in range(64) if plain.table[s]["id"] != 0]
        assert len(last) == 2
        uncovered_plain[t] = 0
        for face_t in tr.rows_of(truth[t]):
            hit, total = mr.coverage(face_t[1:5], regions, 448, 448)
            assert total > 90 * 120 and hit == total, (t, hit, total)              # every pixel of the true box is covered
            hit, total = mr.coverage(face_t[1:5], last, 448, 448)
            uncovered_plain[t] += total - hit
    assert ids == {1, 2} and len(plain_ids) == 4
    assert uncovered_plain[5] > 0                                                  # where the faces were last seen no longer covers them


# ---------------------------------------------------------------------------------------------- the sanitizer program
def test_host_step_under_address_and_ub_sanitizers(tmp_path):
    """tests/csrc/test_motion_host.cpp: a few hundred random frames through track_step_motion and the predicted faces, host code only,
    built with -fsanitize=address,undefined.  No GPU and no library: track.h and motion.h are compiled into the program."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    clang = os.path.join(rocm, "llvm", "bin", "clang++")                   # the compiler the library is built with
    clang = clang if os.path.exists(clang) else shutil.which("clang++")
    assert clang, "no clang++ next to hipcc"
    exe = str(tmp_path / "test_motion_host")
    subprocess.check_call([clang, "-O1", "-g", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "csrc", "test_motion_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])
