"""The best-shot gallery on the host: rf_shot_resolve (retinaface_amd/csrc/shot.h, the decisions the two shot kernels make) against
tests/shot_ref.py.  The frame-by-frame definition (shot_ref.Gallery) says which face's crop a delivered shot is; rf_shot_resolve decides
the same per LAUNCH of one to five images from tags, ended lists and stored records alone, and the two must name the same faces."""
import ctypes as C

import numpy as np
import pytest

import align_ref
import shot_ref
import track_ref as tr
from retinaface_amd import _lib, shot_resolve
from test_track_host import by_score, face, sequence

CROP = 16
CAP = 48            # faces per image in these tests


class TokenGallery(shot_ref.Gallery):
    """shot_ref.Gallery whose "crop" of a face is a token naming it (frame index + the face's own 60 bytes): no pixels needed"""

    def __init__(self, spec):
        super().__init__(spec, 1, size=CROP)

    def face_bytes(self, frame, row, cs=1.0):
        return token(frame, row), align_ref.align_matrix(row, cs, CROP)[1]


def token(frame_index, row):
    out = np.zeros(3 * CROP * CROP, np.uint8)
    out[:8] = np.frombuffer(np.int64(frame_index).tobytes(), np.uint8)
    out[8:68] = np.frombuffer(np.asarray(row, np.float32).tobytes(), np.uint8)
    return out


def run_launches(launches, spec, cap_ended=8, quality=None):
    """launches: lists of per-image face arrays (FACE records in score order).  Drives the frame-by-frame reference and rf_shot_resolve
    side by side and checks every delivered shot, every slot and every record.  Returns what happened, for the property tests."""
    ref = TokenGallery(spec)
    T = spec.max_tracks
    stored = np.zeros((T, 3 * CROP * CROP), np.uint8)               # the gallery as the owners rf_shot_resolve names fill it
    records = np.zeros(T, shot_ref.SHOT)
    log = dict(kinds=[], delivered=0, owners=[], truncated=False, shots=[])
    g = 0
    for imgs in launches:
        n = len(imgs)
        first = ref.streams[0].frames
        tags = np.zeros((n, CAP), tr.TAG)
        ended = np.zeros((n, cap_ended), tr.TRACK)
        counts, ecounts = np.zeros(n, np.int32), np.zeros(n, np.int32)
        faces = np.zeros((n, CAP, 15), np.float32)
        want_shots, want_info = [], []
        for i, f in enumerate(imgs):
            rows = tr.rows_of(f)
            q = quality[g] if quality is not None else None
            t, e, over, sh, info = ref.step(0, first + i, rows, 1.0, q, cap_ended)
            counts[i], ecounts[i] = len(rows), len(e)
            tags[i, :len(t)], faces[i, :len(rows)] = t, rows
            ended[i, :len(sh)] = e[:cap_ended]
            want_shots.append(sh); want_info.append(info)
            log["truncated"] |= len(e) > cap_ended
            g += 1
        mats = np.zeros((n, CAP, 6))
        for i in range(n):
            for k in range(counts[i]):
                mats[i, k] = align_ref.align_matrix(faces[i, k], 1.0, CROP)[1]
        delivered, source, owner, after = shot_resolve(T, tags, counts, ended, ecounts, first, records, faces, None, CROP)
        r_del, r_source, r_owner, r_after = shot_ref.resolve(T, tags, counts, ended, ecounts, first, records, mats)
        assert delivered == r_del == sum(len(s) for s in want_shots)
        assert source.tobytes() == r_source.tobytes() and owner.tobytes() == r_owner.tobytes()
        assert after.tobytes() == r_after.tobytes()
        for i in range(n):                                          # every delivered shot is the face the definition names
            for e in range(len(want_shots[i])):
                kind, a, b = source[i, e]
                got = np.zeros_like(stored[0]) if kind == shot_ref.NONE else stored[a] if kind == shot_ref.STORED else token(first + a, faces[a, b])
                got_info = np.zeros((), shot_ref.SHOT)
                if kind == shot_ref.STORED:
                    got_info = records[a]
                elif kind == shot_ref.LAUNCH:
                    got_info = np.array((ended[i, e]["id"], first + a, mats[a, b]), shot_ref.SHOT)
                assert got.tobytes() == want_shots[i][e].tobytes(), (i, e, kind)
                assert got_info.tobytes() == want_info[i][e].tobytes()
                assert (kind == shot_ref.NONE) == (ended[i, e]["best_frame"] < 0)
                log["kinds"].append(int(kind))
                log["shots"].append((int(ended[i, e]["id"]), int(ended[i, e]["best_frame"])))
            assert (source[i, len(want_shots[i]):] == -1).all()
        for s in range(T):                                          # the keep launch: the owners write their slots
            if owner[s, 0] >= 0:
                stored[s] = token(first + owner[s, 0], faces[owner[s, 0], owner[s, 1]])
        records = after
        log["delivered"] += delivered
        log["owners"].append(owner.copy())
        want_ent, want_rec = ref.read(0)
        valid = want_rec["id"] != 0
        assert stored[valid].tobytes() == want_ent[valid].tobytes()
        assert records[valid].tobytes() == want_rec[valid].tobytes()
        tb = ref.streams[0].table                                   # a slot the launch leaves alone has no owner
        inside = (tb["id"] != 0) & (tb["best_frame"] >= first)
        assert ((owner[:, 0] >= 0) == inside).all() or log["truncated"]
    return log


def test_struct_size():
    assert C.sizeof(_lib.rf_shot) == 64 == shot_ref.SHOT.itemsize


@pytest.mark.parametrize("seed,max_tracks,max_missed,n_people", [(1, 64, -1, 10), (2, 8, 1, 12), (3, 256, 0, 30), (4, 5, -1, 9), (5, 16, 1, 14),
                                                                 (6, 32, 0, 12)])
def test_sequences_match_the_definition(built_lib, seed, max_tracks, max_missed, n_people):
    spec = tr.Spec(max_tracks, 0.0, max_missed, 1, 0.0)            # max_missed 0 = the default, 10; -1 = 0
    frames = sequence(seed, 60, n_people, spec.max_missed)
    rng = np.random.default_rng(seed)
    launches, at = [], 0
    while at < len(frames):
        k = int(rng.integers(1, 6))
        launches.append(frames[at:at + k]); at += k
    log = run_launches(launches, spec)
    assert log["delivered"] > 3
    assert shot_ref.STORED in log["kinds"]
    assert spec.max_missed != 0 or shot_ref.LAUNCH in log["kinds"]      # a shot taken and delivered inside one launch needs a short life


def test_gated_sequences(built_lib):
    spec = tr.Spec(16, 0.0, 1, 1, 0.0)
    frames = sequence(11, 50, 12, 1)
    rng = np.random.default_rng(11)
    quality = []
    for f in frames:
        q = np.zeros(len(f), tr.QUALITY)
        q["flags"] = rng.integers(0, 3, len(f)) == 0
        q["sharpness"] = rng.integers(1, 9, len(f))
        quality.append(q)
    log = run_launches([frames[i:i + 3] for i in range(0, 50, 3)], spec, quality=quality)
    assert shot_ref.NONE in log["kinds"] and shot_ref.STORED in log["kinds"]


def one(score, x=100.0):
    return by_score([face(score, x, 100, 40)])


NOBODY = np.zeros(0, tr.FACE)


def test_best_shot_improves_then_does_not(built_lib):
    spec = tr.Spec(4, 0.0, -1, 1, 0.0)
    log = run_launches([[one(0.5), one(0.75), one(0.625), NOBODY]], spec)
    assert log["shots"] == [(1, 1)] and log["kinds"] == [shot_ref.LAUNCH]
    log = run_launches([[one(0.5)], [one(0.75)], [one(0.625)], [NOBODY]], spec)
    assert log["shots"] == [(1, 1)] and log["kinds"] == [shot_ref.STORED]
    assert [int(o[0, 0]) for o in log["owners"]] == [0, 0, -1, -1]          # frame 2 does not touch the slot


def test_opens_shoots_and_ends_inside_one_launch(built_lib):
    log = run_launches([[NOBODY, one(0.5), NOBODY, NOBODY]], tr.Spec(4, 0.0, -1, 1, 0.0))
    assert log["shots"] == [(1, 1)] and log["kinds"] == [shot_ref.LAUNCH]
    assert (log["owners"][0] == -1).all()


def test_ends_with_a_shot_from_before_the_launch(built_lib):
    log = run_launches([[one(0.5), one(0.25)], [one(0.25), NOBODY, NOBODY]], tr.Spec(4, 0.0, 1, 1, 0.0))
    assert log["shots"] == [(1, 0)] and log["kinds"] == [shot_ref.STORED]


def test_same_frame_slot_reuse(built_lib):
    # max_tracks 1: the track of frame 0 ends in frame 1, whose face (far away) opens a track in the same slot in the same frame
    log = run_launches([[one(0.5, 100.0)], [one(0.75, 400.0), one(0.5, 700.0)], [NOBODY]], tr.Spec(1, 0.0, -1, 1, 0.0))
    assert log["shots"] == [(1, 0), (2, 1), (3, 2)]
    assert log["kinds"] == [shot_ref.STORED, shot_ref.LAUNCH, shot_ref.STORED]
    assert [tuple(o[0]) for o in log["owners"]] == [(0, 0), (1, 0), (-1, -1)]


def test_gated_tracks_end_without_a_shot(built_lib):
    q = np.zeros(1, tr.QUALITY)
    q["flags"] = 1
    log = run_launches([[one(0.5), NOBODY]], tr.Spec(4, 0.0, -1, 1, 0.0), quality=[q, q[:0]])
    assert log["shots"] == [(1, -1)] and log["kinds"] == [shot_ref.NONE]


def test_cut_ended_list(built_lib):
    three = by_score([face(0.5, 100, 100, 40), face(0.25, 300, 100, 40), face(0.125, 500, 100, 40)])
    log = run_launches([[three], [NOBODY], [one(0.5)], [NOBODY]], tr.Spec(4, 0.0, -1, 1, 0.0), cap_ended=1)
    assert log["truncated"] and log["shots"] == [(1, 0), (4, 2)]


def test_refusals(built_lib):
    rec = np.zeros(4, shot_ref.SHOT)
    p = rec.ctypes.data_as(C.POINTER(_lib.rf_shot))
    lib = built_lib
    assert lib.rf_shot_resolve(0, 0, None, 1, None, None, 0, None, 0, None, None, CROP, p, None, None) == _lib.RF_ERR_INVALID_ARG
    assert lib.rf_shot_resolve(257, 0, None, 1, None, None, 0, None, 0, None, None, CROP, p, None, None) == _lib.RF_ERR_INVALID_ARG
    assert lib.rf_shot_resolve(4, 1, None, 1, None, None, 0, None, 0, None, None, CROP, p, None, None) == _lib.RF_ERR_INVALID_ARG
    assert lib.rf_shot_resolve(4, 0, None, 1, None, None, 0, None, -1, None, None, CROP, p, None, None) == _lib.RF_ERR_INVALID_ARG
    assert lib.rf_shot_resolve(4, 0, None, 1, None, None, 0, None, 0, None, None, CROP, None, None, None) == _lib.RF_ERR_INVALID_ARG
    assert lib.rf_shot_resolve(4, 0, None, 1, None, None, 0, None, 0, None, None, CROP, p, None, None) == 0
    assert lib.rf_tracker_enable_shots(None, None) == _lib.RF_ERR_INVALID_ARG
