"""Face tracks on the GPU: the track kernel against tests/track_ref.py byte for byte on constructed faces (no forward pass) -- tags,
ended lists, counts and the table read back -- then the fused calls against their own parts (rf_detect_batch_device + the reference
fed with its result), the pan sequence, the fused face batch, the refusals and the C++ class."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import track_ref as tr
from conftest import ASSETS, ROOT
from test_face_aa_gpu import same, same_records
from test_gpu_align import FP16, engine, rfa, rows_of, to_device  # noqa: F401  (rfa: fixture)
from test_tile_gpu import INT8, SPLIT2, SPLIT3, split_engine
from test_track_host import SCORES, by_score, face

pytestmark = pytest.mark.gpu
f32 = np.float32
MD = 256


# ---------------------------------------------------------------------------------------------- 1. constructed faces
def crowd(rng, m, t, jitter=3.0):
    """m faces on a 16 x 16 grid of 40-pixel cells that drifts 2 pixels per frame: face j of frame t overlaps face j of frame t - 1 by
    well over 0.3 and no other.  Scores come from 31 values."""
    ids = np.sort(rng.permutation(256)[:m])
    rows = [face(SCORES[rng.integers(0, 31)], 40.0 * (j % 16) + 2.0 * t + rng.uniform(0, jitter), 40.0 * (j // 16) + rng.uniform(0, jitter), 30.0)
            for j in ids]
    return by_score(rows) if rows else np.zeros(0, tr.FACE)


def pack(per_image, cap):
    faces = np.zeros((len(per_image), cap), tr.FACE)
    counts = np.zeros(len(per_image), np.int32)
    for i, f in enumerate(per_image):
        faces[i, :min(len(f), cap)] = f[:cap]
        counts[i] = len(f)
    return faces, counts


def check_update(trk, ref_streams, streams, per_image, cap=MD, quality=None, cap_ended=8, **kw):
    """one rf_track_update_device call against the reference: the whole tag, ended and count buffers, then every stream's table"""
    trk.update(streams, per_image, cap_per_image=cap, cap_ended=cap_ended, quality=quality, **kw)
    faces, counts = pack(per_image, cap)
    mf = kw.get("max_faces") or MD
    q = None
    if quality is not None:
        q = np.zeros((len(per_image), mf), tr.QUALITY)
        for i, rec in enumerate(quality):
            q[i, :min(len(rec), mf)] = rec[:mf]
    tags, ended, ecounts, trunc = tr.update(ref_streams, streams, faces, counts, cap, kw.get("coord_scale"), q, mf, cap_ended)
    n = len(streams)
    assert trk.last_ended_counts[:n].tobytes() == ecounts.tobytes()
    assert trk.last_tags[:n].tobytes() == tags.tobytes()
    if cap_ended:
        assert trk.last_ended[:n].tobytes() == ended.tobytes()
    assert trk.truncated == trunc
    check_tables(trk, ref_streams)
    return tags, ended, ecounts


def check_tables(trk, ref_streams):
    for s, ref in enumerate(ref_streams):
        table, frames, next_id = trk.read(s)
        assert table.tobytes() == ref.table.tobytes(), s
        assert (frames, next_id) == (ref.frames, ref.next_id), s


@pytest.mark.parametrize("max_tracks", (1, 63, 64, 65, 256))
def test_update_of_constructed_faces_equals_the_reference(rfa, max_tracks):
    """one wavefront with (63, 64) and without (1) a full last ballot, two wavefronts (65), four (256); m = 0, 1, 64, 65 and 256 faces;
    three streams interleaved, one stream five times in a call, an untracked image"""
    det = engine(rfa)
    kw = dict(max_tracks=max_tracks, max_missed=1, min_hits=2)
    trk = det.tracker(3, **kw)
    ref = [tr.Stream(tr.Spec(**kw)) for _ in range(3)]
    rng = np.random.default_rng(max_tracks)
    try:
        ms = (1, 64, 65, 0, 256, 64, 1, 256, 0, 0, 65)
        streams = [0, 1, 2, 0, 1, -1, 2, 0, 0, 0, 0, 0, 1, 2]
        t_of = [0, 0, 0]
        for call in range(3):
            per_image = []
            for i, s in enumerate(streams):
                m = ms[(call * 5 + i) % len(ms)]
                per_image.append(crowd(rng, m, t_of[max(s, 0)]))
                t_of[max(s, 0)] += s >= 0
            tags, ended, ecounts = check_update(trk, ref, streams, per_image, cap_ended=6)
            assert not tags[5].view(np.uint8).any() and ecounts[5] == 0                 # stream -1
        assert ref[0].frames == 3 * 7 and ref[0].next_id > max_tracks                   # ids went past the table size: slots were reused
        # reset: empty tables, frame counter 0, next id 1
        trk.reset(-1)
        check_tables(trk, [tr.Stream(tr.Spec(**kw)) for _ in range(3)])
    finally:
        trk.close()


def test_overflow_max_faces_and_cut_ended_lists(rfa):
    det = engine(rfa)
    kw = dict(max_tracks=4, max_missed=-1)
    trk = det.tracker(2, **kw)
    ref = [tr.Stream(tr.Spec(**kw)) for _ in range(2)]
    rng = np.random.default_rng(7)
    try:
        six = crowd(rng, 6, 0)
        tags, _, _ = check_update(trk, ref, [0], [six])                                  # 6 faces, 4 slots
        assert trk.truncated and [int(t["flags"]) for t in tags[0, :6]] == [5, 5, 5, 5, 24, 24]
        # three tracks end in one frame, cap_ended 1: the count stays true, the first by slot is stored
        tags, ended, ecounts = check_update(trk, ref, [0, 1], [six[:1], six], cap_ended=1)
        assert ecounts[0] == 3 and trk.truncated and ended[0, 0]["id"] in (1, 2, 3, 4)
        # max_faces below the count: the rest is untracked, not overflow
        tags, _, _ = check_update(trk, ref, [1], [six], max_faces=2)
        assert [int(t["flags"]) & tr.UNTRACKED for t in tags[0, :6]] == [0, 0, 8, 8, 8, 8] and not trk.truncated
        # cap_per_image below the count, and no ended buffer at all
        check_update(trk, ref, [0, 1], [six, six], cap=3, cap_ended=0)
        # a coordinate scale per image
        check_update(trk, ref, [0, 1], [six[:2], six[:3]], coord_scale=[float(f32(1280) / f32(448)), 1.0])
    finally:
        trk.close()


def test_quality_records_choose_the_best_shot(rfa):
    det = engine(rfa)
    trk = det.tracker(1, max_tracks=8)
    ref = [tr.Stream(tr.Spec(max_tracks=8))]
    try:
        sharp = [((5.0, 2), (1.0, 0)), ((9.0, 0), (1.0, 4)), ((7.0, 0), (3.0, 0)), ((9.0, 0), (2.0, 0)), ((99.0, 16), (8.0, 0))]
        frames, quality = [], []
        for t, recs in enumerate(sharp):
            frames.append(by_score([face(0.9, 10 + t, 10, 30), face(0.8, 200 + t, 10, 30)]))
            q = np.zeros(2, tr.QUALITY)
            for k, (v, fl) in enumerate(recs):
                q[k]["sharpness"], q[k]["flags"] = v, fl
            quality.append(q)
        check_update(trk, ref, [0] * 5, frames, quality=quality)
        table, _, _ = trk.read(0)
        assert (table[0]["best_frame"], table[0]["best_value"]) == (1, 9.0) and (table[1]["best_frame"], table[1]["best_value"]) == (4, 8.0)
        assert [bool(t["flags"] & tr.BEST) for t in trk.last_tags[:5, 0]] == [False, True, False, False, False]
    finally:
        trk.close()


def test_state_persists_across_calls_and_flush_ends_the_tracks(rfa):
    det = engine(rfa)
    kw = dict(max_tracks=65, max_missed=2)
    rng = np.random.default_rng(3)
    frames = [crowd(rng, (40, 70, 0, 5, 64, 65, 3, 0, 0, 0, 9, 33)[t], t) for t in range(12)]
    one = det.tracker(1, **kw)
    parts = det.tracker(1, **kw)
    try:
        ref = [tr.Stream(tr.Spec(**kw))]
        check_update(one, ref, [0] * 12, frames, cap=80, cap_ended=80)
        whole = (one.last_tags.copy(), one.last_ended.copy(), one.last_ended_counts.copy())
        at = 0
        for k in (1, 5, 6):
            parts.update([0] * k, frames[at:at + k], cap_per_image=80, cap_ended=80)
            det.detect_device([to_device([np.zeros((448, 448, 3), np.uint8)])[0].data_ptr()], [448], [448], 0.5)      # an unrelated call in between
            assert parts.last_tags[:k].tobytes() == whole[0][at:at + k].tobytes()
            assert parts.last_ended[:k].tobytes() == whole[1][at:at + k].tobytes()
            assert parts.last_ended_counts[:k].tobytes() == whole[2][at:at + k].tobytes()
            at += k
        assert parts.read(0)[0].tobytes() == one.read(0)[0].tobytes()
        # flush: the live tracks, slot-ascending; the counters stay
        want = tr.flush(ref[0])
        got = one.flush(0)
        assert len(want) > 0 and got.tobytes() == want.tobytes()
        check_tables(one, ref)
        assert len(one.flush(0)) == 0
        # the whole thing again after a reset: the same bytes
        one.reset(0)
        one.update([0] * 12, frames, cap_per_image=80, cap_ended=80)
        assert (one.last_tags.tobytes(), one.last_ended.tobytes()) == (whole[0].tobytes(), whole[1].tobytes())
    finally:
        one.close()
        parts.close()


# ---------------------------------------------------------------------------------------------- 2. the fused call
def reference_of_call(det, dets_rows, counts, rows, cols, streams, ref_streams, cap_ended):
    faces, _ = pack([tr.faces_array(r) for r in dets_rows], MD)
    scales = [tr_scale(det, r, c) for r, c in zip(rows, cols)]
    return tr.update(ref_streams, streams, faces, np.array(counts, np.int32), MD, scales, None, MD, cap_ended)


def tr_scale(det, rows, cols):
    return f32(det.frame_scale(rows, cols)) if rows and cols else f32(1)


def check_fused(det, trk, ref, ptrs, rows, cols, streams, cap_ended=8, host_frames=None):
    if host_frames is None:
        plain = det.detect_device(ptrs, rows, cols, 0.5)
        got, tags, ended = det.detect_tracked_device(ptrs, rows, cols, trk, streams, 0.5, cap_ended=cap_ended)
    else:
        plain = det.detectBatchImages(host_frames, 0.5)
        got, tags, ended = det.detect_tracked(host_frames, trk, streams, 0.5, cap_ended=cap_ended)
    assert got == plain                                                                  # faces, counts and anchor indices
    n = len(streams)
    wt, we, wc, trunc = reference_of_call(det, [rows_of(d) for d in plain], [len(d) for d in plain], rows, cols, streams, ref, cap_ended)
    assert trk.last_tags[:n].tobytes() == wt.tobytes()
    assert trk.last_ended_counts[:n].tobytes() == wc.tobytes() and trk.last_ended[:n].tobytes() == we.tobytes()
    assert trk.truncated == trunc
    check_tables(trk, ref)
    return plain, tags


@pytest.mark.parametrize("prec,kw", ((FP16, {}), (FP16, SPLIT2), (FP16, SPLIT3), (INT8, {})))
def test_fused_call_equals_detection_plus_the_reference(rfa, base_frame, crop448, prec, kw):
    """SPLIT2 / SPLIT3: the 20 frames of the call ride on launches of 8, 8 and 4 images on different lanes, so both streams have
    frames in every launch and only the chain between the track launches keeps their order."""
    det = split_engine(rfa, kw, prec=prec)
    wins = [np.ascontiguousarray(base_frame[30 + t:478 + t, 380 + 4 * t:828 + 4 * t]) for t in range(20)]
    dev = to_device(wins)
    spec = dict(max_tracks=64, max_missed=1, min_hits=2)
    trk = det.tracker(2, **spec)
    ref = [tr.Stream(tr.Spec(**spec)) for _ in range(2)]
    try:
        streams = [t % 2 for t in range(20)]
        plain, tags = check_fused(det, trk, ref, [d.data_ptr() for d in dev], [448] * 20, [448] * 20, streams)
        assert all(len(p) >= 1 for p in plain)
        assert ref[0].frames == ref[1].frames == 10 and max(int(t["hits"]) for t in tags[18]) == 10
        # a second call continues the streams; an untracked image and a NULL frame (which ages stream 1)
        ptrs = [dev[0].data_ptr(), 0, dev[1].data_ptr(), dev[2].data_ptr()]
        check_fused(det, trk, ref, ptrs, [448, 0, 448, 448], [448, 0, 448, 448], [0, 1, -1, 1])
        assert ref[1].frames == 12
        if prec != FP16 or kw:
            return
        # an oversize frame: tracks live in source pixels (scale 1280 / 448); host frames, an empty one among them
        big = to_device([base_frame])[0]
        check_fused(det, trk, ref, [big.data_ptr(), dev[3].data_ptr()], [896, 448], [1280, 448], [0, 1])
        assert float(ref[0].table["last"]["x2"].max()) > 448
        check_fused(det, trk, ref, None, [896, 0, 448], [1280, 0, 448], [0, 1, 1], host_frames=[base_frame, None, wins[4]])
        # the ordinary call is what it was
        assert det.detect_device([dev[0].data_ptr()], [448], [448], 0.5)[0] == plain[0]
    finally:
        trk.close()


@pytest.mark.parametrize("stem", ("mnet-deconv-0517", "mnet25"))
def test_pan_sequence_keeps_two_ids(rfa, base_frame, stem):
    det = engine(rfa, stem=stem)
    wins = [np.ascontiguousarray(base_frame[30 + 2 * t:478 + 2 * t, 380 + 8 * t:828 + 8 * t]) for t in range(12)]
    dev = to_device(wins)
    trk = det.tracker(1)
    ref = [tr.Stream(tr.Spec())]
    try:
        plain, tags = check_fused(det, trk, ref, [d.data_ptr() for d in dev], [448] * 12, [448] * 12, [0] * 12)
        assert [len(p) for p in plain] == [2] * 12
        ids = {int(g["id"]) for t in tags for g in t}
        assert ids == {1, 2} and all(not (g["flags"] & tr.UNTRACKED) for t in tags for g in t) and sum(len(t) for t in tags) == 24
        table, frames, next_id = trk.read(0)
        assert sorted(table["hits"][table["id"] != 0].tolist()) == [12, 12] and (frames, next_id) == (12, 3)
        for t in range(12):
            assert all(bool(g["flags"] & tr.CONFIRMED) == (t >= 2) for g in tags[t]), t
        if stem == "mnet-deconv-0517":               # the two faces swap score order: ids must not follow rank
            assert len({int(tags[t][0]["id"]) for t in range(12)}) == 2
    finally:
        trk.close()


# ---------------------------------------------------------------------------------------------- 3. the fused face batch
@pytest.mark.parametrize("kw", ({}, SPLIT2))
def test_fused_face_batch_tracks_by_sharpness(rfa, base_frame, kw):
    det = split_engine(rfa, kw)
    wins = [np.ascontiguousarray(base_frame[30 + 2 * t:478 + 2 * t, 380 + 8 * t:828 + 8 * t]) for t in range(12)]
    dev = to_device(wins)
    args = ([d.data_ptr() for d in dev], [448] * 12, [448] * 12)
    base = det.detect_face_batch_device(*args, 0.5, crop_size=112, dtype="f16", return_quality=True)
    sharp = np.array([q["sharpness"] for q in base[4]])                  # (12, 2)
    assert sharp.shape == (12, 2)
    # a gate that drops the first frame's less sharp face, and only some of the later ones
    gate = dict(min_sharpness=float(np.nextafter(f32(sharp[0].min()), f32(np.inf))))
    for g in (None, gate):
        fkw = dict(crop_size=112, dtype="f16", gate=g, return_quality=True)
        want = det.detect_face_batch_device(*args, 0.5, **fkw)
        trk = det.tracker(1, min_hits=1)
        ref = [tr.Stream(tr.Spec(min_hits=1))]
        try:
            got = det.detect_track_face_batch_device(*args, trk, [0] * 12, 0.5, **fkw)
            assert got[0] == want[0] and same(got[1], want[1]) and np.array_equal(got[2], want[2]) and list(got[3]) == list(want[3])
            assert same_records(got[4], want[4])
            faces, counts = pack([tr.faces_array(rows_of(d)) for d in want[0]], MD)
            q = np.zeros((12, MD), tr.QUALITY)
            for i, rec in enumerate(want[4]):
                q[i, :len(rec)] = rec
            wt, _, wc, _ = tr.update(ref, [0] * 12, faces, counts, MD, None, q, MD, 64)
            assert trk.last_tags[:12].tobytes() == wt.tobytes() and trk.last_ended_counts[:12].tobytes() == wc.tobytes()
            check_tables(trk, ref)
            table = trk.read(0)[0]
            live = table[table["id"] != 0]
            assert len(live) == 2 and all(t["best_value"] in sharp for t in live)
            if g is not None:
                k = int(np.argmin(sharp[0]))
                assert want[4][0][k]["flags"] != 0 and wt[0, k]["id"] != 0 and not (wt[0, k]["flags"] & tr.BEST)
                slot = int(wt[0, k]["slot"])
                assert table[slot]["best_frame"] != 0
            # without records the best shot goes by score
            trk.reset(-1)
            plain = det.detect_track_face_batch_device(*args, trk, [0] * 12, 0.5, crop_size=112, dtype="f16")
            assert len(plain) == 6 and same(plain[1], det.detect_face_batch_device(*args, 0.5, crop_size=112, dtype="f16")[1])
            t2 = trk.read(0)[0]
            assert all(float(t["best_value"]) == float(t["best"]["score"]) for t in t2[t2["id"] != 0])
        finally:
            trk.close()


# ---------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_leave_tracker_and_handle_usable(rfa, crop448):
    det = engine(rfa)
    dev = to_device([crop448])[0]
    before = det.detect_device([dev.data_ptr()], [448], [448], 0.5)[0]
    for bad in (dict(max_tracks=257), dict(min_iou=1.5), dict(min_iou=float("nan")), dict(new_score=-1.0)):
        with pytest.raises(rfa.RFError) as e:
            det.tracker(1, **bad)
        assert e.value.status == -1, bad
    for n_streams in (0, 1025):
        with pytest.raises(rfa.RFError):
            det.tracker(n_streams)
    trk = det.tracker(2, max_tracks=4)
    other = engine(rfa, stem="mnet-deconv-0517")
    try:
        one = [by_score([face(0.9, 10, 10, 30)])]
        trk.update([0], one)
        state = trk.read(0)[0].tobytes()
        for call in (lambda: trk.update([2], one), lambda: trk.update([-2], one), lambda: trk.read(2), lambda: trk.reset(5),
                     lambda: det.detect_tracked_device([dev.data_ptr()], [448], [448], trk, [7], 0.5),
                     lambda: other.detect_tracked_device([dev.data_ptr()], [448], [448], trk, [0], 0.5)):      # a tracker of another handle
            with pytest.raises(rfa.RFError) as e:
                call()
            assert e.value.status == -1
        assert trk.read(0)[0].tobytes() == state and trk.read(0)[1] == 1
        assert det.detect_device([dev.data_ptr()], [448], [448], 0.5)[0] == before
        got, tags, _ = det.detect_tracked_device([dev.data_ptr()], [448], [448], trk, [1], 0.5)
        assert got[0] == before and len(tags[0]) == len(before)
    finally:
        trk.close()


def test_multi_device_handles_refuse_trackers(rfa):
    det = rfa.RetinaFace(ASSETS, "net3", 0.4, precision=FP16, net_hw=(448, 448), model_stem="mnet25", devices=[0, 0])
    try:
        with pytest.raises(rfa.RFError) as e:
            det.tracker(1)
        assert e.value.status == -5
    finally:
        det.close()


# ---------------------------------------------------------------------------------------------- 5. the C++ class
def test_cpp_class_detect_tracked(rfa, base_frame, tmp_path):
    src = os.path.join(ROOT, "tests", "csrc", "test_track.cpp")
    exe = str(tmp_path / "test_track")
    lib_dir = os.path.dirname(rfa.lib_path())
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DRF_NO_OPENCV", "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                           "-L" + lib_dir, "-lretinaface_amd", "-Wl,-rpath," + lib_dir])
    wins = [np.ascontiguousarray(base_frame[30 + 2 * t:478 + 2 * t, 380 + 8 * t:828 + 8 * t]) for t in range(6)]
    raw, out = str(tmp_path / "frames.raw"), str(tmp_path / "out.bin")
    np.stack(wins).tofile(raw)
    r = subprocess.run([exe, ASSETS, "mnet25", "448", "448", raw, "6", "0.5", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    blob = open(out, "rb").read()
    det = engine(rfa)
    trk = det.tracker(2)
    try:
        # the program makes two calls of three frames each, streams 0, 1, 0
        pos = 0
        for call in range(2):
            frames = wins[3 * call:3 * call + 3]
            _, tags, ended = det.detect_tracked(frames, trk, [0, 1, 0], 0.5)
            for i in range(3):
                k = int(np.frombuffer(blob, np.int32, 1, pos)[0])
                got = np.frombuffer(blob, tr.TAG, k, pos + 4)
                pos += 4 + 24 * k
                assert got.tobytes() == tags[i].tobytes() and k == 2, (call, i)
                e = int(np.frombuffer(blob, np.int32, 1, pos)[0])
                pos += 4 + 176 * e
                assert e == len(ended[i])
        assert pos == len(blob)
    finally:
        trk.close()
