"""Motion-predicted tracks on the GPU: track_motion_kernel against tests/motion_ref.py byte for byte on constructed faces (tags, ended
lists, counts, tables and motion records), the fused calls on a vertical pan with three dropped frames (ids survive, the plain tracker
loses them), redaction at the predicted coasting boxes, the gallery on a motion tracker, the refusals and the C++ class."""
import os
import subprocess

import numpy as np
import pytest

import face_batch_ref as fbr
import motion_ref as mr
import redact_ref as rr
import shot_ref
import track_ref as tr
from conftest import ASSETS, ROOT, STEMS
from test_gpu_align import FP16, engine, rfa, rows_of, to_device  # noqa: F401  (rfa: fixture)
from test_motion_host import DROPPED, crowd, pan_windows
from test_tile_gpu import INT8
from test_track_gpu import check_tables, pack, tr_scale
from test_track_host import by_score, face

pytestmark = pytest.mark.gpu
f32 = np.float32
MD = 256


def check_motion(trk, ref_streams):
    for s, ref in enumerate(ref_streams):
        assert trk.read_motion(s).tobytes() == ref.motion.tobytes(), s


def check_update(trk, ref_streams, streams, per_image, cap=MD, cap_ended=8):
    """one rf_track_update_device call on a motion tracker against the reference: the whole tag, ended and count buffers, then every
    stream's table and motion records"""
    trk.update(streams, per_image, cap_per_image=cap, cap_ended=cap_ended)
    faces, counts = pack(per_image, cap)
    tags, ended, ecounts, trunc = mr.update(ref_streams, streams, faces, counts, cap, None, None, MD, cap_ended)
    n = len(streams)
    assert trk.last_ended_counts[:n].tobytes() == ecounts.tobytes()
    assert trk.last_tags[:n].tobytes() == tags.tobytes()
    assert trk.last_ended[:n].tobytes() == ended.tobytes()
    assert trk.truncated == trunc
    check_tables(trk, ref_streams)
    check_motion(trk, ref_streams)
    return tags, ended, ecounts


# ---------------------------------------------------------------------------------------------- 1. constructed faces
@pytest.mark.parametrize("max_tracks,alpha,horizon", ((1, 1.0, 1), (64, 0.5, 8), (65, 0.3, -1), (256, 0.0, 0)))
def test_update_of_constructed_faces_equals_the_reference(rfa, max_tracks, alpha, horizon):
    """one wavefront (1, 64), two (65), four (256); m = 0, 1, 64, 65 and 256 faces; three streams interleaved, one stream five times in
    a call, an untracked image; empty images make gaps of one and two frames; a face that moves 12 pixels a frame rides along"""
    det = engine(rfa)
    kw = dict(max_tracks=max_tracks, max_missed=3, min_hits=2)
    trk = det.tracker(3, motion=dict(alpha=alpha, horizon=horizon), **kw)
    plain = det.tracker(3, **kw)
    ref = [mr.Stream(tr.Spec(**kw), mr.Spec(alpha, horizon)) for _ in range(3)]
    rng = np.random.default_rng(max_tracks)
    try:
        ms = (1, 64, 65, 0, 256, 64, 1, 256, 0, 0, 65)
        streams = [0, 1, 2, 0, 1, -1, 2, 0, 0, 0, 0, 0, 1, 2]
        t_of = [0, 0, 0]
        for call in range(3):
            per_image = []
            for i, s in enumerate(streams):
                m = ms[(call * 5 + i) % len(ms)]
                t = t_of[max(s, 0)]
                faces = crowd(rng, min(m, 255), t)
                if m:
                    faces = by_score(list(tr.rows_of(faces)) + [face(0.97, 12.0 * t, 700.0, 30.0)])
                per_image.append(faces)
                t_of[max(s, 0)] += s >= 0
            tags, ended, ecounts = check_update(trk, ref, streams, per_image, cap_ended=6)
            assert not tags[5].view(np.uint8).any() and ecounts[5] == 0                 # stream -1
            plain.update(streams, per_image, cap_per_image=MD, cap_ended=6)
            if horizon < 0:                                                             # never extrapolates: the plain tracker's bytes
                assert plain.last_tags.tobytes() == trk.last_tags.tobytes() and plain.last_ended.tobytes() == trk.last_ended.tobytes()
                assert all(plain.read(s)[0].tobytes() == trk.read(s)[0].tobytes() for s in range(3))
        assert ref[0].frames == 3 * 7 and max(int(r.motion["samples"].max()) for r in ref) > 1
        if max_tracks == 64:                                                            # the mover kept one id over the gaps
            movers = [t for t in ref[0].table if t["id"] != 0 and t["last"]["y1"] == 700]
            assert len(movers) == 1 and movers[0]["hits"] > 8
        # flush ends the live tracks and zeroes their records; reset: empty tables, zero records
        want = mr.flush(ref[1])
        assert trk.flush(1).tobytes() == want.tobytes()
        check_tables(trk, ref)
        check_motion(trk, ref)
        trk.reset(-1)
        fresh = [mr.Stream(tr.Spec(**kw)) for _ in range(3)]
        check_tables(trk, fresh)
        check_motion(trk, fresh)
    finally:
        trk.close()
        plain.close()


# ---------------------------------------------------------------------------------------------- 2. the fused call on the pan
def pan_frames(base_frame):
    wins = pan_windows(base_frame)
    return [np.zeros_like(w) if t in DROPPED else w for t, w in enumerate(wins)], wins


def reference_of_call(det, got, streams, ref_streams, cap_ended):
    faces, _ = pack([tr.faces_array(rows_of(d)) for d in got], MD)
    scales = [tr_scale(det, 448, 448)] * len(got)
    return mr.update(ref_streams, streams, faces, np.array([len(d) for d in got], np.int32), MD, scales, None, MD, cap_ended)


@pytest.mark.parametrize("parts", ((9,), (4, 5)))
@pytest.mark.parametrize("prec", (FP16, INT8))
@pytest.mark.parametrize("stem", STEMS)
def test_pan_with_dropped_frames_keeps_two_ids(rfa, base_frame, stem, prec, parts):
    det = engine(rfa, stem=stem, prec=prec)
    frames, _ = pan_frames(base_frame)
    dev = to_device(frames)
    trk, plain = det.tracker(1, motion=True), det.tracker(1)
    ref = [mr.Stream(tr.Spec())]
    ids, plain_ids, at = set(), set(), 0
    try:
        for k in parts:
            ptrs = [d.data_ptr() for d in dev[at:at + k]]
            got, tags, _ = det.detect_tracked_device(ptrs, [448] * k, [448] * k, trk, [0] * k, 0.5)
            assert [len(g) for g in got] == [0 if t in DROPPED else 2 for t in range(at, at + k)]
            wt, we, wc, trunc = reference_of_call(det, got, [0] * k, ref, 64)
            assert trk.last_tags[:k].tobytes() == wt.tobytes() and trk.last_ended_counts[:k].tobytes() == wc.tobytes()
            assert trk.last_ended[:k].tobytes() == we.tobytes() and trk.truncated == trunc
            check_tables(trk, ref)
            check_motion(trk, ref)
            ids |= {int(g["id"]) for t in tags for g in t}
            want, ptags, _ = det.detect_tracked_device(ptrs, [448] * k, [448] * k, plain, [0] * k, 0.5)
            assert want == got
            plain_ids |= {int(g["id"]) for t in ptags for g in t}
            at += k
        assert ids == {1, 2} and len(plain_ids) == 4
        live = ref[0].table[ref[0].table["id"] != 0]
        assert sorted(live["hits"].tolist()) == [6, 6] and (ref[0].motion["samples"][:2] == 5).all()
        assert (np.abs(ref[0].motion["vy"][:2] + 24) < 6).all()                         # the faces move up 24 pixels a frame
    finally:
        trk.close()
        plain.close()


# ---------------------------------------------------------------------------------------------- 3. redaction at the predicted boxes
@pytest.mark.parametrize("stem", STEMS)
def test_tracked_redaction_follows_the_dropped_faces(rfa, base_frame, stem):
    """one call per frame (a stream may appear once per call).  In the black frames the two coasting regions lie at the predicted boxes;
    rf_redact_device on the REAL window of frame 5 with no faces then covers every pixel of both faces, which the plain tracker's
    `last` boxes do not."""
    import torch
    det = engine(rfa, stem=stem)
    frames, wins = pan_frames(base_frame)
    trk, plain = det.tracker(1, motion=True), det.tracker(1)
    ref = [mr.Stream(tr.Spec())]
    spec = dict(mode=rr.FILL, fill=(0, 255, 0))
    sp = rr.Spec(default_regions=MD, **spec)
    green = np.array([0, 255, 0], np.uint8)
    try:
        for t, f in enumerate(frames):
            work = to_device([f])[0]
            got, tags, _ = trk.detect_redacted_device([work.data_ptr()], [448], [448], [0], 0.5, spec=spec)
            torch.cuda.synchronize()
            wt, _, _, _ = reference_of_call(det, got, [0], ref, 64)
            assert trk.last_tags[:1].tobytes() == wt.tobytes()
            check_tables(trk, ref)
            check_motion(trk, ref)
            want, wpx, true = rr.redact_image(sp, f, rows_of(got[0]), 1.0, mr.predicted_table(ref[0], 0), 10)
            out = work.cpu().numpy()
            assert out.tobytes() == want.tobytes(), (t, int((out != want).any(2).sum()))
            assert trk.last_pixels[0].tobytes() == wpx.tobytes() and trk.last_region_counts[0] == true == 2
            keep = to_device([f])[0]
            det.detect_tracked_device([keep.data_ptr()], [448], [448], plain, [0], 0.5)
            if t != 5:
                continue
            # the real window of frame 5, no faces given: what coasts is all that is redacted
            truth = rows_of(det.detect_device([to_device([wins[5]])[0].data_ptr()], [448], [448], 0.5)[0])
            assert len(truth) == 2
            uncovered = {}
            for name, tracker in (("motion", trk), ("plain", plain)):
                work = to_device([wins[5]])[0]
                _, counts = det.redact_device([work.data_ptr()], [448], [448], [np.zeros((0, 15), f32)], spec=spec, tracker=tracker, streams=[0])
                torch.cuda.synchronize()
                out = work.cpu().numpy()
                assert counts[0] == 2
                uncovered[name] = 0
                for box in truth[:, 1:5]:
                    x0, y0, x1, y1 = mr.box_pixels(box, 448, 448)
                    uncovered[name] += int((out[y0:y1, x0:x1] != green).any(2).sum())
                if name == "motion":
                    table = mr.predicted_table(ref[0], 0)
                    assert out.tobytes() == rr.redact_image(sp, wins[5], np.zeros((0, 15), f32), 1.0, table, 10)[0].tobytes()
            assert uncovered["motion"] == 0 and uncovered["plain"] > 0, uncovered
    finally:
        trk.close()
        plain.close()


# ---------------------------------------------------------------------------------------------- 4. the gallery on a motion tracker
@pytest.mark.parametrize("shots_first", (True, False))
def test_gallery_on_a_motion_tracker_delivers_two_shots(rfa, base_frame, monkeypatch, shots_first):
    det = engine(rfa)
    frames, _ = pan_frames(base_frame)
    dev = to_device(frames)
    ptrs = [d.data_ptr() for d in dev]
    trk, plain = det.tracker(1), det.tracker(1)
    if shots_first:
        trk.enable_shots(crop_size=32, dtype="u8", rgb=False).enable_motion()
    else:
        trk.enable_motion().enable_shots(crop_size=32, dtype="u8", rgb=False)
    plain.enable_shots(crop_size=32, dtype="u8", rgb=False)
    # the reference gallery steps its streams with the motion step
    gal = shot_ref.Gallery(tr.Spec(), 1, fbr.FORMAT_OF["u8"], size=32, rgb=0, max_faces=MD)
    gal.streams = [mr.Stream(tr.Spec())]
    monkeypatch.setattr(shot_ref.track_ref, "step", mr.step)
    try:
        got = det.detect_track_shots_device(ptrs, [448] * 9, [448] * 9, trk, [0] * 9, 0.5)
        faces, counts = pack([tr.faces_array(rows_of(d)) for d in got[0]], MD)
        scales = [tr_scale(det, 448, 448)] * 9
        tags, ended, ecounts, trunc, shots, info, delivered = gal.update(frames, [0] * 9, faces, counts, MD, scales, None, 64)
        assert trk.last_tags[:9].tobytes() == tags.tobytes() and trk.last_ended_counts[:9].tobytes() == ecounts.tobytes()
        assert delivered.sum() == 0 and not trk.truncated
        check_tables(trk, gal.streams)
        check_motion(trk, gal.streams)
        ent, rec = trk.read_shots(0)
        want_ent, want_rec = gal.read(0)
        assert rec.tobytes() == want_rec.tobytes() and ent.tobytes() == want_ent.tobytes()
        g_ended, g_shots, g_info = trk.flush_shots(0)
        w_ended, w_shots, w_info = gal.flush(0)
        assert len(g_ended) == 2 and sorted(g_info["id"].tolist()) == [1, 2]
        assert g_ended.tobytes() == w_ended.tobytes() and g_shots.tobytes() == w_shots.tobytes() and g_info.tobytes() == w_info.tobytes()
        assert not trk.read_motion(0).view(np.uint8).any()                               # the flushed slots' records are zero
        # the plain gallery tracker delivers four shots for the two people
        det.detect_track_shots_device(ptrs, [448] * 9, [448] * 9, plain, [0] * 9, 0.5)
        assert len(plain.flush_shots(0)[0]) == 4
    finally:
        trk.close()
        plain.close()


# ---------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_leave_tracker_and_handle_usable(rfa, crop448):
    det = engine(rfa)
    dev = to_device([crop448])[0]
    before = det.detect_device([dev.data_ptr()], [448], [448], 0.5)[0]
    trk = det.tracker(2, max_tracks=4)
    try:
        with pytest.raises(rfa.RFError) as e:
            trk.read_motion(0)                                                           # no motion yet
        assert e.value.status == -1
        for bad in (dict(alpha=1.5), dict(alpha=-0.5), dict(alpha=float("nan")), dict(horizon=65537)):
            with pytest.raises(rfa.RFError) as e:
                trk.enable_motion(**bad)
            assert e.value.status == -1, bad
        sp = rfa.motion_spec()
        sp.reserved = 1
        assert det._lib.rf_tracker_enable_motion(trk._t, sp) == -1
        sp.reserved, sp.struct_size = 0, 12
        assert det._lib.rf_tracker_enable_motion(trk._t, sp) == -1
        with pytest.raises(rfa.RFError):
            trk.read_motion(0)                                                           # the refusals changed nothing
        one = [by_score([face(0.9, 10, 10, 30)])]
        trk.update([1], one)
        with pytest.raises(rfa.RFError) as e:
            trk.enable_motion()                                                          # a tracker that has stepped a frame
        assert e.value.status == -1
        trk.reset(-1)
        trk.enable_motion(alpha=0.25, horizon=-1)
        with pytest.raises(rfa.RFError) as e:
            trk.enable_motion()                                                          # twice
        assert e.value.status == -1
        for call in (lambda: trk.read_motion(2), lambda: trk.read_motion(-1)):
            with pytest.raises(rfa.RFError) as e:
                call()
            assert e.value.status == -1
        trk.update([0], one)
        trk.update([0], [by_score([face(0.9, 14, 10, 30)])])
        rec = trk.read_motion(0)
        assert rec[0]["samples"] == 1 and rec[0]["vx"] == 4 and not rec[1:].view(np.uint8).any()
        assert not trk.read_motion(1).view(np.uint8).any()
        assert det.detect_device([dev.data_ptr()], [448], [448], 0.5)[0] == before
        got, tags, _ = det.detect_tracked_device([dev.data_ptr()], [448], [448], trk, [1], 0.5)
        assert got[0] == before and len(tags[0]) == len(before)
        # the convenience keyword refuses a bad spec and leaves no tracker behind
        with pytest.raises(rfa.RFError):
            det.tracker(1, motion=dict(alpha=2.0))
    finally:
        trk.close()


def test_multi_device_handles_refuse_motion(rfa):
    det = rfa.RetinaFace(ASSETS, "net3", 0.4, precision=FP16, net_hw=(448, 448), model_stem="mnet25", devices=[0, 0])
    try:
        with pytest.raises(rfa.RFError) as e:
            det.tracker(1, motion=True)
        assert e.value.status == -5
    finally:
        det.close()


# ---------------------------------------------------------------------------------------------- 6. the C++ class
def test_cpp_class_enable_motion(rfa, base_frame, tmp_path):
    src = os.path.join(ROOT, "tests", "csrc", "test_motion.cpp")
    exe = str(tmp_path / "test_motion")
    lib_dir = os.path.dirname(rfa.lib_path())
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DRF_NO_OPENCV", "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                           "-L" + lib_dir, "-lretinaface_amd", "-Wl,-rpath," + lib_dir])
    frames, _ = pan_frames(base_frame)
    raw, out = str(tmp_path / "frames.raw"), str(tmp_path / "out.bin")
    np.stack(frames).tofile(raw)
    r = subprocess.run([exe, ASSETS, "mnet25", "448", "448", raw, "9", "0.5", "0.3", "4", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    blob = open(out, "rb").read()
    det = engine(rfa)
    trk = det.tracker(1, motion=dict(alpha=0.3, horizon=4))
    try:
        pos, ids = 0, set()
        for t in range(9):
            _, tags, _ = det.detect_tracked([frames[t]], trk, [0], 0.5)
            k = int(np.frombuffer(blob, np.int32, 1, pos)[0])
            got = np.frombuffer(blob, tr.TAG, k, pos + 4)
            pos += 4 + 24 * k
            assert got.tobytes() == tags[0].tobytes() and k == (0 if t in DROPPED else 2), t
            ids |= {int(g["id"]) for g in got}
            T = int(np.frombuffer(blob, np.int32, 1, pos)[0])
            rec = trk.read_motion(0)
            assert T == 64 and blob[pos + 4:pos + 4 + 16 * T] == rec.tobytes(), t
            pos += 4 + 16 * T
            table = trk.read(0)[0]
            want = [rfa.track_predict(table[s], rec[s], 1, dict(alpha=0.3, horizon=4)) for s in range(64) if table[s]["id"] != 0 and rec[s]["samples"] > 0]
            p = int(np.frombuffer(blob, np.int32, 1, pos)[0])
            assert p == len(want) and blob[pos + 4:pos + 4 + 60 * p] == b"".join(w.tobytes() for w in want), t
            pos += 4 + 60 * p
        assert pos == len(blob) and ids == {1, 2}
    finally:
        trk.close()
