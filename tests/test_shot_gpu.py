"""The best-shot gallery on the GPU: rf_track_shots_device against tests/shot_ref.py byte for byte on constructed faces (no forward pass)
-- delivered shots and records, tags, ended lists, counts, the table and the gallery read back, and the same frame steps as
rf_track_update_device on a twin tracker without a gallery -- then the fused calls against their own parts (rf_detect_batch_device +
rf_face_quality_device + the reference), the pan sequence, the refusals and the C++ class."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import face_batch_ref as fbr
import shot_ref
import track_ref as tr
from conftest import ASSETS, ROOT
from test_gpu_align import FP16, engine, rfa, rows_of, to_device  # noqa: F401  (rfa: fixture)
from test_tile_gpu import INT8, SPLIT2, SPLIT3, split_engine
from test_track_gpu import check_tables, crowd, pack
from test_track_host import by_score, face
from test_tta_gpu import odd_view

pytestmark = pytest.mark.gpu
f32 = np.float32
MD = 256
NOBODY = np.zeros(0, tr.FACE)


def noise(seed, h=64, w=64):
    """seeded noise plus a gradient, so that crops differ from frame to frame and from place to place"""
    rng = np.random.default_rng(seed)
    g = (np.arange(h)[:, None, None] * 2 + np.arange(w)[None, :, None] * 3 + np.arange(3)[None, None, :] * 40) % 160
    return (g + rng.integers(0, 96, (h, w, 3))).astype(np.uint8)


class Rig:
    """a tracker with a gallery, its twin without one and the reference, fed the same frames and faces"""

    def __init__(self, det, n_streams, spec, dtype="u8", crop=16, **fkw):
        self.det = det
        self.trk = det.tracker(n_streams, **spec).enable_shots(crop_size=crop, dtype=dtype, **fkw)
        self.twin = det.tracker(n_streams, **spec)
        self.gal = shot_ref.Gallery(tr.Spec(**spec), n_streams, fbr.FORMAT_OF[dtype], size=crop, rgb=1 if fkw.get("rgb", True) else 0,
                                    max_faces=fkw.get("max_faces") or MD, antialias=1 if fkw.get("antialias") else 0, aa_max=fkw.get("aa_max") or 4)

    def close(self):
        self.trk.close()
        self.twin.close()

    def call(self, frames, streams, per_image, cap=None, cap_ended=8, quality=None, coord_scale=None, dev=None, **kw):
        """one rf_track_shots_device call against the reference: every buffer whole, then the tables and the gallery"""
        n = len(streams)
        cap = cap or max([len(f) for f in per_image] + [1])
        dev = dev if dev is not None else to_device([f for f in frames if f is not None])
        it = iter(dev)
        ptrs, rows, cols, steps = [], [], [], []
        for f in frames:
            d = next(it) if f is not None else None
            ptrs.append(d[0] if isinstance(d, tuple) else d.data_ptr() if d is not None else 0)
            rows.append(f.shape[0] if f is not None else 0)
            cols.append(f.shape[1] if f is not None else 0)
            steps.append(d[1] if isinstance(d, tuple) else 3 * cols[-1])
        trk, gal = self.trk, self.gal
        trk.update_shots(ptrs, rows, cols, streams, per_image, steps=steps, cap_per_image=cap, cap_ended=cap_ended, quality=quality,
                         coord_scale=coord_scale, **kw)
        faces, counts = pack(per_image, cap)
        q = None
        if quality is not None:
            q = np.zeros((n, gal.max_faces), tr.QUALITY)
            for i, rec in enumerate(quality):
                q[i, :len(rec)] = rec
        tags, ended, ecounts, trunc, shots, info, delivered = gal.update(frames, streams, faces, counts, cap, coord_scale, q, cap_ended)
        assert trk.last_ended_counts[:n].tobytes() == ecounts.tobytes()
        assert trk.last_tags[:n].tobytes() == tags.tobytes()
        if cap_ended:
            assert trk.last_ended[:n].tobytes() == ended.tobytes()
        assert trk.truncated == trunc
        for i in range(n):                       # the delivered shots and records; nothing is written beyond them
            k = int(delivered[i])
            if trk.last_shots is not None:
                assert trk.last_shots[i, :k].tobytes() == shots[i, :k].tobytes(), i
                assert (trk.last_shots[i, k:] == 0xA5).all()
            assert trk.last_shot_info[i, :k].tobytes() == info[i, :k].tobytes(), i
            assert (trk.last_shot_info[i, k:].view(np.uint8) == 0xA5).all()
        check_tables(trk, gal.streams)
        for s in range(len(gal.streams)):
            ent, rec = trk.read_shots(s)
            want_ent, want_rec = gal.read(s)
            assert rec.tobytes() == want_rec.tobytes() and ent.tobytes() == want_ent.tobytes(), s
        # the invariant: the frame steps are those of the plain call on a tracker without a gallery
        twin = self.twin
        twin.update(streams, [p if f is not None else NOBODY for p, f in zip(per_image, frames)], cap_per_image=cap, cap_ended=cap_ended,
                    quality=quality, coord_scale=coord_scale, max_faces=gal.max_faces)
        assert twin.last_tags[:n].tobytes() == trk.last_tags[:n].tobytes() and twin.last_ended[:n].tobytes() == trk.last_ended[:n].tobytes()
        assert twin.last_ended_counts[:n].tobytes() == trk.last_ended_counts[:n].tobytes() and twin.truncated == trk.truncated
        for s in range(len(gal.streams)):
            assert twin.read(s)[0].tobytes() == trk.read(s)[0].tobytes()
        return shots, info, delivered


def small(f, k=0.2):
    """the faces of test_track_gpu.crowd (40-pixel cells) shrunk to 8-pixel cells: 256 of them fit a 140 x 140 frame"""
    rows = tr.rows_of(f).copy()
    rows[:, 1:] *= f32(k)
    return tr.faces_array(rows)


def one(score, x=20.0, y=18.0, w=24.0):
    return by_score([face(score, x, y, w)])


# ---------------------------------------------------------------------------------------------- 1. constructed faces
@pytest.mark.parametrize("dtype,crop,rgb", (("u8", 16, False), ("f16", 112, True)))
def test_one_face_in_one_frame(rfa, dtype, crop, rgb):
    det = engine(rfa)
    rig = Rig(det, 1, dict(max_tracks=4, max_missed=-1), dtype, crop, rgb=rgb)
    try:
        fr = noise(1)
        rig.call([fr], [0], [one(0.5)])
        # the reference crop, cross-checked once against rf_face_batch_device on the same face
        dev = to_device([fr])
        _, tensor, mats, _ = det.face_batch([dev[0].data_ptr()], [64], [64], [tr.rows_of(one(0.5))], crop_size=crop, dtype=dtype, rgb=rgb)
        ent, rec = rig.trk.read_shots(0)
        assert ent[0].tobytes() == tensor[0].tobytes() and ent[0].any()
        assert rec[0]["id"] == 1 and rec[0]["frame"] == 0 and rec[0]["matrix"].tobytes() == mats[0].tobytes()
        assert not ent[1:].any() and not rec[1:].view(np.uint8).any()
        shots, info, delivered = rig.call([noise(2)], [0], [NOBODY])         # the track ends: its shot is frame 0's crop
        assert delivered[0] == 1 and shots[0, 0].tobytes() == tensor[0].tobytes() and info[0, 0]["id"] == 1
    finally:
        rig.close()


def test_antialiased_gallery(rfa):
    det = engine(rfa)
    rig = Rig(det, 1, dict(max_tracks=4, max_missed=-1), "u8", 32, rgb=False, antialias=True)
    try:
        big = by_score([face(0.5, 30, 20, 140)])                          # 140 source pixels onto a 32-pixel crop: factor 4
        rig.call([noise(3, 200, 200), noise(4, 200, 200)], [0, 0], [big, NOBODY])
    finally:
        rig.close()


@pytest.mark.parametrize("split", (False, True))
def test_best_shot_improves_then_does_not_and_the_pixels_are_retained(rfa, split):
    import torch
    det = engine(rfa)
    rig = Rig(det, 1, dict(max_tracks=4, max_missed=-1))
    try:
        frames = [noise(10 + t) for t in range(4)]
        faces = [one(0.5), one(0.75, 21.0), one(0.625, 22.0), NOBODY]
        dev = to_device(frames)
        if split:
            for t in range(3):
                rig.call(frames[t:t + 1], [0], faces[t:t + 1], dev=dev[t:t + 1])
            for d in dev:                                                  # the caller recycles its frame buffers
                d.fill_(7)
            torch.cuda.synchronize()
            shots, info, delivered = rig.call(frames[3:], [0], faces[3:], dev=dev[3:])
            shots, info = shots[0], info[0]
        else:
            shots, info, delivered = rig.call(frames, [0] * 4, faces, dev=dev)
            assert delivered.tolist() == [0, 0, 0, 1]
            shots, info = shots[3], info[3]
        want, m = rig.gal.face_bytes(frames[1], tr.rows_of(faces[1])[0])
        assert shots[0].tobytes() == want.tobytes() and info[0]["frame"] == 1 and info[0]["matrix"].tobytes() == m.tobytes()
    finally:
        rig.close()


def test_born_shot_and_ended_within_one_call_and_slot_reuse(rfa):
    det = engine(rfa)
    rig = Rig(det, 1, dict(max_tracks=1, max_missed=-1))
    try:
        frames = [noise(20 + t) for t in range(5)]
        # frame 1: a track is born; frame 2: it ends and a face elsewhere takes its slot in the same frame; frame 3: that one ends
        shots, info, delivered = rig.call(frames, [0] * 5, [NOBODY, one(0.5, 4.0), one(0.75, 34.0), NOBODY, one(0.25)])
        assert delivered.tolist() == [0, 0, 1, 1, 0] and [int(info[2, 0]["id"]), int(info[3, 0]["id"])] == [1, 2]
        assert shots[2, 0].tobytes() != shots[3, 0].tobytes() and shots[2, 0].any() and shots[3, 0].any()
        # the slot's stored entry is delivered in the call in which its next owner arrives
        shots, info, delivered = rig.call(frames[:2], [0, 0], [one(0.5, 34.0, 30.0), NOBODY])
        assert delivered.tolist() == [1, 1] and [int(info[0, 0]["frame"]), int(info[1, 0]["frame"])] == [4, 5]
    finally:
        rig.close()


@pytest.mark.parametrize("max_tracks", (1, 64, 65, 256))
def test_crowds_three_streams_interleaved(rfa, max_tracks):
    """one wavefront's worth of slots and fewer (1, 64), two (65) and four (256); three streams interleaved, one stream five times in a
    call, an untracked image and a NULL frame; tracks end (max_missed 1) and their slots are reused"""
    det = engine(rfa)
    rig = Rig(det, 3, dict(max_tracks=max_tracks, max_missed=1, min_hits=2))
    rng = np.random.default_rng(max_tracks)
    try:
        ms = (1, 64, 65, 0, 256, 64, 1, 256, 0, 0, 65)
        streams = [0, 1, 2, 0, 1, -1, 2, 0, 0, 0, 0, 0, 1, 2]
        t_of = [0, 0, 0]
        any_shot = 0
        for call in range(3):
            per_image, frames = [], []
            for i, s in enumerate(streams):
                m = min(ms[(call * 5 + i) % len(ms)], 2 * max_tracks)
                per_image.append(small(crowd(rng, m, t_of[max(s, 0)])))
                frames.append(noise(100 * call + i, 140, 140) if (call, i) != (1, 4) else None)
                t_of[max(s, 0)] += s >= 0
            shots, info, delivered = rig.call(frames, streams, per_image, cap=MD, cap_ended=6)
            assert delivered[5] == 0 and not rig.trk.last_tags[5].view(np.uint8).any()      # stream -1
            any_shot += int(delivered.sum())
        assert any_shot > 0 and rig.gal.streams[0].next_id > max_tracks
        # flush: the live tracks with their shots, slot-ascending; then the gallery reads as zeros; reset starts over
        want = rig.gal.flush(0)
        got = rig.trk.flush_shots(0)
        rig.twin.flush(0)
        assert len(want[0]) > 0 and all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
        assert not rig.trk.read_shots(0)[0].any() and not rig.trk.read_shots(0)[1].view(np.uint8).any()
        rig.trk.reset(1)
        rig.twin.reset(1)
        rig.gal.reset(1)
        assert not rig.trk.read_shots(1)[1].view(np.uint8).any()
        rig.call([noise(5, 140, 140)] * 2, [1, 2], [small(crowd(rng, 9, 0)), small(crowd(rng, 5, t_of[2]))], cap=MD)
    finally:
        rig.close()


def test_cut_ended_list_delivers_one_shot_and_the_state_stays_exact(rfa):
    det = engine(rfa)
    rig = Rig(det, 1, dict(max_tracks=4, max_missed=-1))
    try:
        three = by_score([face(0.5, 2, 2, 16), face(0.25, 24, 2, 16), face(0.125, 44, 2, 16)])
        shots, info, delivered = rig.call([noise(30), noise(31)], [0, 0], [three, NOBODY], cap_ended=1)
        assert rig.trk.truncated and rig.trk.last_ended_counts[1] == 3 and delivered.tolist() == [0, 1] and info[1, 0]["id"] == 1
        rig.call([noise(32), noise(33), noise(34)], [0] * 3, [three[:2], three[1:], NOBODY])
    finally:
        rig.close()


def test_gated_faces_deliver_zero_shots(rfa):
    det = engine(rfa)
    rig = Rig(det, 1, dict(max_tracks=4, max_missed=-1))
    try:
        two = by_score([face(0.5, 2, 2, 20), face(0.25, 34, 30, 20)])
        q = np.zeros(2, tr.QUALITY)
        q["flags"], q["sharpness"] = (0, 4), (3.0, 9.0)                  # the second face is gated in every frame
        shots, info, delivered = rig.call([noise(40), noise(41), noise(42)], [0] * 3, [two, two, NOBODY], quality=[q, q, q[:0]])
        assert delivered.tolist() == [0, 0, 2] and info[2, 0]["id"] == 1 and shots[2, 0].any()
        assert info[2, 1]["id"] == 0 and not shots[2, 1].any() and rig.trk.last_ended[2, 1]["best_frame"] == -1
    finally:
        rig.close()


def test_partly_outside_pitched_views_and_scales(rfa):
    det = engine(rfa)
    rig = Rig(det, 2, dict(max_tracks=4, max_missed=-1), "f16", 24)
    try:
        frames = [noise(50), noise(51, 61, 67), noise(52), noise(53)]
        views = [odd_view(f) for f in frames]                            # (tensor, pointer, step): an odd pointer and an odd step
        dev = [(v[1], v[2]) for v in views]
        faces = [one(0.5, 40.0, 40.0, 40.0), one(0.5, -12.0, 10.0, 30.0), NOBODY, NOBODY]      # both faces leave their frames
        shots, info, delivered = rig.call(frames, [0, 1, 0, 1], faces, dev=dev, coord_scale=[1.0, float(f32(1.25)), 1.0, 1.0])
        assert delivered.tolist() == [0, 0, 1, 1] and shots[2, 0].any() and shots[3, 0].any()
    finally:
        rig.close()


def test_device_and_host_destinations(rfa):
    import torch
    det = engine(rfa)
    rig = Rig(det, 1, dict(max_tracks=4, max_missed=-1), "f32", 17)
    try:
        bpf = rig.trk.bytes_per_face
        frames, faces = [noise(60), noise(61)], [one(0.5), NOBODY]
        shots, _, _ = rig.call(frames, [0, 0], faces)                                              # host only
        want = shots[1, 0].tobytes()
        d = torch.full((2 * 8 * bpf + 4,), 0xA5, dtype=torch.uint8, device="cuda")
        for host in (False, True):                                                                   # device only, then both
            d.fill_(0xA5)
            torch.cuda.synchronize()                                                                 # the call runs on a stream of its own
            rig.trk.reset(-1); rig.twin.reset(-1); rig.gal.reset(0)
            rig.call(frames, [0, 0], faces, d_shots=d.data_ptr() + 4, host_shots=host)              # aligned to the element, not to 16
            got = d.cpu().numpy()[4:].reshape(2, 8, bpf)
            assert got[1, 0].tobytes() == want and (got[0] == 0xA5).all() and (got[1, 1:] == 0xA5).all()
    finally:
        rig.close()


# ---------------------------------------------------------------------------------------------- 2. the fused call
def check_fused(det, rig, frames, ptrs, rows, cols, streams, mode, cap_ended=8, host=False):
    """the fused call against rf_detect_batch_device + rf_face_quality_device + the reference"""
    gal, trk = rig.gal, rig.trk
    gate = dict(min_sharpness=1.0) if mode == "gate" else None
    kw = dict(cap_ended=cap_ended, gate=gate, return_quality=mode != "score")
    if host:
        plain = det.detectBatchImages(frames, 0.5)
        got = det.detect_track_shots(frames, trk, streams, 0.5, **kw)
        dev = to_device([f for f in frames if f is not None])
        it = iter(dev)
        ptrs = [next(it).data_ptr() if f is not None else 0 for f in frames]
    else:
        plain = det.detect_device(ptrs, rows, cols, 0.5)
        got = det.detect_track_shots_device(ptrs, rows, cols, trk, streams, 0.5, **kw)
    assert got[0] == plain
    n = len(streams)
    scales = [f32(det.frame_scale(r, c)) if r and c else f32(1) for r, c in zip(rows, cols)]
    per = [tr.faces_array(rows_of(d)) for d in plain]
    quality = None
    if mode != "score":
        quality = det.face_quality(ptrs, rows, cols, [rows_of(d) for d in plain], coord_scale=[float(s) for s in scales], crop_size=gal.size,
                                   max_faces=MD, gate=gate)
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got[5], quality))
    faces, counts = pack(per, MD)
    q = None
    if quality is not None:
        q = np.zeros((n, MD), tr.QUALITY)
        for i, rec in enumerate(quality):
            q[i, :len(rec)] = rec
    tags, ended, ecounts, trunc, shots, info, delivered = gal.update(frames, streams, faces, counts, MD, scales, q, cap_ended)
    assert trk.last_tags[:n].tobytes() == tags.tobytes() and trk.last_ended_counts[:n].tobytes() == ecounts.tobytes()
    assert trk.last_ended[:n].tobytes() == ended.tobytes() and trk.truncated == trunc
    for i in range(n):
        k = int(delivered[i])
        assert trk.last_shots[i, :k].tobytes() == shots[i, :k].tobytes() and (trk.last_shots[i, k:] == 0xA5).all(), i
        assert trk.last_shot_info[i, :k].tobytes() == info[i, :k].tobytes(), i
    check_tables(trk, gal.streams)
    for s in range(len(gal.streams)):
        ent, rec = trk.read_shots(s)
        want_ent, want_rec = gal.read(s)
        assert rec.tobytes() == want_rec.tobytes() and ent.tobytes() == want_ent.tobytes(), s
    return plain, delivered


@pytest.mark.parametrize("prec,kw,mode", ((FP16, {}, "gate"), (FP16, SPLIT2, "quality"), (FP16, SPLIT3, "score"), (INT8, {}, "score")))
def test_fused_call_equals_detection_plus_quality_plus_the_reference(rfa, base_frame, prec, kw, mode):
    """SPLIT2 / SPLIT3: the 20 frames of the call ride on launches of 8, 8 and 4 images on different lanes, so both streams have frames
    in every launch and only the chain between the track and shot launches keeps their order.  Every fourth frame is blank, so tracks
    end (max_missed 0) and are born again inside the call."""
    det = split_engine(rfa, kw, prec=prec)
    wins = [np.ascontiguousarray(base_frame[30 + t:478 + t, 380 + 4 * t:828 + 4 * t]) if t % 8 < 6 else noise(t, 448, 448) // 8 for t in range(20)]
    dev = to_device(wins)
    spec = dict(max_tracks=64, max_missed=-1, min_hits=2)
    rig = Rig(det, 2, spec, "u8", 32, rgb=False)
    try:
        streams = [t % 2 for t in range(20)]
        plain, delivered = check_fused(det, rig, wins, [d.data_ptr() for d in dev], [448] * 20, [448] * 20, streams, mode)
        assert all(len(plain[t]) >= 1 for t in range(6)) and delivered.sum() >= 2
        # a second call continues the streams; an untracked image and a NULL frame (which ends stream 1's tracks)
        frames = [wins[0], None, wins[1], wins[2]]
        _, delivered = check_fused(det, rig, frames, [dev[0].data_ptr(), 0, dev[1].data_ptr(), dev[2].data_ptr()], [448, 0, 448, 448],
                                   [448, 0, 448, 448], [0, 1, -1, 1], mode)
        if prec != FP16 or kw:
            return
        # an oversize frame is sampled at full resolution (scale 1280 / 448); host frames, an empty one among them
        big = to_device([base_frame])[0]
        check_fused(det, rig, [base_frame, wins[3]], [big.data_ptr(), dev[3].data_ptr()], [896, 448], [1280, 448], [0, 1], mode)
        _, delivered = check_fused(det, rig, [wins[9], None, wins[4]], None, [448, 0, 448], [448, 0, 448], [0, 1, 1], mode, host=True)
        assert delivered.sum() >= 1
    finally:
        rig.close()


@pytest.mark.parametrize("stem", ("mnet-deconv-0517", "mnet25"))
def test_pan_sequence_delivers_two_shots(rfa, base_frame, stem):
    det = engine(rfa, stem=stem)
    wins = [np.ascontiguousarray(base_frame[30 + 2 * t:478 + 2 * t, 380 + 8 * t:828 + 8 * t]) for t in range(12)]
    dev = to_device(wins)
    rig = Rig(det, 1, {}, "f16", 112)
    try:
        plain, delivered = check_fused(det, rig, wins, [d.data_ptr() for d in dev], [448] * 12, [448] * 12, [0] * 12, "quality")
        assert [len(p) for p in plain] == [2] * 12 and delivered.sum() == 0
        ended, shots, info = rig.trk.flush_shots(0)
        assert len(ended) == 2 and sorted(info["id"].tolist()) == [1, 2]
        for e in range(2):                       # each shot is the face-batch crop of its track's best_frame window
            bf = int(ended[e]["best_frame"])
            assert info[e]["frame"] == bf
            k = [int(g["id"]) for g in rig.trk.last_tags[bf, :2]].index(int(ended[e]["id"]))
            _, tensor, mats, _ = det.face_batch([dev[bf].data_ptr()], [448], [448], [rows_of(plain[bf])[k:k + 1]], crop_size=112, dtype="f16")
            assert shots[e].tobytes() == tensor[0].tobytes() and info[e]["matrix"].tobytes() == mats[0].tobytes()
    finally:
        rig.close()


# ---------------------------------------------------------------------------------------------- 3. refusals
def test_refusals_leave_tracker_and_handle_usable(rfa, crop448):
    det = engine(rfa)
    dev = to_device([crop448])[0]
    args = ([dev.data_ptr()], [448], [448])
    one_face = [one(0.9)]
    trk = det.tracker(2, max_tracks=4)
    plain = det.tracker(1, max_tracks=4)
    big = det.tracker(1024, max_tracks=256)
    wide = det.tracker(1, max_tracks=2)
    try:
        def refused(call):
            with pytest.raises(rfa.RFError) as e:
                call()
            assert e.value.status == -1

        refused(lambda: trk.enable_shots(crop_size=8))                                   # a bad spec
        refused(lambda: trk.enable_shots(capacity=0))
        refused(lambda: big.enable_shots(crop_size=112, dtype="f32"))                    # 1024 x 256 x 150 528 bytes: above 1 GiB
        plain.update([0], one_face)
        refused(lambda: plain.enable_shots())                                            # it has stepped a frame
        trk.enable_shots(crop_size=16, dtype="u8")
        refused(lambda: trk.enable_shots(crop_size=16, dtype="u8"))                      # twice
        # an old tracked call on a gallery tracker, a new one on a plain tracker: nothing changes
        refused(lambda: trk.update([0], one_face))
        refused(lambda: det.detect_tracked_device(*args, trk, [0], 0.5))
        refused(lambda: det.detect_track_face_batch_device(*args, trk, [0], 0.5))
        refused(lambda: trk.detect_redacted_device(*args, [0], 0.5))
        plain.shot_max_faces, plain.bytes_per_face = MD, 768
        refused(lambda: det.detect_track_shots_device(*args, plain, [0], 0.5))
        refused(lambda: plain.update_shots(*args, [0], one_face))
        refused(lambda: plain.read_shots(0))
        refused(lambda: trk.update_shots(*args, [2], one_face))                          # a stream out of range
        wide.enable_shots(crop_size=512, dtype="f32")                                    # 3 MiB per face: 400 of them are above 1 GiB
        refused(lambda: wide.update_shots(*args, [0], one_face, d_shots=dev.data_ptr(), host_shots=False, cap_ended=400))
        refused(lambda: trk.read_shots(2))
        assert trk.read(0)[1] == 0 and plain.read(0)[1] == 1
        lib, h = det._lib, det._h
        assert lib.rf_track_shots_device(h, trk._t, None, None, None, None, 1, None, None, 1, None, None, None, None, None, 0, None, None, None,
                                         None) == -1                                     # bad pointers
        assert lib.rf_tracker_enable_shots(trk._t, None) == -1
        got = det.detect_track_shots_device(*args, trk, [1], 0.5)
        assert got[0] == det.detect_device(*args, 0.5) and len(got[1][0]) == len(got[0][0])
    finally:
        for t in (trk, plain, big, wide):
            t.close()


def test_multi_device_handles_refuse_the_gallery(rfa):
    det = rfa.RetinaFace(ASSETS, "net3", 0.4, precision=FP16, net_hw=(448, 448), model_stem="mnet25", devices=[0, 0])
    try:
        lib, h = det._lib, det._h
        fake = C.c_void_p(1)                     # no tracker exists on such a handle: the handle is refused before the tracker is looked at
        assert lib.rf_track_shots_device(h, fake, None, None, None, None, 0, None, None, 1, None, None, None, None, None, 0, None, None, None,
                                         None) == -5
        assert lib.rf_detect_track_shots_batch_device(h, None, None, None, None, 0, 0.5, None, 0, None, fake, None, None, None, 0, None, None, None,
                                                      None, None, None) == -5
    finally:
        det.close()


# ---------------------------------------------------------------------------------------------- 4. the C++ class
def test_cpp_class_detect_track_shots(rfa, base_frame, tmp_path):
    src = os.path.join(ROOT, "tests", "csrc", "test_shot.cpp")
    exe = str(tmp_path / "test_shot")
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
    trk = det.tracker(1).enable_shots(crop_size=32, dtype="u8", rgb=False)
    try:
        # the program makes two calls of three frames each on one stream and then flushes it
        det.detect_track_shots(wins[:3], trk, [0] * 3, 0.5)
        det.detect_track_shots(wins[3:], trk, [0] * 3, 0.5)
        ended, shots, info = trk.flush_shots(0)
        assert len(ended) == 2
        assert blob == np.int32(len(ended)).tobytes() + ended.tobytes() + shots.tobytes() + info.tobytes()
    finally:
        trk.close()
