"""Overlays on the GPU: the two overlay kernels against tests/overlay_ref.py byte for byte on constructed faces (no forward pass) --
whole frames, the bytes around a view, pixel counts and region counts -- with a tracker's coasting tracks and ids, then the fused calls
against their own parts (rf_detect_batch_device + rf_overlay_device fed with its result), the tracked form, non-interference with the
plain, redacting and tracked calls, the refusals and the C++ class."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import motion_ref as mr
import overlay_ref as ov
import track_ref as tr
from conftest import ASSETS, ROOT
from test_gpu_align import FP16, engine, rfa, rows_of, to_device  # noqa: F401  (rfa: fixture)
from test_motion_gpu import check_update as check_motion_update
from test_overlay_host import full_face, with_points
from test_redact_gpu import MD, DevView, grid_faces
from test_redact_host import BIG, face_at, noise, seeded_faces, views
from test_tile_gpu import INT8, SPLIT2, split_engine
from test_track_gpu import check_update
from test_track_host import by_score, face

pytestmark = pytest.mark.gpu
f32 = np.float32


def check_device(det, frames, per_image, ids=None, scales=None, tracker=None, streams=None, tables=None, max_missed=0, **spec):
    """one rf_overlay_device call against the reference.  frames: numpy views or None; ids: per image the faces' track ids, or None;
    tables: per image the track_ref table whose coasting tracks join the list, or None"""
    import torch
    n = len(frames)
    dev = [DevView(f) if f is not None else None for f in frames]
    torch.cuda.synchronize()
    pixels, counts = det.overlay_device([d.ptr if d else 0 for d in dev], [d.rows if d else 0 for d in dev], [d.cols if d else 0 for d in dev],
                                        per_image, ids=ids, steps=[d.step if d else 0 for d in dev], coord_scale=scales, spec=spec,
                                        tracker=tracker, streams=streams)
    sp = ov.Spec(default_regions=MD, **spec)
    assert pixels.shape == (n, sp.max_regions)
    cut = False
    outs = []
    for i, f in enumerate(frames):
        want, wpx, true = ov.overlay_image(sp, f, per_image[i], 1.0 if scales is None else scales[i], ids[i] if ids is not None else None,
                                           tables[i] if tables else None, max_missed)
        cut = cut or true > sp.max_regions
        assert counts[i] == true, (i, counts[i], true)
        if f is None:
            assert not pixels[i].any()
            outs.append(None)
            continue
        got, whole = dev[i].read()
        assert got.tobytes() == want.tobytes(), (i, int((got != want).any(2).sum()))
        assert pixels[i].tobytes() == wpx.tobytes(), (i, np.nonzero(pixels[i] != wpx)[0][:8])
        outside = np.ones(dev[i].base.shape, bool)
        np.lib.stride_tricks.as_strided(outside.reshape(-1)[dev[i].off:], f.shape, f.strides)[:] = False
        assert np.array_equal(whole[outside], np.asarray(dev[i].base)[outside]), i          # nothing around a view was written
        outs.append(got.copy())
    assert det.truncated == cut
    return outs, pixels, counts


# ---------------------------------------------------------------------------------------------- 1. constructed faces
SPECS = (dict(), dict(label=ov.LABEL_SCORE, alpha=128), dict(label=ov.LABEL_ID, color_by_id=True, thickness=3, radius=4, font_scale=1),
         dict(thickness=16, radius=16, font_scale=8, label=ov.LABEL_ID, alpha=77), dict(thickness=1, radius=-1, alpha=1))


@pytest.mark.parametrize("spec", SPECS)
def test_host_shapes_in_one_call_equal_the_reference(rfa, spec):
    """three frames of different sizes and layouts (a padded step, 1 x 1, an ROI view at an odd pointer) and a NULL frame in one call,
    then a coordinate scale per image"""
    det = engine(rfa)
    frames = list(views().values()) + [None]
    rng = np.random.default_rng(3)
    per_image = [with_points(seeded_faces(rng, f.shape[0], f.shape[1], k)) for f, k in zip(frames[:3], (5, 2, 7))] + [face_at(1.0, 1.0, 9.0, 9.0)[None]]
    ids = [[3, 0, 999999, 1000000, 12], [7, 8], [1, 2, 3, 4, 5, 6, 70], [9]]
    outs, pixels, counts = check_device(det, frames, per_image, ids=ids, **spec)
    assert counts[3] == 0 and not np.array_equal(outs[0], frames[0])
    check_device(det, frames[:3], [full_face(-3.0, -2.0, f.shape[1] / 2.0, f.shape[0] / 2.0)[None] for f in frames[:3]], scales=[BIG, 1.0, BIG],
                 **spec)
    check_device(det, frames[:3], per_image[:3], ids=None, scales=[0.5, 3e38, BIG], **spec)


def test_1024_overlapping_regions_in_a_64_x_64_frame_and_the_cut(rfa):
    """the prefilter's worst case: every region meets every other; 1030 faces are cut at 1024"""
    det = engine(rfa)
    rng = np.random.default_rng(9)
    frame = noise(64, 64, 10)
    faces = with_points(grid_faces(rng, 1030, 64, 64))
    faces[:, 3:5] += 20.0                                                        # 22 .. 34 pixels wide: a quarter of the frame each
    _, pixels, counts = check_device(det, [frame], [faces[:1024]], max_regions=1024, thickness=1, radius=1)
    assert counts[0] == 1024 and not det.truncated and (pixels[0] > 0).sum() > 100
    _, pixels, counts = check_device(det, [frame, frame.copy()], [faces, faces[:3]], max_regions=1024, thickness=1, radius=-1)
    assert list(counts) == [1030, 3] and det.truncated
    # the default cap is the engine's max_detections
    _, _, counts = check_device(det, [frame], [faces[:300]], radius=-1)
    assert counts[0] == 300 and det.truncated


@pytest.mark.parametrize("spec", (dict(), dict(thickness=16, radius=16, font_scale=8, label=ov.LABEL_ID, alpha=200)))
def test_a_box_as_large_as_the_frame(rfa, spec):
    """448 x 448: strips that span the frame (several workgroup passes whatever the tiling is), a box larger than the frame on every side
    that paints nothing, one exactly on the border rows and columns, small faces inside"""
    det = engine(rfa)
    frame = noise(448, 448, 3)
    faces = np.stack([full_face(0.0, 0.0, 447.0, 447.0), full_face(-100.0, -60.0, 600.0, 650.0), full_face(8.0, 8.0, 439.0, 439.0),
                      full_face(100.0, 120.0, 180.0, 220.0), full_face(150.0, 150.0, 300.0, 330.0)])
    outs, pixels, _ = check_device(det, [frame], [faces], ids=[[1, 2, 345678, 4, 5]], **spec)
    assert pixels[0, 0] >= 2 * 448 + 2 * 446 and pixels[0, 2] > 0 and pixels[0, 4] > 0
    a = check_device(det, [frame], [faces], ids=[[1, 2, 345678, 4, 5]], **spec)
    assert a[0][0].tobytes() == outs[0].tobytes() and a[1].tobytes() == pixels.tobytes()          # a repeated call gives the same bytes


# ---------------------------------------------------------------------------------------------- 2. trackers
def test_coasting_tracks_are_dashed_where_they_were_last_seen_with_the_tables_ids(rfa):
    det = engine(rfa)
    kw = dict(max_tracks=65, max_missed=3)
    trk = det.tracker(2, **kw)
    ref = [tr.Stream(tr.Spec(**kw)) for _ in range(2)]
    people = [face(0.9, 10, 10, 30), face(0.8, 60, 20, 24), face(0.7, 100, 50, 20), face(0.6, 20, 60, 28)]
    try:
        seq0 = [[0, 1, 2, 3], [0, 2, 3], [0, 2], [0]]
        for t, who in enumerate(seq0):
            tags, _, _ = check_update(trk, ref, [0, 1], [by_score([people[p] for p in who]), by_score([people[2]]) if t < 3 else np.zeros(0, tr.FACE)],
                                      cap_ended=4)
        missed = sorted(int(m) for m in ref[0].table["missed"][ref[0].table["id"] != 0])
        assert missed == [0, 1, 2, 3] and int(ref[1].table["missed"][0]) == 1
        frames = [noise(96, 128, 40), noise(96, 128, 41), noise(96, 128, 42)]
        seen = [tr.rows_of(by_score([people[0]])), np.zeros((0, 15), f32), tr.rows_of(by_score([people[1]]))]
        ids = [[int(tags[0, 0]["id"])], [], [5]]
        tables = [ref[0].table, ref[1].table, None]
        for coast, extra in ((0, 3), (-1, 0), (1, 1), (2, 2)):
            for spec in (dict(), dict(label=ov.LABEL_ID, color_by_id=True, font_scale=1, thickness=3), dict(label=ov.LABEL_SCORE, alpha=99)):
                outs, pixels, counts = check_device(det, frames, seen, ids=ids, tracker=trk, streams=[0, 1, -1], tables=tables, max_missed=3,
                                                    coast=coast, **spec)
                assert list(counts) == [1 + extra, 1 if coast >= 0 else 0, 1]
            if coast < 0:
                assert np.array_equal(outs[1], frames[1])                    # coast negative: no coasting track is drawn
        # a dashed outline paints about half of the solid one
        dashed = check_device(det, frames[1:2], seen[1:2], tracker=trk, streams=[1], tables=tables[1:2], max_missed=3)[1][0, 0]
        solid = check_device(det, frames[1:2], [tr.rows_of(by_score([people[2]]))], radius=-1)[1][0, 0]
        assert solid // 3 < dashed < 2 * solid // 3 + 2
        # the streams the other way round, and a NULL frame on a stream with coasting tracks
        check_device(det, [frames[0], None, frames[2]], [seen[1], seen[0], seen[0]], tracker=trk, streams=[1, 0, -1],
                     tables=[ref[1].table, ref[0].table, None], max_missed=3, label=ov.LABEL_ID)
        for s in range(2):
            assert trk.read(s)[0].tobytes() == ref[s].table.tobytes()      # the overlay only reads the tables
        # refusals leave frames and tracker untouched: a stream twice, a stream out of range
        d = [DevView(f) for f in frames[:2]]
        for streams in ([0, 0], [0, 2]):
            with pytest.raises(rfa.RFError) as e:
                det.overlay_device([v.ptr for v in d], [96, 96], [128, 128], seen[:2], tracker=trk, streams=streams)
            assert e.value.status == -1
        assert all(np.array_equal(v.read()[0], f) for v, f in zip(d, frames))
        for s in range(2):
            assert trk.read(s)[0].tobytes() == ref[s].table.tobytes()
    finally:
        trk.close()


def test_a_motion_tracker_is_dashed_at_the_predicted_box(rfa):
    """a face that moves 12 pixels a frame and then vanishes: the dashed box is at the predicted box, not where it was last seen"""
    det = engine(rfa)
    kw = dict(max_tracks=8, max_missed=3)
    trk = det.tracker(1, motion=dict(alpha=0.5, horizon=8), **kw)
    ref = [mr.Stream(tr.Spec(**kw), mr.Spec(0.5, 8))]
    try:
        for t in range(4):
            check_motion_update(trk, ref, [0], [by_score([face(0.9, 10.0 + 12.0 * t, 30.0, 28.0)])])
        check_motion_update(trk, ref, [0], [np.zeros(0, tr.FACE)])
        table = mr.predicted_table(ref[0], 0)
        live = table[table["id"] != 0]
        assert len(live) == 1 and live["missed"][0] == 1 and live["last"]["x1"][0] > ref[0].table[ref[0].table["id"] != 0]["last"]["x1"][0] + 6
        frame = noise(96, 128, 45)
        _, pixels, counts = check_device(det, [frame], [np.zeros((0, 15), f32)], tracker=trk, streams=[0], tables=[table], max_missed=3,
                                         label=ov.LABEL_ID, color_by_id=True)
        assert counts[0] == 1 and pixels[0, 0] > 0
    finally:
        trk.close()


# ---------------------------------------------------------------------------------------------- 3. the fused calls
def on_device(frames):
    it = iter(to_device([f for f in frames if f is not None]))
    return [next(it) if f is not None else None for f in frames]


def check_fused(det, frames, spec, host=False):
    """rf_detect_overlay_batch[_device] against rf_detect_batch_device on untouched copies + rf_overlay_device (and the reference) on
    its result"""
    import torch
    pd = on_device(frames)
    rows, cols = [f.shape[0] if f is not None else 0 for f in frames], [f.shape[1] if f is not None else 0 for f in frames]
    ptrs = lambda ts: [d.data_ptr() if d is not None else 0 for d in ts]      # noqa: E731
    plain = det.detect_device(ptrs(pd), rows, cols, 0.5)
    anchors = [[d.anchor_index for d in p] for p in plain]
    if host:
        work = [f.copy() if f is not None else None for f in frames]
        got = det.detect_overlay(work, 0.5, spec=spec)                       # out_bgr aliases the input
        outs = work
    else:
        wd = on_device(frames)
        got = det.detect_overlay_device(ptrs(wd), rows, cols, 0.5, spec=spec)
        torch.cuda.synchronize()
        outs = [d.cpu().numpy() if d is not None else None for d in wd]
    assert got == plain and [[d.anchor_index for d in p] for p in got] == anchors          # faces, counts and anchor indices
    fused_pixels = det.last_pixels.copy()
    parts = on_device(frames)
    scales = [det.frame_scale(r, c) if r else 1.0 for r, c in zip(rows, cols)]
    pixels, _ = det.overlay_device(ptrs(parts), rows, cols, [rows_of(p) for p in plain], coord_scale=scales, spec=spec)
    torch.cuda.synchronize()
    sp = ov.Spec(default_regions=MD, **spec)
    total = 0
    for i, f in enumerate(frames):
        if f is None:
            assert not fused_pixels[i].any()
            continue
        assert outs[i].tobytes() == parts[i].cpu().numpy().tobytes(), i
        assert fused_pixels[i].tobytes() == pixels[i].tobytes(), i
        want, wpx, _ = ov.overlay_image(sp, f, rows_of(plain[i]), scales[i])
        assert outs[i].tobytes() == want.tobytes(), (i, int((outs[i] != want).any(2).sum()))
        total += int(wpx.sum())
    assert det.detect_device(ptrs(pd), rows, cols, 0.5) == plain
    assert all(np.array_equal(d.cpu().numpy(), f) for d, f in zip(pd, frames) if f is not None)
    return plain, total


@pytest.mark.parametrize("prec,kw", ((FP16, {}), (FP16, SPLIT2), (INT8, {})))
def test_fused_call_equals_detection_plus_overlay_device(rfa, base_frame, crop448, prec, kw):
    """SPLIT2: the 20 frames of the call ride on launches of 8, 8 and 4 images on two lanes"""
    det = split_engine(rfa, kw, prec=prec)
    wins = [np.ascontiguousarray(base_frame[30 + t:478 + t, 380 + 4 * t:828 + 4 * t]) for t in range(20 if kw else 4)]
    plain, total = check_fused(det, wins, dict(label=ov.LABEL_SCORE))
    assert all(len(p) >= 1 for p in plain) and total > len(wins) * 200
    if kw or prec != FP16:
        return
    # a NULL frame and a frame smaller than the net; then host frames, the annotated frames written over the input
    small = np.ascontiguousarray(crop448[40:400, 20:440])
    plain, _ = check_fused(det, [crop448, None, small, wins[3]], dict(alpha=128, thickness=4))
    assert len(plain[0]) >= 2 and len(plain[1]) == 0
    check_fused(det, [crop448, None, small], dict(label=ov.LABEL_SCORE, font_scale=3), host=True)


def test_tracked_call_over_three_frames_with_a_dropped_face(rfa, crop448):
    """frames 0 and 2 are the fixture crop, frame 1 is grey: the detector finds nothing there, the tracks coast and are drawn dashed with
    their ids.  Tags and tables are those of the tracked call without overlay on a second tracker; the frames are those of
    rf_overlay_device on the call's results."""
    import torch
    det = engine(rfa)
    grey = np.full_like(crop448, 128)
    a, b = det.tracker(1), det.tracker(1)
    spec = dict(label=ov.LABEL_ID, color_by_id=True)
    sp = ov.Spec(default_regions=MD, **spec)
    try:
        for t, f in enumerate([crop448, grey, crop448]):
            work, keep, parts = to_device([f, f, f])
            got, tags, ended = a.detect_tracked_overlay([work.data_ptr()], [448], [448], [0], 0.5, spec=spec)
            torch.cuda.synchronize()
            fused_pixels, fused_counts = a.last_pixels.copy(), a.last_region_counts.copy()
            want, wtags, wended = det.detect_tracked_device([keep.data_ptr()], [448], [448], b, [0], 0.5)
            assert got == want and a.last_tags.tobytes() == b.last_tags.tobytes() and a.last_ended_counts.tobytes() == b.last_ended_counts.tobytes()
            table = b.read(0)[0]
            assert a.read(0)[0].tobytes() == table.tobytes() and a.read(0)[1:] == b.read(0)[1:]
            ids = [a.last_tags[0]["id"][:len(want[0])]]
            pixels, counts = det.overlay_device([parts.data_ptr()], [448], [448], [rows_of(want[0])], ids=ids, spec=spec, tracker=b, streams=[0])
            torch.cuda.synchronize()
            out = work.cpu().numpy()
            assert out.tobytes() == parts.cpu().numpy().tobytes() and fused_pixels[0].tobytes() == pixels[0].tobytes() and fused_counts[0] == counts[0]
            ref_out, wpx, true = ov.overlay_image(sp, f, rows_of(want[0]), 1.0, ids[0], table, 10)
            assert out.tobytes() == ref_out.tobytes(), (t, int((out != ref_out).any(2).sum()))
            assert fused_pixels[0].tobytes() == wpx.tobytes() and fused_counts[0] == true
            if t == 0:
                n_faces = len(want[0])
                assert n_faces >= 1 and true == n_faces and (ids[0] > 0).all()
            if t == 1:
                assert len(want[0]) == 0 and true == n_faces and int(wpx.sum()) > 20 * n_faces and not np.array_equal(out, grey)
        # coast < 0: no coasting tracks; the grey frame stays grey
        work = to_device([grey])[0]
        a.detect_tracked_overlay([work.data_ptr()], [448], [448], [0], 0.5, spec=dict(coast=-1))
        torch.cuda.synchronize()
        assert np.array_equal(work.cpu().numpy(), grey) and a.last_region_counts[0] == 0
        # a stream twice in one call is refused before the tracker changes
        state = a.read(0)[0].tobytes()
        two = to_device([crop448, crop448])
        with pytest.raises(rfa.RFError) as e:
            a.detect_tracked_overlay([d.data_ptr() for d in two], [448] * 2, [448] * 2, [0, 0], 0.5)
        assert e.value.status == -1 and a.read(0)[0].tobytes() == state
        assert all(np.array_equal(d.cpu().numpy(), crop448) for d in two)
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------------------------------------- 4. non-interference, refusals
def test_plain_redacting_and_tracked_calls_are_what_they_were_around_overlay_calls(rfa, crop448):
    import torch
    det = engine(rfa)

    def others():
        dev = to_device([crop448, crop448])
        plain = det.detect_device([dev[0].data_ptr()], [448], [448], 0.5)
        red = det.detect_redacted_device([dev[1].data_ptr()], [448], [448], 0.5, spec=dict(shape=1))
        torch.cuda.synchronize()
        trk = det.tracker(1)
        try:
            tracked = det.detect_tracked_device([dev[0].data_ptr()], [448], [448], trk, [0], 0.5)
            state = (trk.last_tags.tobytes(), trk.read(0)[0].tobytes())
        finally:
            trk.close()
        return plain, red, dev[1].cpu().numpy().tobytes(), det.last_pixels.tobytes(), tracked[0], state

    before = others()
    work = to_device([crop448])[0]
    det.detect_overlay_device([work.data_ptr()], [448], [448], 0.5, spec=dict(label=ov.LABEL_SCORE))
    det.overlay_device([work.data_ptr()], [448], [448], [rows_of(before[0][0])], spec=dict(thickness=5))
    trk = det.tracker(1)
    try:
        trk.detect_tracked_overlay([work.data_ptr()], [448], [448], [0], 0.5)
    finally:
        trk.close()
    assert others() == before


def test_refusals_leave_frames_and_handle_usable(rfa, crop448):
    det = engine(rfa)
    dev = to_device([crop448, crop448])
    args = ([d.data_ptr() for d in dev], [448, 448], [448, 448])
    before = det.detect_device(*args, 0.5)
    faces = [rows_of(before[0]), rows_of(before[1])]
    bad = [dict(thickness=17), dict(radius=17), dict(label=3), dict(font_scale=9), dict(max_regions=1025), dict(thickness=-2)]
    for kw in bad:
        for call in (lambda: det.overlay_device(*args, faces, spec=kw), lambda: det.detect_overlay_device(*args, 0.5, spec=kw),
                     lambda: det.detect_overlay([crop448.copy()], 0.5, spec=kw)):
            with pytest.raises(rfa.RFError) as e:
                call()
            assert e.value.status == -1, kw
    sp = rfa.overlay_spec()
    sp.struct_size = 36
    with pytest.raises(rfa.RFError):
        det.overlay_device(*args, faces, spec=sp)
    # two frames of the call that share bytes: the same frame twice, and a view that starts inside the other
    same = ([dev[0].data_ptr()] * 2, [448, 448], [448, 448])
    inside = ([dev[0].data_ptr(), dev[0].data_ptr() + 448 * 3 * 100], [448, 200], [448, 448])
    for a in (same, inside):
        for call in (lambda: det.overlay_device(*a, faces), lambda: det.detect_overlay_device(*a, 0.5)):
            with pytest.raises(rfa.RFError) as e:
                call()
            assert e.value.status == -1
    # a NULL frame array, more faces than cap_per_image
    lib = rfa.load_library()
    n2 = (C.c_int * 2)(448, 448)
    cnt = (C.c_int * 2)(1, 1)
    one = (rfa._lib.rf_face * 2)()
    assert lib.rf_overlay_device(det._h, None, n2, n2, None, 2, one, None, 1, cnt, None, None, None, None, None, None) == -1
    assert lib.rf_detect_overlay_batch_device(det._h, None, n2, n2, None, 2, 0.5, one, 1, cnt, None, None) == -1
    cnt[0] = 2
    p = (C.c_void_p * 2)(*args[0])
    assert lib.rf_overlay_device(det._h, p, n2, n2, None, 2, one, None, 1, cnt, None, None, None, None, None, None) == -1
    ms = C.c_float()
    # nothing was written, the handle works
    assert all(np.array_equal(d.cpu().numpy(), crop448) for d in dev)
    assert det.detect_device(*args, 0.5) == before
    pixels, counts = det.overlay_device(*args, faces)
    assert list(counts) == [len(f) for f in faces] and pixels[0].sum() > 0 and not np.array_equal(dev[0].cpu().numpy(), crop448)
    assert lib.rf_overlay_last_launch_ms(det._h, C.byref(ms)) == 0 and 0.0 < ms.value < 1000.0


def test_multi_device_handles_refuse_overlays(rfa, crop448):
    det = rfa.RetinaFace(ASSETS, "net3", 0.4, precision=FP16, net_hw=(448, 448), model_stem="mnet25", devices=[0, 0])
    try:
        dev = to_device([crop448])[0]
        for call in (lambda: det.overlay_device([dev.data_ptr()], [448], [448], [face_at(10.0, 10.0, 90.0, 90.0)[None]]),
                     lambda: det.detect_overlay_device([dev.data_ptr()], [448], [448], 0.5),
                     lambda: det.detect_overlay([crop448.copy()], 0.5)):
            with pytest.raises(rfa.RFError) as e:
                call()
            assert e.value.status == -5
        assert np.array_equal(dev.cpu().numpy(), crop448)
    finally:
        det.close()


# ---------------------------------------------------------------------------------------------- 5. the C++ class
def test_cpp_class_detect_overlay_and_detect_tracked_overlay(rfa, crop448, tmp_path):
    src = os.path.join(ROOT, "tests", "csrc", "test_overlay.cpp")
    exe = str(tmp_path / "test_overlay")
    lib_dir = os.path.dirname(rfa.lib_path())
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DRF_NO_OPENCV", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(rocm, "include"), "-o", exe, src, "-L" + lib_dir, "-lretinaface_amd",
                           "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + lib_dir, "-Wl,-rpath," + os.path.join(rocm, "lib")])
    seq = [crop448, np.full_like(crop448, 128), crop448]
    raw, out = str(tmp_path / "frames.raw"), str(tmp_path / "out.bin")
    np.stack(seq).tofile(raw)
    r = subprocess.run([exe, ASSETS, "mnet25", "448", "448", raw, "3", "0.5", str(ov.LABEL_ID), out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    blob = open(out, "rb").read()
    det = engine(rfa)
    spec = dict(label=ov.LABEL_ID, color_by_id=True)
    fb = 448 * 448 * 3

    def section(pos, frames, pixels):
        for i in range(3):
            assert blob[pos + i * fb:pos + (i + 1) * fb] == frames[i].tobytes(), i
        pos += 3 * fb
        for i in range(3):
            k = int(np.frombuffer(blob, np.int32, 1, pos)[0])
            assert k == len(pixels[i]) and np.frombuffer(blob, np.int32, k, pos + 4).tobytes() == pixels[i].tobytes(), i
            pos += 4 + 4 * k
        return pos

    work = [w.copy() for w in seq]
    dets = det.detect_overlay(work, 0.5, spec=spec)
    assert not np.array_equal(work[0], seq[0]) and np.array_equal(work[1], seq[1])
    pos = section(0, work, [det.last_pixels[i, :len(dets[i])] for i in range(3)])
    trk = det.tracker(1)
    try:
        frames, pixels = [], []
        for f in seq:
            d = to_device([f])[0]
            trk.detect_tracked_overlay([d.data_ptr()], [448], [448], [0], 0.5, spec=spec)
            frames.append(d.cpu().numpy())
            pixels.append(trk.last_pixels[0, :min(int(trk.last_region_counts[0]), MD)].copy())
    finally:
        trk.close()
    assert not np.array_equal(frames[1], seq[1]) and len(pixels[1]) == len(pixels[0])      # the dropped faces coast, dashed
    assert section(pos, frames, pixels) == len(blob)
