"""Blur redaction on the GPU: redact_blur_kernel and the shadow-copying write kernel against tests/redact_blur_ref.py byte for byte on
constructed faces (no forward pass) -- whole frames, the bytes around a view, pixel counts and region counts --, with coasting and
motion-predicted tracks, then the fused calls against their own parts, non-interference with the plain and the pixelating calls, the
refusals and the C++ class."""
import os
import subprocess

import numpy as np
import pytest

import motion_ref as mr
import redact_blur_ref as rb
import redact_ref as rr
import track_ref as tr
from conftest import ASSETS, ROOT
from test_gpu_align import FP16, engine, rfa, rows_of, to_device  # noqa: F401  (rfa: fixture)
from test_motion_gpu import check_update as check_motion_update
from test_redact_gpu import MD, DevView, grid_faces
from test_redact_host import BIG, face_at, noise, seeded_faces, views
from test_tile_gpu import INT8, SPLIT2, split_engine
from test_track_gpu import check_update
from test_track_host import by_score, face

pytestmark = pytest.mark.gpu
f32 = np.float32


def check_device(det, frames, per_image, scales=None, tracker=None, streams=None, tables=None, max_missed=0, dev=None, **spec):
    """one rf_redact_device call against the blur reference.  frames: numpy views or None; tables: per image the track_ref table whose
    coasting tracks join the list, or None; dev: DevViews to reuse (frames already on the device)"""
    import torch
    n = len(frames)
    dev = dev or [DevView(f) if f is not None else None for f in frames]
    torch.cuda.synchronize()
    pixels, counts = det.redact_device([d.ptr if d else 0 for d in dev], [d.rows if d else 0 for d in dev], [d.cols if d else 0 for d in dev],
                                       per_image, steps=[d.step if d else 0 for d in dev], coord_scale=scales, spec=spec, tracker=tracker,
                                       streams=streams)
    sp = rb.Spec(default_regions=MD, **spec)
    assert pixels.shape == (n, sp.max_regions)
    cut = False
    outs = []
    for i, f in enumerate(frames):
        want, wpx, true = rb.redact_image(sp, f, per_image[i], 1.0 if scales is None else scales[i], tables[i] if tables else None, max_missed)
        cut = cut or true > sp.max_regions
        assert counts[i] == true, (i, counts[i], true)
        assert pixels[i].tobytes() == wpx.tobytes(), (i, np.nonzero(pixels[i] != wpx)[0][:8])
        if f is None:
            outs.append(None)
            continue
        got, whole = dev[i].read()
        assert got.tobytes() == want.tobytes(), (i, int((got != want).any(2).sum()))
        outside = np.ones(dev[i].base.shape, bool)
        np.lib.stride_tricks.as_strided(outside.reshape(-1)[dev[i].off:], f.shape, f.strides)[:] = False
        assert np.array_equal(whole[outside], np.asarray(dev[i].base)[outside]), i          # nothing around a view was written
        outs.append(got.copy())
    assert det.truncated == cut
    return outs, pixels, counts


# ---------------------------------------------------------------------------------------------- 1. constructed faces
@pytest.mark.parametrize("shape", (rr.RECT, rr.ELLIPSE))
@pytest.mark.parametrize("blur", (1, 2, 3))
def test_host_shapes_in_one_call_equal_the_reference(rfa, blur, shape):
    """three frames of different sizes and layouts (a padded step, 1 x 1, an ROI view at an odd pointer) and a NULL frame in one call;
    cells = 1 makes the radius larger than the frames"""
    det = engine(rfa)
    frames = list(views().values()) + [None]
    for cells in (1, 8, 64):
        rng = np.random.default_rng(cells + blur)
        per_image = [seeded_faces(rng, f.shape[0], f.shape[1], k) for f, k in zip(frames[:3], (5, 2, 7))] + [face_at(1.0, 1.0, 9.0, 9.0)[None]]
        outs, pixels, counts = check_device(det, frames, per_image, blur=blur, shape=shape, cells=cells)
        assert counts[3] == 0 and not pixels[3].any()
        assert not np.array_equal(outs[0], frames[0])
    # a coordinate scale per image
    check_device(det, frames[:3], [face_at(-3.0, -2.0, f.shape[1] / 2.0, f.shape[0] / 2.0)[None] for f in frames[:3]], scales=[BIG, 1.0, BIG],
                 blur=blur, shape=shape)


def test_tile_seams_in_both_axes(rfa):
    """448 x 448 noise, one 257 x 131 region (rho = 33): several tiles across and down whatever the tile is, none of them whole at the
    far edges"""
    det = engine(rfa)
    frame = noise(448, 448, 50)
    box = face_at(90.0, 200.0, 346.5, 330.5)[None]
    r = rr.region(rr.Spec(margin=-1.0), box[0, 1:5], 1.0, 448, 448)
    assert (r.ux1 - r.ux0, r.uy1 - r.uy0) == (257, 131)
    for blur in (1, 3):
        _, pixels, _ = check_device(det, [frame], [box], blur=blur, margin=-1.0)
        assert pixels[0, 0] == 257 * 131
    check_device(det, [frame], [box], blur=2, margin=-1.0, cells=64, shape=rr.ELLIPSE)          # rho = 5


def test_a_region_that_covers_a_large_frame(rfa):
    """1280 x 896, one region larger than the frame on every side: the radius cap, the clamp at all four borders and many tiles; small
    faces behind it in the list own nothing"""
    det = engine(rfa)
    frame = noise(896, 1280, 3)
    faces = np.concatenate([face_at(-100.0, -60.0, 1400.0, 950.0)[None], seeded_faces(np.random.default_rng(4), 896, 1280, 3)])
    _, pixels, _ = check_device(det, [frame], [faces], blur=3, margin=-1.0)
    assert pixels[0, 0] == 896 * 1280 and not pixels[0, 1:].any()
    assert rb.radius(rr.region(rr.Spec(margin=-1.0), faces[0, 1:5], 1.0, 896, 1280)) == 64


@pytest.mark.parametrize("shape", (rr.RECT, rr.ELLIPSE))
def test_a_small_region_inside_a_large_one(rfa, shape):
    """index 0 small (rho 3), index 1 large (rho 19): inside the small one its own radius, around it the large one's"""
    det = engine(rfa)
    frame = noise(200, 240, 51)
    faces = np.stack([face_at(100.0, 80.0, 123.0, 103.0), face_at(30.0, 20.0, 180.0, 170.0)])
    outs, pixels, _ = check_device(det, [frame], [faces], blur=2, margin=-1.0, shape=shape)
    sp = rb.Spec(blur=2, margin=-1.0, shape=shape)
    regs = [rr.region(sp, f[1:5], 1.0, 200, 240) for f in faces]
    assert [rb.radius(r) for r in regs] == [3, 19] and pixels[0, 0] > 0 and pixels[0, 1] > 0
    m0 = rr.mask(sp, regs[0])
    inner = outs[0][regs[0].cy0:regs[0].cy1, regs[0].cx0:regs[0].cx1]
    assert np.array_equal(inner[m0], rb.blurred(frame, 3, 2)[regs[0].cy0:regs[0].cy1, regs[0].cx0:regs[0].cx1][m0])
    assert tuple(outs[0][25, 100]) == tuple(rb.blurred(frame, 19, 2)[25, 100])
    # the other way round the small one owns nothing
    _, pixels, _ = check_device(det, [frame], [faces[::-1].copy()], blur=2, margin=-1.0)
    assert pixels[0, 1] == 0


def test_region_counts_up_to_the_cap_and_beyond(rfa):
    det = engine(rfa)
    rng = np.random.default_rng(9)
    counts = (0, 1, 65, 1024)
    frames = [noise(96, 128, 10 + i) for i in range(len(counts))]
    per_image = [grid_faces(rng, k, 96, 128) for k in counts]
    _, pixels, got = check_device(det, frames, per_image, blur=2, cells=4, max_regions=1024, shape=rr.ELLIPSE)
    assert list(got) == list(counts) and not det.truncated and (pixels[3] > 0).sum() > 200
    more = grid_faces(rng, 1025, 96, 128)
    _, _, got = check_device(det, frames[:2], [more, per_image[1]], blur=1, cells=4, max_regions=1024)
    assert list(got) == [1025, 1] and det.truncated


def test_scratch_is_reused_across_calls_of_different_sizes(rfa):
    """a large frame, then small ones (their offsets lie inside the block the large call left), then the large one again"""
    det = engine(rfa)
    large = noise(600, 800, 60)
    big_face = [face_at(100.0, 80.0, 500.0, 420.0)[None]]
    small = [noise(96, 128, 61), noise(50, 70, 62), noise(96, 128, 63)]
    rng = np.random.default_rng(64)
    small_faces = [seeded_faces(rng, f.shape[0], f.shape[1], 3) for f in small]
    a = check_device(det, [large], big_face, blur=3)
    check_device(det, small, small_faces, blur=3)
    check_device(det, small[::-1], small_faces[::-1], blur=1, cells=3)
    b = check_device(det, [large], big_face, blur=3)
    assert a[0][0].tobytes() == b[0][0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---------------------------------------------------------------------------------------------- 2. coasting tracks
def test_coasting_tracks_are_blurred_where_they_were_last_seen(rfa):
    det = engine(rfa)
    kw = dict(max_tracks=65, max_missed=3)
    trk = det.tracker(2, **kw)
    ref = [tr.Stream(tr.Spec(**kw)) for _ in range(2)]
    people = [face(0.9, 10, 10, 30), face(0.8, 60, 20, 24), face(0.7, 100, 50, 20), face(0.6, 20, 60, 28)]
    try:
        seq0 = [[0, 1, 2, 3], [0, 2, 3], [0, 2], [0]]
        for t, who in enumerate(seq0):
            check_update(trk, ref, [0, 1], [by_score([people[p] for p in who]), by_score([people[2]]) if t < 3 else np.zeros(0, tr.FACE)], cap_ended=4)
        frames = [noise(96, 128, 40), noise(96, 128, 41), noise(96, 128, 42)]
        seen = [by_score([people[0]]), np.zeros((0, 15), f32), by_score([people[1]])]
        tables = [ref[0].table, ref[1].table, None]
        for coast, extra in ((0, 3), (1, 1)):
            _, _, counts = check_device(det, frames, seen, tracker=trk, streams=[0, 1, -1], tables=tables, max_missed=3, coast=coast, blur=2,
                                        shape=rr.ELLIPSE)
            assert list(counts) == [1 + extra, 1, 1]
        for s in range(2):
            assert trk.read(s)[0].tobytes() == ref[s].table.tobytes()
    finally:
        trk.close()


def test_a_motion_tracker_coasts_at_the_predicted_box(rfa):
    """a face that moves 12 pixels a frame and then vanishes: the blurred region is at the predicted box, not where it was last seen"""
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
        _, pixels, counts = check_device(det, [frame], [np.zeros((0, 15), f32)], tracker=trk, streams=[0], tables=[table], max_missed=3, blur=3)
        assert counts[0] == 1 and pixels[0, 0] > 0
    finally:
        trk.close()


# ---------------------------------------------------------------------------------------------- 3. the fused calls
def check_fused(det, frames, spec, host=False):
    """rf_detect_redact_batch[_device] with a blur against rf_detect_batch_device on untouched copies + the reference on its result"""
    import torch
    plain_dev = to_device([f for f in frames if f is not None])
    it = iter(plain_dev)
    pd = [next(it) if f is not None else None for f in frames]
    rows, cols = [f.shape[0] if f is not None else 0 for f in frames], [f.shape[1] if f is not None else 0 for f in frames]
    plain = det.detect_device([d.data_ptr() if d is not None else 0 for d in pd], rows, cols, 0.5)
    if host:
        work = [f.copy() if f is not None else None for f in frames]
        got = det.detect_redacted(work, 0.5, spec=spec)
        outs = work
    else:
        wd = to_device([f for f in frames if f is not None])
        it = iter(wd)
        wd = [next(it) if f is not None else None for f in frames]
        got = det.detect_redacted_device([d.data_ptr() if d is not None else 0 for d in wd], rows, cols, 0.5, spec=spec)
        torch.cuda.synchronize()
        outs = [d.cpu().numpy() if d is not None else None for d in wd]
    assert got == plain                                                                  # faces, counts and anchor indices
    sp = rb.Spec(default_regions=MD, **spec)
    total = 0
    for i, f in enumerate(frames):
        if f is None:
            assert not det.last_pixels[i].any()
            continue
        want, wpx, _ = rb.redact_image(sp, f, rows_of(plain[i]), det.frame_scale(rows[i], cols[i]))
        assert outs[i].tobytes() == want.tobytes(), (i, int((outs[i] != want).any(2).sum()))
        assert det.last_pixels[i].tobytes() == wpx.tobytes(), i
        total += int(wpx.sum())
    assert det.detect_device([d.data_ptr() if d is not None else 0 for d in pd], rows, cols, 0.5) == plain
    assert all(np.array_equal(d.cpu().numpy(), f) for d, f in zip(pd, frames) if f is not None)
    return plain, total


@pytest.mark.parametrize("prec,kw", ((FP16, {}), (FP16, SPLIT2), (INT8, {})))
def test_fused_call_equals_detection_plus_the_reference(rfa, base_frame, crop448, prec, kw):
    """SPLIT2: the 20 frames of the call ride on launches on different lanes, each with its own slice of the shadow"""
    det = split_engine(rfa, kw, prec=prec)
    wins = [np.ascontiguousarray(base_frame[30 + t:478 + t, 380 + 4 * t:828 + 4 * t]) for t in range(20 if kw else 3)]
    plain, total = check_fused(det, wins, dict(blur=3, shape=rr.ELLIPSE))
    assert all(len(p) >= 1 for p in plain) and total > len(wins) * 400
    if kw or prec != FP16:
        return
    # a NULL frame and an oversize frame, which is blurred at its full resolution
    plain, total = check_fused(det, [crop448, None, base_frame, wins[2]], dict(blur=3, cells=6))
    assert len(plain[2]) >= 2 and len(plain[1]) == 0
    check_fused(det, [crop448, None, wins[1]], dict(blur=3), host=True)


def test_tracked_fused_call_blurs_a_missed_face(rfa, crop448):
    """frames 0 and 1 are the fixture crop, frame 2 is a gradient the detector finds nothing in: the tracks coast and their regions are
    blurred where the faces were last seen"""
    import torch
    det = engine(rfa)
    ramp = np.ascontiguousarray(np.broadcast_to((np.arange(448) % 256).astype(np.uint8)[None, :, None], (448, 448, 3)))
    a, b = det.tracker(1), det.tracker(1)
    spec = dict(blur=3)
    sp = rb.Spec(default_regions=MD, **spec)
    try:
        for t, f in enumerate([crop448, crop448, ramp]):
            work, keep = to_device([f, f])
            got, _, _ = a.detect_redacted_device([work.data_ptr()], [448], [448], [0], 0.5, spec=spec)
            torch.cuda.synchronize()
            want, _, _ = det.detect_tracked_device([keep.data_ptr()], [448], [448], b, [0], 0.5)
            assert got == want and a.last_tags.tobytes() == b.last_tags.tobytes()
            table = b.read(0)[0]
            assert a.read(0)[0].tobytes() == table.tobytes()
            ref_out, wpx, true = rb.redact_image(sp, f, rows_of(want[0]), 1.0, table, 10)
            out = work.cpu().numpy()
            assert out.tobytes() == ref_out.tobytes(), (t, int((out != ref_out).any(2).sum()))
            assert a.last_pixels[0].tobytes() == wpx.tobytes() and a.last_region_counts[0] == true
            if t == 1:
                n_faces = len(want[0])
                assert n_faces >= 1
            if t == 2:
                assert len(want[0]) == 0 and true == n_faces and int(wpx.sum()) > 400 * n_faces and not np.array_equal(out, ramp)
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------------------------------------- 4. non-interference, refusals
def test_plain_and_pixelating_calls_are_what_they_were_around_a_blurred_one(rfa, crop448):
    import torch
    det = engine(rfa)

    def plain_and_pixelated():
        d = to_device([crop448, crop448])
        dets = det.detect_device([d[0].data_ptr()], [448], [448], 0.5)
        red = det.detect_redacted_device([d[1].data_ptr()], [448], [448], 0.5, spec=dict(blur=0, shape=rr.ELLIPSE))
        torch.cuda.synchronize()
        assert np.array_equal(d[0].cpu().numpy(), crop448)
        return dets, red, d[1].cpu().numpy().tobytes(), det.last_pixels.tobytes()

    before = plain_and_pixelated()
    want, _, _ = rr.redact_image(rr.Spec(default_regions=MD, shape=rr.ELLIPSE), crop448, rows_of(before[0][0]), 1.0)
    assert before[2] == want.tobytes() and before[0] == before[1]
    work = to_device([crop448])[0]
    det.detect_redacted_device([work.data_ptr()], [448], [448], 0.5, spec=dict(blur=3, shape=rr.ELLIPSE))
    torch.cuda.synchronize()
    assert work.cpu().numpy().tobytes() != before[2]
    assert plain_and_pixelated() == before


def test_refusals_leave_frames_and_handle_usable(rfa, crop448):
    det = engine(rfa)
    dev = to_device([crop448, crop448])
    args = ([d.data_ptr() for d in dev], [448, 448], [448, 448])
    before = det.detect_device(*args, 0.5)
    faces = [rows_of(before[0]), rows_of(before[1])]
    trk = det.tracker(2)
    try:
        for kw in (dict(blur=4), dict(blur=255), dict(blur=1, mode=rr.FILL), dict(blur=2, mode=2)):
            for call in (lambda: det.redact_device(*args, faces, spec=kw), lambda: det.detect_redacted_device(*args, 0.5, spec=kw),
                         lambda: det.detect_redacted([crop448.copy()], 0.5, spec=kw),
                         lambda: trk.detect_redacted_device(*args, [0, 1], 0.5, spec=kw)):
                with pytest.raises(rfa.RFError) as e:
                    call()
                assert e.value.status == -1, kw
        assert all(np.array_equal(d.cpu().numpy(), crop448) for d in dev)
        assert det.detect_device(*args, 0.5) == before
        pixels, counts = det.redact_device(*args, faces, spec=dict(blur=3))
        assert list(counts) == [len(f) for f in faces] and pixels[0].sum() > 0 and not np.array_equal(dev[0].cpu().numpy(), crop448)
    finally:
        trk.close()


# ---------------------------------------------------------------------------------------------- 5. the C++ class
def test_cpp_class_detect_redacted_with_blur(rfa, base_frame, tmp_path):
    src = os.path.join(ROOT, "tests", "csrc", "test_redact_blur.cpp")
    exe = str(tmp_path / "test_redact_blur")
    lib_dir = os.path.dirname(rfa.lib_path())
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DRF_NO_OPENCV", "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                           "-L" + lib_dir, "-lretinaface_amd", "-Wl,-rpath," + lib_dir])
    wins = [np.ascontiguousarray(base_frame[30 + 2 * t:478 + 2 * t, 380 + 8 * t:828 + 8 * t]) for t in range(3)]
    raw, out = str(tmp_path / "frames.raw"), str(tmp_path / "out.bin")
    np.stack(wins).tofile(raw)
    r = subprocess.run([exe, ASSETS, "mnet25", "448", "448", raw, "3", "0.5", "3", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    blob = open(out, "rb").read()
    det = engine(rfa)
    work = [w.copy() for w in wins]
    dets = det.detect_redacted(work, 0.5, spec=dict(blur=3))
    fb = 448 * 448 * 3
    pos = 3 * fb
    sp = rb.Spec(default_regions=MD, blur=3)
    for i in range(3):
        assert blob[i * fb:(i + 1) * fb] == work[i].tobytes(), i
        assert work[i].tobytes() == rb.redact_image(sp, wins[i], rows_of(dets[i]), 1.0)[0].tobytes()
        k = int(np.frombuffer(blob, np.int32, 1, pos)[0])
        assert k == len(dets[i]) and np.frombuffer(blob, np.int32, k, pos + 4).tobytes() == det.last_pixels[i, :k].tobytes()
        pos += 4 + 4 * k
    assert pos == len(blob)
