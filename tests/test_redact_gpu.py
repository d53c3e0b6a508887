"""Face redaction on the GPU: the three redaction kernels against tests/redact_ref.py byte for byte on constructed faces (no forward
pass) -- whole frames, the bytes around a view, pixel counts and region counts -- with a tracker's coasting tracks, then the fused
calls against their own parts (rf_detect_batch_device + the reference fed with its result), the tracked form, the refusals and the
C++ class."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import redact_ref as rr
import track_ref as tr
from conftest import ASSETS, ROOT
from test_gpu_align import FP16, engine, rfa, rows_of, to_device  # noqa: F401  (rfa: fixture)
from test_redact_host import BIG, face_at, noise, seeded_faces, views
from test_tile_gpu import INT8, SPLIT2, SPLIT3, split_engine
from test_track_gpu import check_update
from test_track_host import by_score, face

pytestmark = pytest.mark.gpu
f32 = np.float32
MD = 256


class DevView:
    """a numpy frame (any view) in device memory with the view's layout: ptr and step address the view inside a copy of its base"""

    def __init__(self, frame):
        import torch
        self.frame = frame
        self.base = frame.base if frame.base is not None else frame
        self.off = frame.ctypes.data - self.base.ctypes.data
        self.t = torch.from_numpy(np.array(self.base, copy=True).reshape(-1)).cuda()
        self.ptr, self.rows, self.cols, self.step = self.t.data_ptr() + self.off, frame.shape[0], frame.shape[1], frame.strides[0]

    def read(self):
        """(the view, the whole base) as they are on the device now"""
        flat = self.t.cpu().numpy()
        return np.lib.stride_tricks.as_strided(flat[self.off:], self.frame.shape, self.frame.strides), flat.reshape(self.base.shape)


def check_device(det, frames, per_image, scales=None, tracker=None, streams=None, tables=None, max_missed=0, **spec):
    """one rf_redact_device call against the reference.  frames: numpy views or None; tables: per image the track_ref table whose
    coasting tracks join the list, or None"""
    import torch
    n = len(frames)
    dev = [DevView(f) if f is not None else None for f in frames]
    torch.cuda.synchronize()
    pixels, counts = det.redact_device([d.ptr if d else 0 for d in dev], [d.rows if d else 0 for d in dev], [d.cols if d else 0 for d in dev],
                                       per_image, steps=[d.step if d else 0 for d in dev], coord_scale=scales, spec=spec, tracker=tracker,
                                       streams=streams)
    sp = rr.Spec(default_regions=MD, **spec)
    assert pixels.shape == (n, sp.max_regions)
    cut = False
    outs = []
    for i, f in enumerate(frames):
        want, wpx, true = rr.redact_image(sp, f, per_image[i], 1.0 if scales is None else scales[i], tables[i] if tables else None, max_missed)
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
@pytest.mark.parametrize("mode", (rr.PIXELATE, rr.FILL))
def test_host_shapes_in_one_call_equal_the_reference(rfa, shape, mode):
    """three frames of different sizes and layouts (a padded step, 1 x 1, an ROI view at an odd pointer) and a NULL frame in one call"""
    det = engine(rfa)
    frames = list(views().values()) + [None]
    for cells in (1, 2, 8, 64):
        rng = np.random.default_rng(cells)
        per_image = [seeded_faces(rng, f.shape[0], f.shape[1], k) for f, k in zip(frames[:3], (5, 2, 7))] + [face_at(1.0, 1.0, 9.0, 9.0)[None]]
        outs, pixels, counts = check_device(det, frames, per_image, mode=mode, shape=shape, cells=cells, fill=(9, 200, 31))
        assert counts[3] == 0 and not pixels[3].any()
        if cells == 1 and mode == rr.PIXELATE:
            continue
        assert not np.array_equal(outs[0], frames[0])
    # cells at least the region's longer side: c = 1, pixelation is the identity, and the pixels are still owned
    small = [np.stack([face_at(10.0, 10.0, 15.0, 14.0), face_at(30.0, 20.0, 33.0, 40.0)])]
    outs, pixels, _ = check_device(det, frames[:1], small, mode=rr.PIXELATE, shape=shape, cells=64)
    assert np.array_equal(outs[0], frames[0]) and pixels[0, 0] > 0 and pixels[0, 1] > 0
    # a coordinate scale per image
    check_device(det, frames[:3], [face_at(-3.0, -2.0, f.shape[1] / 2.0, f.shape[0] / 2.0)[None] for f in frames[:3]], scales=[BIG, 1.0, BIG],
                 mode=mode, shape=shape)


@pytest.mark.parametrize("shape", (rr.RECT, rr.ELLIPSE))
def test_a_region_that_covers_a_large_frame(rfa, shape):
    """1280 x 896, one region larger than the frame on every side (cells of 200 x 200 pixels split over workgroups by cell row, the clip
    on all four sides), small faces behind it in the list that own nothing inside a rectangle, something inside an ellipse's corners"""
    det = engine(rfa)
    frame = noise(896, 1280, 3)
    faces = np.concatenate([face_at(-100.0, -60.0, 1400.0, 950.0)[None], seeded_faces(np.random.default_rng(4), 896, 1280, 3),
                            face_at(2.0, 2.0, 60.0, 50.0)[None]])
    outs, pixels, _ = check_device(det, [frame], [faces], shape=shape, margin=-1.0)
    if shape == rr.RECT:
        assert pixels[0, 0] == 896 * 1280 and not pixels[0, 1:].any()
    else:
        assert 0 < pixels[0, 0] < 896 * 1280 and pixels[0, 4] > 0
    check_device(det, [frame], [faces[:1]], shape=shape, mode=rr.FILL, fill=(1, 2, 3))


def grid_faces(rng, count, rows, cols):
    """`count` small boxes, many of them overlapping their neighbours"""
    out = [face_at(x, y, x + rng.uniform(2, 14), y + rng.uniform(2, 14), 1.0 - k / 4096.0)
           for k, (x, y) in enumerate(zip(rng.uniform(-4, cols, count), rng.uniform(-4, rows, count)))]
    return np.stack(out) if out else np.zeros((0, 15), f32)


def test_region_counts_up_to_the_cap_and_beyond(rfa):
    det = engine(rfa)
    rng = np.random.default_rng(9)
    counts = (0, 1, 64, 65, 256, 1024)
    frames = [noise(96, 128, 10 + i) for i in range(len(counts))]
    per_image = [grid_faces(rng, k, 96, 128) for k in counts]
    for shape in (rr.RECT, rr.ELLIPSE):
        _, pixels, got = check_device(det, frames, per_image, shape=shape, cells=4, max_regions=1024)
        assert list(got) == list(counts) and not det.truncated
        assert (pixels[5] > 0).sum() > 200
    # 1025 faces: the list is cut at 1024, the count stays true
    more = grid_faces(rng, 1025, 96, 128)
    _, _, got = check_device(det, frames[:2], [more, per_image[1]], cells=4, max_regions=1024)
    assert list(got) == [1025, 1] and det.truncated
    # the default cap is the engine's max_detections
    _, _, got = check_device(det, frames[:1], [per_image[5][:300]], cells=2)
    assert got[0] == 300 and det.truncated


@pytest.mark.parametrize("shape", (rr.RECT, rr.ELLIPSE))
def test_a_chain_of_64_mutually_overlapping_regions(rfa, shape):
    det = engine(rfa)
    frame = noise(120, 160, 21)
    chain = np.stack([face_at(10.0 + k, 8.0 + 0.5 * k, 70.0 + k, 60.0 + 0.5 * k, 0.99 - 0.01 * k) for k in range(64)])
    _, pixels, _ = check_device(det, [frame], [chain], shape=shape, margin=-1.0, cells=5)
    assert (pixels[0, :64] > 0).all() and pixels[0, 0] > 10 * pixels[0, 1]                     # every later region owns its sliver only
    _, pixels, _ = check_device(det, [frame], [chain[::-1].copy()], shape=shape, margin=-1.0, mode=rr.FILL, fill=(0, 255, 0))
    assert (pixels[0, :64] > 0).all()


def test_a_repeated_call_gives_the_same_bytes(rfa):
    det = engine(rfa)
    frames = [noise(96, 128, 31), noise(200, 90, 32)]
    rng = np.random.default_rng(33)
    per_image = [grid_faces(rng, 80, 96, 128), seeded_faces(rng, 200, 90, 9)]
    a = check_device(det, frames, per_image, shape=rr.ELLIPSE, cells=3)
    b = check_device(det, frames, per_image, shape=rr.ELLIPSE, cells=3)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[0], b[0])) and a[1].tobytes() == b[1].tobytes()


# ---------------------------------------------------------------------------------------------- 2. coasting tracks
def test_coasting_tracks_are_redacted_where_they_were_last_seen(rfa):
    det = engine(rfa)
    kw = dict(max_tracks=65, max_missed=3)
    trk = det.tracker(2, **kw)
    ref = [tr.Stream(tr.Spec(**kw)) for _ in range(2)]
    people = [face(0.9, 10, 10, 30), face(0.8, 60, 20, 24), face(0.7, 100, 50, 20), face(0.6, 20, 60, 28)]
    try:
        # stream 0: four tracks open; then person 1 misses three frames, person 3 two, person 2 one; stream 1: one track that misses one
        seq0 = [[0, 1, 2, 3], [0, 2, 3], [0, 2], [0]]
        for t, who in enumerate(seq0):
            check_update(trk, ref, [0, 1], [by_score([people[p] for p in who]), by_score([people[2]]) if t < 3 else np.zeros(0, tr.FACE)], cap_ended=4)
        missed = sorted(int(m) for m in ref[0].table["missed"][ref[0].table["id"] != 0])
        assert missed == [0, 1, 2, 3] and int(ref[1].table["missed"][0]) == 1
        frames = [noise(96, 128, 40), noise(96, 128, 41), noise(96, 128, 42)]
        seen = [by_score([people[0]]), np.zeros((0, 15), f32), by_score([people[1]])]
        tables = [ref[0].table, ref[1].table, None]
        for coast, extra in ((0, 3), (-1, 0), (1, 1), (2, 2)):
            outs, pixels, counts = check_device(det, frames, seen, tracker=trk, streams=[0, 1, -1], tables=tables, max_missed=3, coast=coast,
                                                mode=rr.FILL, fill=(0, 0, 255))
            assert list(counts) == [1 + extra, 1 if coast >= 0 else 0, 1]
        # pixelate + ellipse, the streams the other way round, and a NULL frame on a stream with coasting tracks
        check_device(det, [frames[0], None, frames[2]], [seen[1], seen[0], seen[0]], tracker=trk, streams=[1, 0, -1],
                     tables=[ref[1].table, ref[0].table, None], max_missed=3, shape=rr.ELLIPSE)
        # the tables are what they were: redaction only reads them
        for s in range(2):
            assert trk.read(s)[0].tobytes() == ref[s].table.tobytes()
        # a stream twice in one call is refused
        d = [DevView(f) for f in frames[:2]]
        with pytest.raises(rfa.RFError) as e:
            det.redact_device([v.ptr for v in d], [96, 96], [128, 128], seen[:2], tracker=trk, streams=[0, 0])
        assert e.value.status == -1
        with pytest.raises(rfa.RFError):
            det.redact_device([v.ptr for v in d], [96, 96], [128, 128], seen[:2], tracker=trk, streams=[0, 2])
        assert all(np.array_equal(v.read()[0], f) for v, f in zip(d, frames))
    finally:
        trk.close()


# ---------------------------------------------------------------------------------------------- 3. the fused calls
def check_fused(det, frames, spec, host=False):
    """rf_detect_redact_batch[_device] against rf_detect_batch_device on untouched copies + the reference on its result"""
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
    sp = rr.Spec(default_regions=MD, **spec)
    total = 0
    for i, f in enumerate(frames):
        if f is None:
            assert not det.last_pixels[i].any()
            continue
        want, wpx, _ = rr.redact_image(sp, f, rows_of(plain[i]), det.frame_scale(rows[i], cols[i]))
        assert outs[i].tobytes() == want.tobytes(), (i, int((outs[i] != want).any(2).sum()))
        assert det.last_pixels[i].tobytes() == wpx.tobytes(), i
        total += int(wpx.sum())
    # the plain call is what it was, and the untouched copies are untouched
    assert det.detect_device([d.data_ptr() if d is not None else 0 for d in pd], rows, cols, 0.5) == plain
    assert all(np.array_equal(d.cpu().numpy(), f) for d, f in zip(pd, frames) if f is not None)
    return plain, total


@pytest.mark.parametrize("prec,kw", ((FP16, {}), (FP16, SPLIT2), (FP16, SPLIT3), (INT8, {})))
def test_fused_call_equals_detection_plus_the_reference(rfa, base_frame, crop448, prec, kw):
    """SPLIT2 / SPLIT3: the 20 frames of the call ride on launches of 8, 8 and 4 images on different lanes"""
    det = split_engine(rfa, kw, prec=prec)
    wins = [np.ascontiguousarray(base_frame[30 + t:478 + t, 380 + 4 * t:828 + 4 * t]) for t in range(20)]
    plain, total = check_fused(det, wins, dict(shape=rr.ELLIPSE))
    assert all(len(p) >= 1 for p in plain) and total > 20 * 400
    if kw:
        return
    # a NULL frame and an oversize frame, which is redacted at its full resolution
    plain, total = check_fused(det, [crop448, None, base_frame, wins[3]], dict(cells=6))
    assert len(plain[2]) >= 2 and len(plain[1]) == 0
    if prec != FP16:
        return
    check_fused(det, [crop448, None, base_frame], dict(mode=rr.FILL, fill=(255, 255, 255)), host=True)
    check_fused(det, wins[:3], {}, host=True)


def test_tracked_call_keeps_a_missed_face_covered(rfa, crop448):
    """frames 0, 1 and 3 are the fixture crop, frame 2 is grey: the detector finds nothing there, the tracks coast and their regions are
    redacted where the faces were last seen.  Tags and tables are those of the unredacted tracked call on a second tracker."""
    import torch
    det = engine(rfa)
    grey = np.full_like(crop448, 128)
    seq = [crop448, crop448, grey, crop448]
    a, b = det.tracker(1), det.tracker(1)
    spec = dict(mode=rr.FILL, fill=(0, 0, 0), shape=rr.ELLIPSE)
    sp = rr.Spec(default_regions=MD, **spec)
    try:
        for t, f in enumerate(seq):
            work, keep = to_device([f, f])
            got, tags, ended = a.detect_redacted_device([work.data_ptr()], [448], [448], [0], 0.5, spec=spec)
            torch.cuda.synchronize()
            want, wtags, wended = det.detect_tracked_device([keep.data_ptr()], [448], [448], b, [0], 0.5)
            assert got == want and a.last_tags.tobytes() == b.last_tags.tobytes() and a.last_ended_counts.tobytes() == b.last_ended_counts.tobytes()
            table = b.read(0)[0]
            assert a.read(0)[0].tobytes() == table.tobytes() and a.read(0)[1:] == b.read(0)[1:]
            ref_out, wpx, true = rr.redact_image(sp, f, rows_of(want[0]), 1.0, table, 10)
            out = work.cpu().numpy()
            assert out.tobytes() == ref_out.tobytes(), (t, int((out != ref_out).any(2).sum()))
            assert a.last_pixels[0].tobytes() == wpx.tobytes() and a.last_region_counts[0] == true
            if t == 1:
                n_faces = len(want[0])
                assert n_faces >= 1 and true == n_faces
            if t == 2:
                assert len(want[0]) == 0 and true == n_faces and int(wpx.sum()) > 400 * n_faces      # the coasting regions
                assert not np.array_equal(out, grey)
            if t == 3:
                assert true == n_faces                                                               # matched again: nothing coasts
        # coast < 0: no coasting regions; the grey frame stays grey
        work = to_device([grey])[0]
        a.detect_redacted_device([work.data_ptr()], [448], [448], [0], 0.5, spec=dict(coast=-1))
        torch.cuda.synchronize()
        assert np.array_equal(work.cpu().numpy(), grey) and a.last_region_counts[0] == 0
        # a stream twice in one call is refused before the tracker changes
        state = a.read(0)[0].tobytes()
        two = to_device([crop448, crop448])
        with pytest.raises(rfa.RFError) as e:
            a.detect_redacted_device([d.data_ptr() for d in two], [448] * 2, [448] * 2, [0, 0], 0.5)
        assert e.value.status == -1 and a.read(0)[0].tobytes() == state
        assert all(np.array_equal(d.cpu().numpy(), crop448) for d in two)
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_leave_frames_and_handle_usable(rfa, crop448):
    det = engine(rfa)
    dev = to_device([crop448, crop448])
    args = ([d.data_ptr() for d in dev], [448, 448], [448, 448])
    before = det.detect_device(*args, 0.5)
    faces = [rows_of(before[0]), rows_of(before[1])]
    bad = [dict(mode=2), dict(shape=-1), dict(cells=65), dict(margin=1.5), dict(margin=float("nan")), dict(max_regions=1025)]
    for kw in bad:
        for call in (lambda: det.redact_device(*args, faces, spec=kw), lambda: det.detect_redacted_device(*args, 0.5, spec=kw),
                     lambda: det.detect_redacted([crop448.copy()], 0.5, spec=kw)):
            with pytest.raises(rfa.RFError) as e:
                call()
            assert e.value.status == -1, kw
    sp = rfa.redact_spec()
    sp.struct_size = 24
    with pytest.raises(rfa.RFError):
        det.redact_device(*args, faces, spec=sp)
    # two frames of the call that share bytes: the same frame twice, and a view that starts inside the other
    same = ([dev[0].data_ptr()] * 2, [448, 448], [448, 448])
    inside = ([dev[0].data_ptr(), dev[0].data_ptr() + 448 * 3 * 100], [448, 200], [448, 448])
    for a in (same, inside):
        for call in (lambda: det.redact_device(*a, faces), lambda: det.detect_redacted_device(*a, 0.5)):
            with pytest.raises(rfa.RFError) as e:
                call()
            assert e.value.status == -1
    # a NULL frame array, more faces than cap_per_image
    lib = rfa.load_library()
    n2 = (C.c_int * 2)(448, 448)
    cnt = (C.c_int * 2)(1, 1)
    one = (rfa._lib.rf_face * 2)()
    assert lib.rf_redact_device(det._h, None, n2, n2, None, 2, one, 1, cnt, None, None, None, None, None, None) == -1
    assert lib.rf_detect_redact_batch_device(det._h, None, n2, n2, None, 2, 0.5, one, 1, cnt, None, None) == -1
    cnt[0] = 2
    p = (C.c_void_p * 2)(*args[0])
    assert lib.rf_redact_device(det._h, p, n2, n2, None, 2, one, 1, cnt, None, None, None, None, None, None) == -1
    # nothing was written, the handle works
    assert all(np.array_equal(d.cpu().numpy(), crop448) for d in dev)
    assert det.detect_device(*args, 0.5) == before
    pixels, counts = det.redact_device(*args, faces)
    assert list(counts) == [len(f) for f in faces] and pixels[0].sum() > 0 and not np.array_equal(dev[0].cpu().numpy(), crop448)


def test_multi_device_handles_refuse_redaction(rfa, crop448):
    det = rfa.RetinaFace(ASSETS, "net3", 0.4, precision=FP16, net_hw=(448, 448), model_stem="mnet25", devices=[0, 0])
    try:
        dev = to_device([crop448])[0]
        for call in (lambda: det.redact_device([dev.data_ptr()], [448], [448], [face_at(10.0, 10.0, 90.0, 90.0)[None]]),
                     lambda: det.detect_redacted_device([dev.data_ptr()], [448], [448], 0.5),
                     lambda: det.detect_redacted([crop448.copy()], 0.5)):
            with pytest.raises(rfa.RFError) as e:
                call()
            assert e.value.status == -5
        assert np.array_equal(dev.cpu().numpy(), crop448)
    finally:
        det.close()


# ---------------------------------------------------------------------------------------------- 5. the C++ class
def test_cpp_class_detect_redacted(rfa, base_frame, tmp_path):
    src = os.path.join(ROOT, "tests", "csrc", "test_redact.cpp")
    exe = str(tmp_path / "test_redact")
    lib_dir = os.path.dirname(rfa.lib_path())
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DRF_NO_OPENCV", "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                           "-L" + lib_dir, "-lretinaface_amd", "-Wl,-rpath," + lib_dir])
    wins = [np.ascontiguousarray(base_frame[30 + 2 * t:478 + 2 * t, 380 + 8 * t:828 + 8 * t]) for t in range(3)]
    raw, out = str(tmp_path / "frames.raw"), str(tmp_path / "out.bin")
    np.stack(wins).tofile(raw)
    r = subprocess.run([exe, ASSETS, "mnet25", "448", "448", raw, "3", "0.5", "1", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    blob = open(out, "rb").read()
    det = engine(rfa)
    work = [w.copy() for w in wins]
    dets = det.detect_redacted(work, 0.5, spec=dict(shape=rr.ELLIPSE))
    fb = 448 * 448 * 3
    pos = 3 * fb
    for i in range(3):
        assert blob[i * fb:(i + 1) * fb] == work[i].tobytes(), i
        assert not np.array_equal(work[i], wins[i])
        k = int(np.frombuffer(blob, np.int32, 1, pos)[0])
        assert k == len(dets[i]) and np.frombuffer(blob, np.int32, k, pos + 4).tobytes() == det.last_pixels[i, :k].tobytes()
        pos += 4 + 4 * k
    assert pos == len(blob)
