"""Face quality on the GPU: every record, and the tensor, matrices and offsets of every quality-gated face batch, must equal
tests/face_quality_ref.py byte for byte -- the standalone records call, the accumulator widths, the gated standalone batch, the gated
fused call (whose detections must be the bytes rf_detect_batch_device returns) across the launches of one call, the NULL gate
(the ungated call's bytes), the capacity cut, oversize frames, and the C++ class."""
import os
import subprocess

import numpy as np
import pytest

import face_batch_ref as fbr
import face_quality_ref as fqr
from conftest import ASSETS, ROOT, golden
from test_gpu_align import FP16, FP32, _template_face, engine, rfa, rows_of, to_device  # noqa: F401  (rfa: fixture)

pytestmark = pytest.mark.gpu

ES = {"u8": 1, "f16": 2, "f32": 4}


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_records(got, want):
    """per image: the considered records, byte for byte"""
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == fqr.DTYPE and len(g) == len(w), (i, len(g), len(w))
        for k in range(len(w)):
            assert g[k].tobytes() == w[k].tobytes(), (i, k, g[k], w[k])
    return True


def between(values, lo):
    """the midpoint of sorted values[lo] and values[lo + 1], which must differ"""
    v = sorted(float(x) for x in values)
    assert v[lo] < v[lo + 1]
    return (v[lo] + v[lo + 1]) / 2


# ---------------------------------------------------------------------------------------------- 1. standalone records
def test_standalone_records_over_borders_rotations_and_invalid_faces(rfa):
    import torch
    rng = np.random.default_rng(11)
    H, W = 211, 317
    frame = rng.integers(1, 256, size=(H, W, 3), dtype=np.uint8)
    det = engine(rfa)
    dev = to_device([frame])[0]
    step = W * 3 + 14                                                      # the same frame as an ROI: odd pointer, odd step (965)
    wide = torch.zeros((H + 1, step), dtype=torch.uint8, device="cuda")
    wide.view(-1)[1:1 + H * step].view(H, step)[:, :W * 3] = dev.view(H, W * 3)
    torch.cuda.synchronize()
    assert (wide.data_ptr() + 1) % 2 == 1 and step % 2 == 1
    for size in (16, 17, 112):
        faces = [_template_face(size, 1.0, 0.0, ox, oy) for ox in (-40.0, 100.5, W - 60.0) for oy in (-50.0, 60.25, H - 30.0)]
        faces += [_template_face(size, 1.7, 0.6, -30.0, 90.0), _template_face(size, 0.4, -2.5, W - 10.0, H - 5.0),
                  _template_face(size, 1.0, 0.0, -1.5, -1.5), _template_face(size, 1.0, 0.0, W - size + 0.75, H - size + 0.75)]
        same_pt = np.zeros(15, np.float32)
        same_pt[5:10], same_pt[10:15] = 100.0, 80.0
        nan = faces[4].copy()
        nan[8] = np.nan
        faces += [_template_face(size, 1.0, 0.0, -5000.0, 40.0), same_pt, nan]
        faces = np.array(faces, np.float32)
        n = len(faces)
        want = fqr.records([frame], [faces], None, size=size)
        got = det.face_quality([dev.data_ptr()], [H], [W], [faces], crop_size=size)
        assert same_records(got, want), size
        w = want[0]
        assert (w["covered"][:n - 3] < size * size).sum() >= 6 and w["covered"][4] > 0           # an edge on every side
        assert w["covered"][n - 3] == 0 and w["sum_luma"][n - 3] == 0 and w["sum_lap2"][n - 3] == 0 and w["iod2"][n - 3] > 0   # outside: valid
        assert not any(w[k].tobytes().strip(b"\0") for k in (n - 2, n - 1))                      # invalid, no gate: all zero
        # under a gate the invalid faces carry RF_GATE_INVALID and whatever their zeros fail
        gate = dict(min_covered=0.5, min_sharpness=1.0)
        want = fqr.records([frame], [faces], gate, size=size)
        assert want[0]["flags"][n - 1] == fqr.INVALID | fqr.COVERED | fqr.SHARPNESS and (want[0]["flags"] == 0).any()
        assert same_records(det.face_quality([dev.data_ptr()], [H], [W], [faces], crop_size=size, gate=gate), want), size
        got = det.face_quality([wide.data_ptr() + 1], [H], [W], [faces], steps=[step], crop_size=size, gate=gate)
        assert same_records(got, want), size
        # max_faces below the count: only the first records exist
        assert same_records(det.face_quality([dev.data_ptr()], [H], [W], [faces], crop_size=size, gate=gate, max_faces=5), [want[0][:5]])


# ---------------------------------------------------------------------------------------------- 2. accumulator width
def test_checkerboard_sums_need_more_than_32_bits(rfa):
    board = (((np.arange(640)[:, None] + np.arange(640)[None, :]) & 1) * 255).astype(np.uint8)
    frame = np.ascontiguousarray(np.repeat(board[:, :, None], 3, axis=2))
    flat = np.full((640, 640, 3), 93, np.uint8)
    det = engine(rfa)
    dev, dflat = to_device([frame, flat])
    for size, lap, lap2 in ((16, 0, 203918400), (17, -1020, 234090000), (512, 0, 270608040000)):
        face = _template_face(size, 1.0, 0.0, 64.0, 64.0)
        want = fqr.quality(frame, face, 1.0, size)
        want["flags"] = 0
        assert int(want["sum_lap"]) == lap and int(want["sum_lap2"]) == lap2 and int(want["covered"]) == size * size
        assert int(want["sum_luma"]) == 255 * (size * size // 2)
        if size == 512:
            assert int(want["sum_lap2"]) > 2 ** 32
        got = det.face_quality([dev.data_ptr()], [640], [640], [[face]], crop_size=size)
        assert got[0][0].tobytes() == want.tobytes(), (size, got[0][0], want)
        got = det.face_quality([dflat.data_ptr()], [640], [640], [[face]], crop_size=size)[0][0]
        assert got["sharpness"].tobytes() == np.float64(0.0).tobytes() and got["sum_lap"] == 0 and got["sum_lap2"] == 0
        assert got["sum_luma"] == 93 * size * size and got["covered"] == size * size


# ---------------------------------------------------------------------------------------------- 3. gated standalone batch
_ref_cache = {}


def _golden_records(base_frame, cols):
    if cols not in _ref_cache:
        faces = golden("fixture_mnet25.npz")["det"]
        _ref_cache[cols] = fqr.records([base_frame[:, :cols]], [faces], None, size=112)[0]
    return _ref_cache[cols]


def _gates(base_frame, cut):
    """(name, gate, frame columns): one gate per flag bit and one combination, thresholds between two adjacent reference values"""
    q = _golden_records(base_frame, 1280)
    qc = _golden_records(base_frame, cut)
    area = 112.0 * 112.0
    return [("sharpness", dict(min_sharpness=between(q["sharpness"], 2)), 1280),
            ("iod", dict(min_iod=float(np.sqrt(between(q["iod2"], 1)))), 1280),
            ("yaw", dict(max_abs_yaw=between(np.abs(q["yaw"]), 3)), 1280),
            ("roll", dict(max_sin2_roll=between(q["sin2_roll"], 2)), 1280),
            ("covered", dict(min_covered=between(sorted(set(qc["covered"] / area)), 0)), cut),
            ("dark", dict(min_luma=between(q["sum_luma"] / area, 1)), 1280),
            ("bright", dict(max_luma=between(q["sum_luma"] / area, 3)), 1280),
            ("sharpness+yaw", dict(min_sharpness=between(q["sharpness"], 0), max_abs_yaw=between(np.abs(q["yaw"]), 4)), 1280)]


@pytest.mark.parametrize("dtype", ("u8", "f16", "f32"))
def test_gated_standalone_batch_on_the_golden_detections(rfa, base_frame, dtype):
    import torch
    det = engine(rfa)
    faces = golden("fixture_mnet25.npz")["det"]
    dev = to_device([base_frame])[0]
    cut = int(np.sort(faces[:, 7])[2]) + 1                                 # a frame that ends at the third nose: faces right of it lose cover
    es, size = ES[dtype], 112
    fb = 3 * size * size * es
    seen = 0
    for name, gate, cols in _gates(base_frame, cut):
        frame = base_frame[:, :cols]
        for rgb in (0, 1):
            want_t, want_m, want_o, want_q = fqr.gated_batch([frame], [faces], fbr.FORMAT_OF[dtype], gate, size=size, rgb=rgb)
            kept = int(want_o[1])
            assert 1 <= kept <= len(faces) - 1, (name, kept)               # the reference keeps one at least and drops one at least
            seen |= int(np.bitwise_or.reduce(want_q[0]["flags"]))
            buf = torch.full((len(faces) * fb + 64,), 77, dtype=torch.uint8, device="cuda")
            d_out = buf.data_ptr() + es                                    # one element into the canary: no band starts 16-aligned
            _, t, m, off, q = det.face_batch([dev.data_ptr()], [896], [cols], [faces], steps=[1280 * 3], crop_size=size, dtype=dtype,
                                             rgb=bool(rgb), capacity=len(faces), d_out=d_out, gate=gate, return_quality=True)
            torch.cuda.synchronize()
            assert list(off) == list(want_o) and same_records(q, want_q), (name, rgb)
            assert same(t, want_t) and np.array_equal(m.reshape(-1, 6), want_m), (name, rgb)
            got = buf.cpu().numpy()
            assert got[es:es + kept * fb].tobytes() == want_t.tobytes(), (name, rgb)             # device output = host output
            assert (got[:es] == 77).all() and (got[es + kept * fb:] == 77).all()                 # nothing beyond the kept faces
            assert not det.faces_truncated
    assert seen == fqr.SHARPNESS | fqr.IOD | fqr.YAW | fqr.ROLL | fqr.COVERED | fqr.DARK | fqr.BRIGHT


# ---------------------------------------------------------------------------------------------- 4. NULL gate = ungated
def test_null_gate_gives_the_bytes_of_the_ungated_call(rfa):
    from retinaface_amd.frames import synth_frames
    frames = synth_frames(448, 448, 8, config=1)
    det = engine(rfa)
    dev = to_device(frames)
    ptrs = [t.data_ptr() for t in dev]
    for dtype, kw in (("f16", {}), ("u8", dict(rgb=False, max_faces=2))):
        plain = det.detect_face_batch_device(ptrs, [448] * 8, [448] * 8, 0.5, dtype=dtype, **kw)
        dets, t, m, off, q = det.detect_face_batch_device(ptrs, [448] * 8, [448] * 8, 0.5, dtype=dtype, return_quality=True, **kw)
        assert dets == plain[0] == det.detect_device(ptrs, [448] * 8, [448] * 8, 0.5)
        assert len(t) >= 8 and same(t, plain[1]) and np.array_equal(m, plain[2]) and list(off) == list(plain[3])
        mf = kw.get("max_faces", 256)
        want_q = fqr.records(frames, [rows_of(d) for d in dets], None, max_faces=mf)
        assert same_records(q, want_q) and all((r["flags"] == 0).all() for r in q)
        assert sum(len(r) for r in q) == int(off[8])


# ---------------------------------------------------------------------------------------------- 5. fused, across launches
@pytest.mark.parametrize("kw", ({}, {"coalesce": 1, "lanes": 2}))
def test_gated_fused_call_across_the_launches_of_a_call(rfa, kw):
    from retinaface_amd.frames import synth_frames
    frames = synth_frames(448, 448, 19, config=2)
    frames[7] = np.full((448, 448, 3), 128, np.uint8)
    frames[9] = None
    det = engine(rfa, max_batch=8, **kw)
    plain = det.detectBatchImages(frames, 0.5)
    rows = [rows_of(d) for d in plain]
    ungated = fqr.records(frames, rows, None, size=96, max_faces=3)
    sharp = np.concatenate([r["sharpness"] for r in ungated])
    total = len(sharp)
    gate = dict(min_sharpness=float(np.float32(np.median(sharp))))
    want_t, want_m, want_o, want_q = fqr.gated_batch(frames, rows, fbr.F16_CHW, gate, size=96, rgb=1, max_faces=3)
    assert total >= 17 and 1 <= int(want_o[19]) <= total - 1               # the reference keeps some and drops some
    # host frames: rf_detect_face_batch_gated
    dets, t, m, off, q = det.detect_face_batch(frames, 0.5, dtype="f16", crop_size=96, max_faces=3, gate=gate, return_quality=True)
    assert dets == plain and len(dets[7]) == 0 and len(dets[9]) == 0 and max(len(d) for d in dets) >= 3
    assert list(off) == list(want_o) and off[8] == off[7] and off[10] == off[9] and same_records(q, want_q)
    assert same(t, want_t) and np.array_equal(m.reshape(-1, 6), want_m)
    # device frames over the frames that exist: the same faces, and the detections of rf_detect_batch_device
    real = [i for i, f in enumerate(frames) if f is not None]
    dev = to_device([frames[i] for i in real])
    ptrs = [x.data_ptr() for x in dev]
    dd, dt, dm, do, dq = det.detect_face_batch_device(ptrs, [448] * 18, [448] * 18, 0.5, dtype="f16", crop_size=96, max_faces=3, gate=gate,
                                                      return_quality=True)
    assert dd == det.detect_device(ptrs, [448] * 18, [448] * 18, 0.5) == [plain[i] for i in real]
    assert same(dt, t) and np.array_equal(dm, m) and do[18] == off[19] and same_records(dq, [want_q[i] for i in real])
    # a capacity cut inside an image: RF_ERR_TRUNCATED, the true offsets, the first `capacity` kept faces
    inside = next(i for i in range(19) if want_o[i + 1] - want_o[i] >= 2)
    cap = int(want_o[inside]) + 1
    assert 1 <= cap < int(want_o[19])
    cd, ct, cm, co = det.detect_face_batch(frames, 0.5, dtype="f16", crop_size=96, max_faces=3, gate=gate, capacity=cap)
    assert det.faces_truncated and det.truncated and cd == plain and list(co) == list(want_o)
    assert len(ct) == cap and same(ct, want_t[:cap]) and np.array_equal(cm.reshape(-1, 6), want_m[:cap])
    assert det.detectBatchImages(frames, 0.5) == plain and not det.truncated


def test_gated_oversize_frames_are_sampled_at_full_resolution(rfa, base_frame, crop448):
    det = engine(rfa)
    frames = [base_frame, crop448]
    dev = to_device(frames)
    ptrs, rows, cols = [t.data_ptr() for t in dev], [896, 448], [1280, 448]
    plain = det.detect_device(ptrs, rows, cols, 0.5)
    scales = [det.frame_scale(896, 1280), det.frame_scale(448, 448)]
    assert scales[0] == float(np.float32(1280) / np.float32(448)) and scales[1] == 1.0
    faces = [rows_of(d) for d in plain]
    ungated = fqr.records(frames, faces, None, scales=scales)
    gate = dict(min_iod=float(np.sqrt(between(np.concatenate([r["iod2"] for r in ungated]), 1))))
    want_t, want_m, want_o, want_q = fqr.gated_batch(frames, faces, fbr.F32_CHW, gate, rgb=1, scales=scales)
    assert 1 <= int(want_o[2]) < sum(len(f) for f in faces) and len(plain[0]) >= 3
    dets, t, m, off, q = det.detect_face_batch_device(ptrs, rows, cols, 0.5, dtype="f32", gate=gate, return_quality=True)
    assert dets == plain and list(off) == list(want_o) and same_records(q, want_q)
    assert same(t, want_t) and np.array_equal(m.reshape(-1, 6), want_m)
    hd, ht, hm, ho, hq = det.detect_face_batch(frames, 0.5, dtype="f32", gate=gate, return_quality=True)      # host frames: the same path
    assert hd == dets and same(ht, t) and np.array_equal(hm, m) and list(ho) == list(off) and same_records(hq, want_q)


# ---------------------------------------------------------------------------------------------- 6. determinism, non-interference
def test_gated_calls_are_deterministic_and_leave_the_other_paths_alone(rfa):
    from retinaface_amd.frames import synth_frames
    frames = synth_frames(448, 448, 8, config=3)
    det = engine(rfa)
    dev = to_device(frames)
    ptrs = [t.data_ptr() for t in dev]
    args = (ptrs, [448] * 8, [448] * 8, 0.5)
    before = det.wait(det.enqueue_device(*args), 8)
    ungated = det.detect_face_batch_device(*args)
    probe = det.detect_face_batch_device(*args, return_quality=True)[4]
    gate = dict(min_sharpness=float(np.float32(np.median(np.concatenate([r["sharpness"] for r in probe])))))
    a = det.detect_face_batch_device(*args, gate=gate, return_quality=True)
    b = det.detect_face_batch_device(*args, gate=gate, return_quality=True)
    assert a[0] == b[0] == before and same(a[1], b[1]) and np.array_equal(a[2], b[2]) and list(a[3]) == list(b[3])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[4], b[4])) and 1 <= a[3][8] < ungated[3][8]
    # a ticket that was still being assembled when the call came in is not disturbed by it
    t = det.enqueue_device(ptrs[:3], [448] * 3, [448] * 3, 0.5)
    c = det.detect_face_batch_device(*args, gate=gate, return_quality=True)
    assert det.wait(t, 3) == before[:3]
    assert c[0] == before and same(c[1], a[1]) and list(c[3]) == list(a[3])
    assert det.wait(det.enqueue_device(*args), 8) == before
    # the standalone gated call on the same detections gives the same faces and records
    s = det.face_batch(ptrs, [448] * 8, [448] * 8, [rows_of(d) for d in before], gate=gate, return_quality=True, max_faces=256)
    assert same(s[1], a[1]) and np.array_equal(s[2], a[2]) and list(s[3]) == list(a[3])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(s[4], a[4]))
    # the ungated call after gated ones is what it was
    again = det.detect_face_batch_device(*args)
    assert again[0] == before and same(again[1], ungated[1]) and list(again[3]) == list(ungated[3])


def test_bad_gates_are_refused_and_multi_device_handles_refuse(rfa, crop448):
    det = engine(rfa)
    dev = to_device([crop448])[0]
    faces = golden("crop448_mnet25.npz")["det"]
    args = ([dev.data_ptr()], [448], [448])
    good = det.detect_face_batch_device(*args, 0.5, gate=dict(min_sharpness=1.0), return_quality=True)
    bad_size = rfa.face_gate(min_sharpness=1.0)
    bad_size.struct_size = 8
    for bad in (dict(min_sharpness=-1.0), dict(min_covered=1.5), dict(max_abs_yaw=float("nan")), dict(min_luma=float("inf")), bad_size):
        for call in (lambda: det.detect_face_batch_device(*args, 0.5, gate=bad), lambda: det.face_batch(*args, [faces], gate=bad),
                     lambda: det.face_quality(*args, [faces], gate=bad), lambda: det.detect_face_batch([crop448], 0.5, gate=bad)):
            with pytest.raises(rfa.RFError) as e:
                call()
            assert e.value.status == -1
    again = det.detect_face_batch_device(*args, 0.5, gate=dict(min_sharpness=1.0), return_quality=True)       # the handle is fine afterwards
    assert again[0] == good[0] and len(good[1]) >= 1 and same(again[1], good[1]) and same_records(again[4], good[4])
    multi = rfa.RetinaFace(ASSETS, "net3", 0.4, precision=FP16, net_hw=(448, 448), model_stem="mnet25", devices=[0, 0])
    try:
        for call in (lambda: multi.detect_face_batch_device(*args, 0.5, gate=dict(min_sharpness=1.0)),
                     lambda: multi.detect_face_batch([crop448], 0.5, return_quality=True),
                     lambda: multi.face_batch(*args, [faces], gate=dict(min_iod=1.0)),
                     lambda: multi.face_quality(*args, [faces])):
            with pytest.raises(rfa.RFError) as e:
                call()
            assert e.value.status == -5          # RF_ERR_UNSUPPORTED
        assert len(multi.detect_device(*args, 0.5)[0]) >= 1
    finally:
        multi.close()


# ---------------------------------------------------------------------------------------------- 7. the C++ class
def test_cpp_class_detect_face_batch_gated(rfa, base_frame, tmp_path):
    src = os.path.join(ROOT, "tests", "csrc", "test_face_quality.cpp")
    exe = str(tmp_path / "test_face_quality")
    lib_dir = os.path.dirname(rfa.lib_path())
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DRF_NO_OPENCV", "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                           "-L" + lib_dir, "-lretinaface_amd", "-Wl,-rpath," + lib_dir])
    raw, out = str(tmp_path / "frame.raw"), str(tmp_path / "out.bin")
    base_frame.tofile(raw)
    det = engine(rfa, prec=FP32, hw=(896, 1280))     # rf_options.precision 0, what the program's zeroed options select
    faces0 = rows_of(det.detect(base_frame, 0.5))
    probe = fqr.records([base_frame], [faces0], None, size=112, max_faces=4)[0]
    thr = float(np.float32(between(probe["sharpness"], 1)))
    for dtype, rgb, capacity, mf, min_sharp in (("f16", 1, 64, 4, thr), ("f32", 0, 3, 4, -1.0)):
        r = subprocess.run([exe, ASSETS, "mnet25", "896", "1280", raw, "896", "1280", "0.5", "112", str(fbr.FORMAT_OF[dtype]), str(rgb),
                            str(capacity), str(mf), repr(min_sharp), out], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        blob = open(out, "rb").read()
        n, tr = (int(v) for v in np.frombuffer(blob, np.int32, 2))
        assert n == 3
        off = np.frombuffer(blob, np.int32, n + 1, 8)
        pos, faces = 8 + 4 * (n + 1), []
        for _ in range(n):
            k = int(np.frombuffer(blob, np.int32, 1, pos)[0])
            faces.append(np.frombuffer(blob, np.float32, k * 15, pos + 4).reshape(k, 15))
            pos += 4 + 60 * k
        stride = int(np.frombuffer(blob, np.int32, 1, pos)[0])
        recs = np.frombuffer(blob, fqr.DTYPE, n * stride, pos + 4).reshape(n, stride)
        pos += 4 + 64 * n * stride
        got = int(np.frombuffer(blob, np.int32, 1, pos)[0])
        mats = np.frombuffer(blob, np.float64, got * 6, pos + 4).reshape(got, 6)
        tensor = np.frombuffer(blob, fbr.DTYPES[fbr.FORMAT_OF[dtype]], got * 3 * 112 * 112, pos + 4 + 48 * got).reshape(got, 3, 112, 112)
        assert stride == mf and np.array_equal(faces[0], faces0) and len(faces[1]) == 0 and np.array_equal(faces[0], faces[2])
        gate = dict(min_sharpness=min_sharp) if min_sharp >= 0 else None
        want_t, want_m, want_o, want_q = fqr.gated_batch([base_frame, None, base_frame], faces, fbr.FORMAT_OF[dtype], gate, rgb=rgb,
                                                         capacity=capacity, max_faces=mf)
        assert list(off) == list(want_o) and got == min(int(off[n]), capacity) and tr == int(off[n] > capacity)
        if gate:
            assert 1 <= want_o[1] < min(len(faces0), mf)
        assert same(tensor, want_t) and np.array_equal(mats, want_m)
        assert same_records([recs[i, :len(want_q[i])] for i in range(n)], want_q) and not recs[1].tobytes().strip(b"\0")
