"""Antialiased face crops on the GPU: with rf_face_batch_spec.antialias set, the tensor, the matrices, the offsets and the quality
records the engine returns must equal tests/face_aa_ref.py byte for byte -- every supersampling factor in one launch, faces over the
frame's border, outside it and invalid, unaligned destinations, the gated calls, the fused call on oversize frames across the
launches of a call, and the C++ class; with the option off (or aa_max = 1) every byte is the plain call's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import face_aa_ref as far
import face_batch_ref as fbr
import face_quality_ref as fqr
from conftest import ASSETS, ROOT
from test_gpu_align import FP16, FP32, engine, rfa, rows_of, to_device  # noqa: F401  (rfa: fixture)

pytestmark = pytest.mark.gpu

ES = {"u8": 1, "f16": 2, "f32": 4}
H, W = 200, 240


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_records(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == fqr.DTYPE and len(g) == len(w), (i, len(g), len(w))
        for k in range(len(w)):
            assert g[k].tobytes() == w[k].tobytes(), (i, k, g[k], w[k])
    return True


def noise_frame():
    return np.random.default_rng(0).integers(0, 256, size=(H, W, 3), dtype=np.uint8)


def multi_k_faces(size):
    """one call's faces: k = 1, 1, 2, 4, 8 under aa_max = 8, then one half outside the frame, one wholly outside, one invalid"""
    faces = [far.build_face(f, 0.3, 20.0, 15.0, size) for f in (0.5, 1.0, 1.5, 3.0, 6.0)]
    faces.append(far.build_face(3.0, 0.4, -10.0, -8.0, size))
    faces.append(far.build_face(3.0, 0.0, -5000.0, 40.0, size))
    same_pt = np.zeros(15, np.float32)
    same_pt[5:10], same_pt[10:15] = 100.0, 80.0
    faces.append(same_pt)
    return np.array(faces, np.float32)


_crops, _recs = {}, {}


def ref_crops(size, aa_max):
    """(u8 BGR crops, matrices) of multi_k_faces on the noise frame; aa_max None = the plain crop.  Computed once, never changed."""
    key = (size, aa_max)
    if key not in _crops:
        import align_ref
        fr, fa = noise_frame(), multi_k_faces(size)
        _crops[key] = align_ref.crops(fr, fa, 1.0, size) if aa_max is None else far.crops_aa(fr, fa, 1.0, size, aa_max)
        for a in _crops[key]:
            a.setflags(write=False)
    return _crops[key]


def ref_records(size, aa_max):
    """the ungated records of multi_k_faces on the noise frame (flags: INVALID or 0); aa_max None = the plain crop"""
    key = (size, aa_max)
    if key not in _recs:
        fr, fa = noise_frame(), multi_k_faces(size)
        _recs[key] = (fqr.records([fr], [fa], None, size=size) if aa_max is None else far.records([fr], [fa], None, size=size, aa_max=aa_max))[0]
        _recs[key].setflags(write=False)
    return _recs[key]


def roi_view(frame):
    """the frame on the device as an ROI of a wider buffer: odd pointer, odd step"""
    import torch
    h, w = frame.shape[:2]
    step = w * 3 + 13
    dev = to_device([frame])[0]
    wide = torch.zeros((h + 1, step), dtype=torch.uint8, device="cuda")
    wide.view(-1)[1:1 + h * step].view(h, step)[:, :w * 3] = dev.view(h, w * 3)
    torch.cuda.synchronize()
    assert (wide.data_ptr() + 1) % 2 == 1 and step % 2 == 1
    return wide, wide.data_ptr() + 1, step


# ---------------------------------------------------------------------------------------------- 1. standalone call
@pytest.mark.parametrize("dtype", ("u8", "f16", "f32"))
def test_standalone_call_with_every_factor_in_one_launch(rfa, dtype):
    import torch
    det = engine(rfa)
    keep, ptr, step = roi_view(noise_frame())
    es = ES[dtype]
    for size in (16, 17, 101):
        faces = multi_k_faces(size)
        n = len(faces)
        fb = 3 * size * size * es
        for aa_max in (2, 8):
            ks = [rfa.face_aa_factor(f, 1.0, size, aa_max) for f in faces]
            assert ks == [far.aa_factor(f, 1.0, size, aa_max) for f in faces]
            assert ks[:5] == [min(k, aa_max) for k in (1, 1, 2, 4, 8)] and ks[5] == min(4, aa_max) and ks[7] == 1
            assert set(ks) == ({1, 2, 4, 8} if aa_max == 8 else {1, 2})
            crops, want_m = ref_crops(size, aa_max)
            for rgb in (0, 1):
                want_t = fbr.convert(crops, fbr.FORMAT_OF[dtype], rgb)
                buf = torch.full((n * fb + 64,), 77, dtype=torch.uint8, device="cuda")
                d_out = buf.data_ptr() + es                                # one element into the canary: no band starts 16-aligned
                _, t, m, off = det.face_batch([ptr], [H], [W], [faces], steps=[step], crop_size=size, dtype=dtype, rgb=bool(rgb),
                                              capacity=n, d_out=d_out, antialias=True, aa_max=aa_max)
                torch.cuda.synchronize()
                assert same(t, want_t), (size, aa_max, rgb, int((t != want_t).sum()))
                assert np.array_equal(m.reshape(-1, 6), want_m) and list(off) == [0, n]
                got = buf.cpu().numpy()
                assert got[es:es + n * fb].tobytes() == want_t.tobytes(), (size, aa_max, rgb)
                assert (got[:es] == 77).all() and (got[es + n * fb:] == 77).all()          # the canaries are intact
        # what the reference says about these faces: the half-outside one is partly zero, the last two are the constant of q = 0
        u8 = ref_crops(size, 8)[0]
        assert u8[5].any() and not u8[5].all() and not u8[6].any() and not u8[7].any() and ref_crops(size, 8)[1][6].any()
        assert not np.array_equal(u8[4], ref_crops(size, None)[0][4])      # k = 8 is not the plain crop


# ---------------------------------------------------------------------------------------------- 2. off is off
def raw_face_batch(det, ptr, step, faces, sp, shape, dtype):
    """rf_face_batch_device with the caller's own rf_face_batch_spec bytes (any struct_size): (status, tensor, matrices, offsets)"""
    from retinaface_amd import _lib
    n = len(faces)
    flat = np.ascontiguousarray(faces, np.float32)
    tensor = np.full((sp.capacity,) + shape, 77, dtype)
    mats = np.zeros((sp.capacity, 6), np.float64)
    off = (C.c_int * 2)()
    st = det._lib.rf_face_batch_device(det._h, (C.c_void_p * 1)(ptr), (C.c_int * 1)(H), (C.c_int * 1)(W), (C.c_int * 1)(step), 1,
                                       flat.ctypes.data_as(C.POINTER(_lib.rf_face)), n, (C.c_int * 1)(n), None, C.byref(sp), None,
                                       tensor.ctypes.data, mats.ctypes.data_as(C.POINTER(C.c_double)), off)
    return st, tensor, mats, list(off)


@pytest.mark.parametrize("dtype", ("u8", "f16", "f32"))
def test_off_is_off_and_factor_one_is_the_plain_call(rfa, dtype):
    det = engine(rfa)
    keep, ptr, step = roi_view(noise_frame())
    for size in (16, 17, 101):
        faces = multi_k_faces(size)
        n = len(faces)
        crops, want_m = ref_crops(size, None)
        want_t = fbr.convert(crops, fbr.FORMAT_OF[dtype], 1)
        shape = (size, size, 3) if dtype == "u8" else (3, size, size)
        old = rfa.face_batch_spec(size, dtype, True, max_faces=n, capacity=n)
        old.struct_size = 48                                               # the struct before antialias / aa_max: they are not read
        old.antialias, old.aa_max = 1, 99
        st, t_old, m_old, off_old = raw_face_batch(det, ptr, step, faces, old, shape, want_t.dtype)
        assert st == 0 and off_old == [0, n] and same(t_old, want_t) and np.array_equal(m_old, want_m)
        new = rfa.face_batch_spec(size, dtype, True, max_faces=n, capacity=n, antialias=False, aa_max=8)
        assert new.struct_size == 56
        st, t_new, m_new, off_new = raw_face_batch(det, ptr, step, faces, new, shape, want_t.dtype)
        assert st == 0 and off_new == off_old and same(t_new, t_old) and np.array_equal(m_new, m_old)
        one = rfa.face_batch_spec(size, dtype, True, max_faces=n, capacity=n, antialias=True, aa_max=1)
        st, t_one, m_one, off_one = raw_face_batch(det, ptr, step, faces, one, shape, want_t.dtype)
        assert st == 0 and off_one == off_old and same(t_one, t_old) and np.array_equal(m_one, m_old)
        for bad in (dict(antialias=True, aa_max=3), dict(antialias=False, aa_max=16)):
            with pytest.raises(rfa.RFError) as e:
                det.face_batch([ptr], [H], [W], [faces], steps=[step], crop_size=size, dtype=dtype, **bad)
            assert e.value.status == -1


# ---------------------------------------------------------------------------------------------- 3. the checkerboard
def test_checkerboard_comes_out_flat_grey_on_the_device(rfa):
    board = (((np.arange(160)[:, None] + np.arange(160)[None, :]) & 1) * 255).astype(np.uint8)
    frame = np.ascontiguousarray(np.repeat(board[:, :, None], 3, axis=2))
    det = engine(rfa)
    dev = to_device([frame])[0]
    for size in (16, 17):
        faces = np.array([far.build_face(f, 0.0, 40.0, 30.0, size) for f in (2.0, 4.0)], np.float32)
        assert [rfa.face_aa_factor(f, 1.0, size, 8) for f in faces] == [2, 4]
        _, t, _, _ = det.face_batch([dev.data_ptr()], [160], [160], [faces], crop_size=size, dtype="u8", rgb=False, antialias=True, aa_max=8)
        assert t.shape == (2, size, size, 3) and (t == 128).all(), (size, np.unique(t))
        assert same(t, far.batch([frame], [faces], fbr.U8_HWC, size=size, aa_max=8)[0])
        _, p, _, _ = det.face_batch([dev.data_ptr()], [160], [160], [faces], crop_size=size, dtype="u8", rgb=False)
        assert (p == 0).all()                                              # the plain crop: every sample on the same parity
        q = det.face_batch([dev.data_ptr()], [160], [160], [faces], crop_size=size, dtype="u8", antialias=True, aa_max=8,
                           return_quality=True)[4][0]
        assert all(r["sharpness"].tobytes() == np.float64(0.0).tobytes() and r["sum_luma"] == 128 * size * size for r in q)


# ---------------------------------------------------------------------------------------------- 4. gated
def between(values, lo):
    v = sorted(float(x) for x in values)
    assert v[lo] < v[lo + 1]
    return (v[lo] + v[lo + 1]) / 2


@pytest.mark.parametrize("size", (16, 17, 112))
def test_gated_records_and_tensor_of_the_antialiased_crop(rfa, size):
    det = engine(rfa)
    keep, ptr, step = roi_view(noise_frame())
    frame, faces = noise_frame(), multi_k_faces(size)
    n = len(faces)
    base = ref_records(size, 8)
    plain = ref_records(size, None)
    assert not base[7].tobytes().strip(b"\0") and base[6]["covered"] == 0 and 0 < base[5]["covered"] < size * size
    assert np.array_equal(base["covered"], plain["covered"]) and np.array_equal(base["iod2"], plain["iod2"])
    gate = dict(min_sharpness=float(np.float32(between(base["sharpness"], 4))))
    want_t, want_m, want_o, want_q = far.gated_batch([frame], [faces], fbr.F16_CHW, gate, size=size, rgb=1, aa_max=8)
    assert 1 <= int(want_o[1]) <= n - 1 and (want_q[0]["flags"] & fqr.SHARPNESS).any()
    _, t, m, off, q = det.face_batch([ptr], [H], [W], [faces], steps=[step], crop_size=size, dtype="f16", gate=gate, return_quality=True,
                                     antialias=True, aa_max=8)
    assert list(off) == list(want_o) and same_records(q, want_q)
    assert same(t, want_t) and np.array_equal(m.reshape(-1, 6), want_m)
    # records without a tensor: d_tensor = tensor = NULL
    _, t0, _, off0, q0 = det.face_batch([ptr], [H], [W], [faces], steps=[step], crop_size=size, dtype="f16", gate=gate, return_quality=True,
                                        antialias=True, aa_max=8, host=False)
    assert t0 is None and list(off0) == list(want_o) and same_records(q0, want_q)
    # a NULL gate: the ungated antialiased bytes, the records with flags 0
    crops, mats = ref_crops(size, 8)
    _, t1, m1, off1, q1 = det.face_batch([ptr], [H], [W], [faces], steps=[step], crop_size=size, dtype="f16", return_quality=True,
                                         antialias=True, aa_max=8)
    ungated = det.face_batch([ptr], [H], [W], [faces], steps=[step], crop_size=size, dtype="f16", antialias=True, aa_max=8)
    assert same(t1, fbr.convert(crops, fbr.F16_CHW, 1)) and same(t1, ungated[1]) and np.array_equal(m1.reshape(-1, 6), mats)
    assert list(off1) == list(ungated[3]) == [0, n]
    assert same_records(q1, far.records([frame], [faces], None, size=size, aa_max=8)) and (q1[0]["flags"] == 0).all()
    # a threshold that keeps a face under plain sampling and drops it under antialias: the decimated noise only looks sharp
    k = int(np.argmax(plain["sharpness"] - base["sharpness"]))
    assert plain["sharpness"][k] > base["sharpness"][k] > 0
    thr = dict(min_sharpness=float(np.float32((plain["sharpness"][k] + base["sharpness"][k]) / 2)))
    assert fqr.gate_flags(plain[k], thr, size) == 0 and fqr.gate_flags(base[k], thr, size) == fqr.SHARPNESS
    qp = det.face_batch([ptr], [H], [W], [faces], steps=[step], crop_size=size, dtype="u8", gate=thr, return_quality=True)[4]
    qa = det.face_batch([ptr], [H], [W], [faces], steps=[step], crop_size=size, dtype="u8", gate=thr, return_quality=True, antialias=True,
                        aa_max=8)[4]
    assert same_records(qp, fqr.records([frame], [faces], thr, size=size)) and qp[0]["flags"][k] == 0
    assert same_records(qa, far.records([frame], [faces], thr, size=size, aa_max=8)) and qa[0]["flags"][k] == fqr.SHARPNESS
    # rf_face_quality_device takes no spec: its records stay those of the plain crop
    assert same_records(det.face_quality([ptr], [H], [W], [faces], steps=[step], crop_size=size), [plain])


# ---------------------------------------------------------------------------------------------- 5. fused call, oversize frames
def enlarge(frame, r=2):
    return None if frame is None else np.ascontiguousarray(np.repeat(np.repeat(frame, r, axis=0), r, axis=1))


def test_fused_call_on_the_fixture_frame_enlarged_twice(rfa, base_frame):
    det = engine(rfa, prec=FP16, hw=(896, 1280))
    frame = enlarge(base_frame)                                            # 1792 x 2560: oversize, the engine shrinks it by 2
    dev = to_device([frame])[0]
    args = ([dev.data_ptr()], [1792], [2560], 0.5)
    assert det.frame_scale(1792, 2560) == 2.0
    plain = det.detect_device(*args)
    faces = rows_of(plain[0])
    ks = [rfa.face_aa_factor(f, 2.0, 112, 0) for f in faces]
    assert len(faces) >= 3 and max(ks) >= 2 and ks == [far.aa_factor(f, 2.0, 112, 4) for f in faces]
    for dtype, rgb in (("f16", 1), ("u8", 0)):
        dets, t, m, off = det.detect_face_batch_device(*args, dtype=dtype, rgb=bool(rgb), antialias=True)
        assert dets == plain                                               # detection does not see the option
        want_t, want_m, want_o = far.batch([frame], [faces], fbr.FORMAT_OF[dtype], rgb=rgb, scales=[2.0], aa_max=4)
        assert same(t, want_t) and np.array_equal(m.reshape(-1, 6), want_m) and list(off) == list(want_o)
    off_t = det.detect_face_batch_device(*args, dtype="u8", rgb=False)[1]
    assert same(off_t, fbr.batch([frame], [faces], fbr.U8_HWC, scales=[2.0])[0]) and not same(off_t, t)      # and it changes the bytes
    hd, ht, hm, ho = det.detect_face_batch([frame], 0.5, dtype="u8", rgb=False, antialias=True)             # host frames: the same path
    assert hd == plain and same(ht, t) and np.array_equal(hm, m) and list(ho) == list(off)


@pytest.mark.parametrize("kw", ({}, {"coalesce": 1, "lanes": 2}))
def test_antialiased_batches_across_the_launches_of_a_call(rfa, kw):
    from retinaface_amd.frames import synth_frames
    small = synth_frames(448, 448, 11, config=2)
    frames = [enlarge(f) for f in small]                                   # 896 x 896 on a 448 x 448 net: rf_frame_scale = 2
    frames[7] = np.full((896, 896, 3), 128, np.uint8)
    frames[9] = None
    det = engine(rfa, max_batch=8, **kw)
    plain = det.detectBatchImages(frames, 0.5)
    rows = [rows_of(d) for d in plain]
    scales = [2.0] * 11
    ks = [rfa.face_aa_factor(f, 2.0, 96, 8) for r in rows for f in r[:3]]
    assert len(set(ks)) >= 2 and max(ks) >= 2                              # pasted at 1/2, 1 and 2: more than one factor occurs
    want_t, want_m, want_o, want_q = far.gated_batch(frames, rows, fbr.F16_CHW, None, size=96, rgb=1, max_faces=3, scales=scales, aa_max=8)
    # host frames: rf_detect_face_batch, then the gated entry point with a NULL gate for the records
    dets, t, m, off = det.detect_face_batch(frames, 0.5, dtype="f16", crop_size=96, max_faces=3, antialias=True, aa_max=8)
    assert dets == plain and len(dets[7]) == 0 and len(dets[9]) == 0 and max(len(d) for d in dets) >= 3
    assert list(off) == list(want_o) and off[11] == len(t) >= 9 and off[8] == off[7] and off[10] == off[9]
    assert same(t, want_t) and np.array_equal(m.reshape(-1, 6), want_m)
    gd, gt, gm, go, gq = det.detect_face_batch(frames, 0.5, dtype="f16", crop_size=96, max_faces=3, antialias=True, aa_max=8, return_quality=True)
    assert gd == plain and same(gt, t) and np.array_equal(gm, m) and list(go) == list(off) and same_records(gq, want_q)
    # device frames over the frames that exist: the same faces, and the detections of rf_detect_batch_device
    real = [i for i, f in enumerate(frames) if f is not None]
    dev = to_device([frames[i] for i in real])
    ptrs = [x.data_ptr() for x in dev]
    dd, dt, dm, do = det.detect_face_batch_device(ptrs, [896] * 10, [896] * 10, 0.5, dtype="f16", crop_size=96, max_faces=3, antialias=True,
                                                  aa_max=8)
    assert dd == det.detect_device(ptrs, [896] * 10, [896] * 10, 0.5) == [plain[i] for i in real]
    assert same(dt, t) and np.array_equal(dm, m) and do[10] == off[11]
    # a capacity cut inside an image: RF_ERR_TRUNCATED, the true offsets, the first `capacity` faces
    inside = next(i for i in range(11) if want_o[i + 1] - want_o[i] >= 2)
    cap = int(want_o[inside]) + 1
    assert 1 <= cap < int(want_o[11])
    cd, ct, cm, co = det.detect_face_batch(frames, 0.5, dtype="f16", crop_size=96, max_faces=3, antialias=True, aa_max=8, capacity=cap)
    assert det.faces_truncated and det.truncated and cd == plain and list(co) == list(want_o)
    assert len(ct) == cap and same(ct, want_t[:cap]) and np.array_equal(cm.reshape(-1, 6), want_m[:cap])
    assert det.detectBatchImages(frames, 0.5) == plain and not det.truncated


# ---------------------------------------------------------------------------------------------- 6. determinism, non-interference
def test_antialiased_calls_are_deterministic_and_leave_tickets_alone(rfa):
    from retinaface_amd.frames import synth_frames
    frames = [enlarge(f) for f in synth_frames(448, 448, 8, config=3)]
    det = engine(rfa)
    dev = to_device(frames)
    ptrs = [t.data_ptr() for t in dev]
    args = (ptrs, [896] * 8, [896] * 8, 0.5)
    before = det.wait(det.enqueue_device(*args), 8)
    off_call = det.detect_face_batch_device(*args)
    a = det.detect_face_batch_device(*args, antialias=True, return_quality=True)
    b = det.detect_face_batch_device(*args, antialias=True, return_quality=True)
    assert a[0] == b[0] == before and same(a[1], b[1]) and np.array_equal(a[2], b[2]) and list(a[3]) == list(b[3])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[4], b[4]))
    assert list(a[3]) == list(off_call[3]) and np.array_equal(a[2], off_call[2]) and not same(a[1], off_call[1])
    # a ticket that was still being assembled when the call came in is not disturbed by it
    t = det.enqueue_device(ptrs[:3], [896] * 3, [896] * 3, 0.5)
    c = det.detect_face_batch_device(*args, antialias=True)
    assert det.wait(t, 3) == before[:3]
    assert c[0] == before and same(c[1], a[1]) and list(c[3]) == list(a[3])
    assert det.wait(det.enqueue_device(*args), 8) == before
    # the standalone call on the same detections gives the same faces
    s = det.face_batch(ptrs, [896] * 8, [896] * 8, [rows_of(d) for d in before], coord_scale=[2.0] * 8, antialias=True, max_faces=256)
    assert same(s[1], a[1]) and np.array_equal(s[2], a[2]) and list(s[3]) == list(a[3])
    # the plain call after antialiased ones is what it was
    again = det.detect_face_batch_device(*args)
    assert again[0] == before and same(again[1], off_call[1]) and list(again[3]) == list(off_call[3])


# ---------------------------------------------------------------------------------------------- 7. the C++ class
def test_cpp_class_with_an_antialiased_spec(rfa, base_frame, tmp_path):
    src = os.path.join(ROOT, "tests", "csrc", "test_face_aa.cpp")
    exe = str(tmp_path / "test_face_aa")
    lib_dir = os.path.dirname(rfa.lib_path())
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DRF_NO_OPENCV", "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                           "-L" + lib_dir, "-lretinaface_amd", "-Wl,-rpath," + lib_dir])
    raw, out = str(tmp_path / "frame.raw"), str(tmp_path / "out.bin")
    base_frame.tofile(raw)
    size, mf = 32, 4
    for dtype, rgb, capacity, aa, aa_max in (("f16", 1, 64, 1, 8), ("u8", 0, 3, 1, 0), ("f16", 1, 64, 0, 8)):
        r = subprocess.run([exe, ASSETS, "mnet25", "448", "448", raw, "896", "1280", "0.5", str(size), str(fbr.FORMAT_OF[dtype]), str(rgb),
                            str(capacity), str(mf), str(aa), str(aa_max), out], capture_output=True, text=True, timeout=300)
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
        shape = (size, size, 3) if dtype == "u8" else (3, size, size)
        tensor = np.frombuffer(blob, fbr.DTYPES[fbr.FORMAT_OF[dtype]], got * 3 * size * size, pos + 4 + 48 * got).reshape((got,) + shape)
        assert stride == mf and len(faces[0]) >= 3 and len(faces[1]) == 0 and np.array_equal(faces[0], faces[2])
        cs = float(np.float32(1280) / np.float32(448))                     # the 896 x 1280 frame on the 448 x 448 net
        kw = dict(size=size, rgb=rgb, capacity=capacity, max_faces=mf, scales=[cs] * 3)
        frames = [base_frame, None, base_frame]
        if aa:
            assert max(far.aa_factor(f, cs, size, aa_max or 4) for f in faces[0][:mf]) >= 2       # the option is in effect
            want_t, want_m, want_o, want_q = far.gated_batch(frames, faces, fbr.FORMAT_OF[dtype], None, aa_max=aa_max or 4, **kw)
        else:
            want_t, want_m, want_o, want_q = fqr.gated_batch(frames, faces, fbr.FORMAT_OF[dtype], None, **kw)
        assert list(off) == list(want_o) and got == min(int(off[n]), capacity) and tr == int(off[n] > capacity)
        assert same(tensor, want_t) and np.array_equal(mats, want_m)
        assert same_records([recs[i, :len(want_q[i])] for i in range(n)], want_q) and not recs[1].tobytes().strip(b"\0")
