"""Face alignment on the GPU: every crop and every matrix the engine returns must equal tests/align_ref.py byte for byte --
the standalone call on caller-supplied faces, the fused detect + align call (whose detections must be the bytes
rf_detect_batch_device returns), oversize frames sampled at full resolution, borders, truncation, and the C++ class."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import align_ref
from conftest import ASSETS, ROOT, STEMS, golden

pytestmark = pytest.mark.gpu

FP32, FP16 = 0, 1


@pytest.fixture(scope="module")
def rfa(built_lib):
    import retinaface_amd
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need the GPU box"
    return retinaface_amd


_engines = {}


def engine(rfa, stem="mnet25", prec=FP16, hw=(448, 448), **kw):
    key = (stem, prec, hw, tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in kw.items())))
    if key not in _engines:
        _engines[key] = rfa.RetinaFace(ASSETS, "net3", 0.4, precision=prec, net_hw=hw, model_stem=stem, **kw)
    return _engines[key]


def to_device(frames):
    import torch
    t = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in frames]
    torch.cuda.synchronize()
    return t


def rows_of(dets):
    return np.stack([d.as_row() for d in dets]).astype(np.float32) if dets else np.zeros((0, 15), np.float32)


def check_against_ref(frames, dets, crops, mats, size, scales=None, max_faces=None):
    total = 0
    for i, f in enumerate(frames):
        faces = rows_of(dets[i])[:max_faces]
        want_c, want_m = align_ref.crops(f, faces, 1.0 if scales is None else scales[i], size)
        assert crops[i].shape == want_c.shape, (i, crops[i].shape, want_c.shape)
        assert np.array_equal(crops[i], want_c), (i, int((crops[i] != want_c).sum()))
        assert np.array_equal(mats[i].reshape(-1, 6), want_m), i
        total += len(faces)
    return total


# ---------------------------------------------------------------------------------------------- 1. standalone call
@pytest.mark.parametrize("stem", STEMS)
def test_standalone_align_of_the_golden_detections(rfa, base_frame, stem):
    import torch
    det = engine(rfa)
    faces = golden(f"fixture_{stem}.npz")["det"]
    dev = to_device([base_frame])[0]
    # the same frame as an ROI of a wider buffer: odd pointer, odd step
    step = 1280 * 3 + 13
    wide = torch.zeros((897, step), dtype=torch.uint8, device="cuda")
    wide.view(-1)[1:1 + 896 * step].view(896, step)[:, :1280 * 3] = dev.view(896, 1280 * 3)
    torch.cuda.synchronize()
    roi_ptr = wide.data_ptr() + 1
    assert roi_ptr % 2 == 1 and step % 2 == 1
    for size in (96, 112, 128):
        want_c, want_m = align_ref.crops(base_frame, faces, 1.0, size)
        d_crops = torch.full((6 * size * size * 3,), 77, dtype=torch.uint8, device="cuda")
        crops, mats = det.align([dev.data_ptr()], [896], [1280], [faces], crop_size=size, d_crops=d_crops.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(crops[0], want_c) and np.array_equal(mats[0].reshape(-1, 6), want_m), size
        assert np.array_equal(d_crops.cpu().numpy().reshape(6, size, size, 3), want_c), size          # device output = host output
        crops, mats = det.align([roi_ptr], [896], [1280], [faces], steps=[step], crop_size=size)
        assert np.array_equal(crops[0], want_c) and np.array_equal(mats[0].reshape(-1, 6), want_m), size


def test_standalone_align_into_an_unaligned_device_buffer(rfa, base_frame):
    """crop size 101 and a crop buffer at an odd address: no band of any slot starts on a 16-byte boundary"""
    import torch
    det = engine(rfa)
    faces = golden("fixture_mnet25.npz")["det"]
    dev = to_device([base_frame])[0]
    size, nb = 101, 6 * 101 * 101 * 3
    buf = torch.full((nb + 64,), 77, dtype=torch.uint8, device="cuda")
    crops, _ = det.align([dev.data_ptr()], [896], [1280], [faces], crop_size=size, d_crops=buf.data_ptr() + 3, host=False)
    torch.cuda.synchronize()
    assert crops is None
    got = buf.cpu().numpy()
    want_c, _ = align_ref.crops(base_frame, faces, 1.0, size)
    assert np.array_equal(got[3:3 + nb].reshape(6, size, size, 3), want_c)
    assert (got[:3] == 77).all() and (got[3 + nb:] == 77).all()                                   # nothing outside the slots


def test_standalone_align_applies_the_coordinate_scale_and_many_images(rfa, base_frame, crop448):
    det = engine(rfa)
    big = golden("fixture_mnet25.npz")["det"]
    small = big.copy()
    small[:, 5:] = (big[:, 5:] / np.float32(2.5)).astype(np.float32)
    sub = golden("crop448_mnet25.npz")["det"]
    dev = to_device([base_frame, crop448])
    none = np.zeros((0, 15), np.float32)
    crops, mats = det.align([dev[0].data_ptr(), dev[1].data_ptr(), dev[1].data_ptr()], [896, 448, 448], [1280, 448, 448],
                            [small, sub, none], coord_scale=[2.5, 1.0, 1.0], crop_size=112)
    want_c, want_m = align_ref.crops(base_frame, small, 2.5, 112)
    assert np.array_equal(crops[0], want_c) and np.array_equal(mats[0].reshape(-1, 6), want_m)
    want_c, want_m = align_ref.crops(crop448, sub, 1.0, 112)
    assert np.array_equal(crops[1], want_c) and np.array_equal(mats[1].reshape(-1, 6), want_m)
    assert crops[2].shape == (0, 112, 112, 3)


# ---------------------------------------------------------------------------------------------- 2. borders, degenerate faces
def _template_face(size, scale, ang, ox, oy):
    """landmarks whose aligned crop is the size x size window at (ox, oy), `scale` source pixels per crop pixel, rotated by ang"""
    k = size / 112.0
    tx, ty = np.array(align_ref.TEMPLATE_X) * k, np.array(align_ref.TEMPLATE_Y) * k
    c, s = scale * np.cos(ang), scale * np.sin(ang)
    row = np.zeros(15, np.float32)
    row[5:10] = c * tx - s * ty + ox
    row[10:15] = s * tx + c * ty + oy
    return row


def test_crops_over_every_edge_and_corner_and_invalid_faces(rfa):
    rng = np.random.default_rng(11)
    H, W, size = 211, 317, 112
    frame = rng.integers(1, 256, size=(H, W, 3), dtype=np.uint8)
    faces = [_template_face(size, 1.0, 0.0, ox, oy) for ox in (-40.0, 100.5, W - 60.0) for oy in (-50.0, 60.25, H - 30.0)]
    faces += [_template_face(size, 1.7, 0.6, -30.0, 90.0), _template_face(size, 0.4, -2.5, W - 10.0, H - 5.0),
              _template_face(size, 1.0, 0.0, -1.5, -1.5), _template_face(size, 1.0, 0.0, W - size + 0.75, H - size + 0.75)]
    outside = _template_face(size, 1.0, 0.0, -5000.0, 40.0)
    same = np.zeros(15, np.float32)
    same[5:10], same[10:15] = 100.0, 80.0
    nan = faces[4].copy()
    nan[8] = np.nan
    faces += [outside, same, nan]
    faces = np.array(faces, np.float32)
    det = engine(rfa)
    dev = to_device([frame])[0]
    crops, mats = det.align([dev.data_ptr()], [H], [W], [faces], crop_size=size)
    want_c, want_m = align_ref.crops(frame, faces, 1.0, size)
    assert np.array_equal(crops[0], want_c)
    assert np.array_equal(mats[0].reshape(-1, 6), want_m)
    n = len(faces)
    assert not crops[0][n - 3].any() and mats[0][n - 3].any()              # entirely outside: zero crop, a valid matrix
    for k in (n - 2, n - 1):                                               # degenerate: zero crop AND zero matrix
        assert not crops[0][k].any() and not mats[0][k].any()
    for k in range(9):                                                     # the edge crops do contain zeros and pixels
        if k != 4:
            assert (crops[0][k] == 0).any() and crops[0][k].any()


# ---------------------------------------------------------------------------------------------- 3. fused call
def _fused_matches_plain(det, frames, size=112, **kw):
    dev = to_device(frames)
    ptrs = [t.data_ptr() for t in dev]
    rows, cols = [f.shape[0] for f in frames], [f.shape[1] for f in frames]
    plain = det.detect_device(ptrs, rows, cols, 0.5)
    dets, crops, mats = det.detect_aligned_device(ptrs, rows, cols, 0.5, crop_size=size, **kw)
    assert dets == plain                         # scores, boxes, landmarks (exact floats), counts, anchor indices
    return dets, crops, mats


@pytest.mark.parametrize("prec", (FP32, FP16))
def test_fused_call_on_synthetic_frames(rfa, prec):
    from retinaface_amd.frames import synth_frames
    frames = synth_frames(448, 448, 8, config=1)
    det = engine(rfa, prec=prec)
    dets, crops, mats = _fused_matches_plain(det, frames)
    assert check_against_ref(frames, dets, crops, mats, 112) >= 8


@pytest.mark.parametrize("prec", (FP32, FP16))
def test_fused_call_on_the_fixture_frame(rfa, base_frame, prec):
    det = engine(rfa, prec=prec, hw=(896, 1280))
    dets, crops, mats = _fused_matches_plain(det, [base_frame], size=128)
    assert check_against_ref([base_frame], dets, crops, mats, 128) == 6


@pytest.mark.parametrize("prec,kw", ((FP16, {}), (FP32, {}), (FP16, {"coalesce": 1, "lanes": 2})))
def test_fused_call_with_more_images_than_max_batch(rfa, prec, kw):
    from retinaface_amd.frames import synth_frames
    frames = synth_frames(448, 448, 19, config=2)
    det = engine(rfa, prec=prec, max_batch=8, **kw)
    dets, crops, mats = _fused_matches_plain(det, frames, size=96)
    assert check_against_ref(frames, dets, crops, mats, 96) >= 19


# ---------------------------------------------------------------------------------------------- 4. oversize frames
@pytest.mark.parametrize("mode", ("area", "bilinear"))
def test_oversize_frames_are_sampled_at_full_resolution(rfa, base_frame, crop448, mode):
    det = engine(rfa, oversize_resize=mode)
    frames = [base_frame, crop448]
    dets, crops, mats = _fused_matches_plain(det, frames)
    scales = [det.frame_scale(896, 1280), det.frame_scale(448, 448)]
    assert scales[0] == float(np.float32(1280) / np.float32(448)) and scales[1] == 1.0
    assert len(dets[0]) >= 3 and len(dets[1]) >= 1
    check_against_ref(frames, dets, crops, mats, 112, scales=scales)
    # host frames take the same path
    hd, hc, hm = det.detect_aligned(frames, 0.5)
    assert hd == dets and all(np.array_equal(a, b) for a, b in zip(hc, crops)) and all(np.array_equal(a, b) for a, b in zip(hm, mats))


# ---------------------------------------------------------------------------------------------- 5. host frames, truncation, no faces
def test_host_call_truncation_and_images_without_faces(rfa):
    from retinaface_amd.frames import synth_frames
    frames = synth_frames(448, 448, 6, config=1)
    blank = np.full((448, 448, 3), 128, np.uint8)
    small = frames[3][:300, :401]                                          # smaller than the net, rows with a pitch on the host
    frames = frames[:3] + [blank, small, None] + frames[3:]
    det = engine(rfa)
    real = [f for f in frames if f is not None]
    dets, crops, mats = det.detect_aligned(frames, 0.5)
    assert dets == det.detectBatchImages(frames, 0.5)
    assert len(dets[3]) == 0 and crops[3].shape == (0, 112, 112, 3) and len(dets[5]) == 0 and crops[5].shape[0] == 0
    keep = [i for i, f in enumerate(frames) if f is not None]
    assert check_against_ref(real, [dets[i] for i in keep], [crops[i] for i in keep], [mats[i] for i in keep], 112) >= 8
    # the device-frame call gives the same bytes
    dev = to_device(real)
    dd, dc, dm = det.detect_aligned_device([t.data_ptr() for t in dev], [f.shape[0] for f in real], [f.shape[1] for f in real], 0.5)
    assert dd == [dets[i] for i in keep]
    assert all(np.array_equal(dc[j], crops[i]) and np.array_equal(dm[j], mats[i]) for j, i in enumerate(keep))
    # fewer slots than faces: the first faces in score order
    assert max(len(d) for d in dets) >= 3
    td, tc, tm = det.detect_aligned(frames, 0.5, max_faces=2)
    assert td == dets
    for i in range(len(frames)):
        k = min(len(dets[i]), 2)
        assert tc[i].shape[0] == k and np.array_equal(tc[i], crops[i][:k]) and np.array_equal(tm[i], mats[i][:k])


def test_bad_alignment_arguments_are_refused_on_the_host(rfa, crop448):
    det = engine(rfa)
    dev = to_device([crop448])[0]
    for bad in (dict(crop_size=8), dict(crop_size=1000, max_faces=1), dict(crop_size=16, max_faces=5000)):
        with pytest.raises(rfa.RFError) as e:
            det.detect_aligned_device([dev.data_ptr()], [448], [448], 0.5, **bad)
        assert e.value.status == -1
        with pytest.raises(rfa.RFError) as e:
            det.align([dev.data_ptr()], [448], [448], [golden("crop448_mnet25.npz")["det"]], **bad)
        assert e.value.status == -1
    assert len(det.detect_device([dev.data_ptr()], [448], [448], 0.5)[0]) >= 1       # the handle is fine afterwards


# ---------------------------------------------------------------------------------------------- 6. determinism, non-interference
def test_alignment_is_deterministic_and_leaves_the_async_path_alone(rfa):
    from retinaface_amd.frames import synth_frames
    frames = synth_frames(448, 448, 8, config=3)
    det = engine(rfa)
    dev = to_device(frames)
    ptrs = [t.data_ptr() for t in dev]
    before = det.wait(det.enqueue_device(ptrs, [448] * 8, [448] * 8, 0.5), 8)
    a = det.detect_aligned_device(ptrs, [448] * 8, [448] * 8, 0.5)
    b = det.detect_aligned_device(ptrs, [448] * 8, [448] * 8, 0.5)
    assert a[0] == b[0] == before
    assert all(np.array_equal(x, y) for x, y in zip(a[1], b[1])) and all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))
    # a ticket that was still being assembled when the fused call came in is not disturbed by it
    t = det.enqueue_device(ptrs[:3], [448] * 3, [448] * 3, 0.5)
    c = det.detect_aligned_device(ptrs, [448] * 8, [448] * 8, 0.5)
    assert det.wait(t, 3) == before[:3]
    assert c[0] == before and all(np.array_equal(x, y) for x, y in zip(a[1], c[1]))
    assert det.wait(det.enqueue_device(ptrs, [448] * 8, [448] * 8, 0.5), 8) == before
    sa = det.align(ptrs, [448] * 8, [448] * 8, [rows_of(d) for d in before])
    assert all(np.array_equal(x, y) for x, y in zip(sa[0], a[1])) and all(np.array_equal(x, y) for x, y in zip(sa[1], a[2]))


def test_multi_device_handles_refuse_alignment(rfa, crop448):
    det = rfa.RetinaFace(ASSETS, "net3", 0.4, precision=FP16, net_hw=(448, 448), model_stem="mnet25", devices=[0, 0])
    try:
        dev = to_device([crop448])[0]
        for call in (lambda: det.detect_aligned_device([dev.data_ptr()], [448], [448], 0.5),
                     lambda: det.detect_aligned([crop448], 0.5),
                     lambda: det.align([dev.data_ptr()], [448], [448], [golden("crop448_mnet25.npz")["det"]])):
            with pytest.raises(rfa.RFError) as e:
                call()
            assert e.value.status == -5          # RF_ERR_UNSUPPORTED
        assert len(det.detect_device([dev.data_ptr()], [448], [448], 0.5)[0]) >= 1
    finally:
        det.close()


# ---------------------------------------------------------------------------------------------- 7. the C++ class
def test_cpp_class_detect_and_align(rfa, base_frame, tmp_path):
    src = os.path.join(ROOT, "tests", "csrc", "test_detect_align.cpp")
    exe = str(tmp_path / "test_detect_align")
    lib_dir = os.path.dirname(rfa.lib_path())
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DRF_NO_OPENCV", "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                           "-L" + lib_dir, "-lretinaface_amd", "-Wl,-rpath," + lib_dir])
    raw, out = str(tmp_path / "frame.raw"), str(tmp_path / "out.bin")
    base_frame.tofile(raw)
    for hw, size in (((896, 1280), 112), ((448, 448), 96)):                # at net size, and shrunk by the engine first
        r = subprocess.run([exe, ASSETS, "mnet25", str(hw[0]), str(hw[1]), raw, "896", "1280", "0.5", str(size), out],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        blob = open(out, "rb").read()
        k = int(np.frombuffer(blob, np.int32, 1)[0])
        assert k >= 3
        faces = np.frombuffer(blob, np.float32, k * 15, 4).reshape(k, 15)
        mats = np.frombuffer(blob, np.float64, k * 6, 4 + k * 60).reshape(k, 6)
        crops = np.frombuffer(blob, np.uint8, k * size * size * 3, 4 + k * 60 + k * 48).reshape(k, size, size, 3)
        cs = float(np.float32(max(1280 / hw[1], 896 / hw[0], 1.0)))
        want_c, want_m = align_ref.crops(base_frame, faces, cs, size)
        assert np.array_equal(crops, want_c) and np.array_equal(mats, want_m)
        det = engine(rfa, prec=FP32, hw=hw)          # rf_options.precision 0, what the program's zeroed options select
        assert np.array_equal(faces, rows_of(det.detect(base_frame, 0.5)))
