"""Face batches, host side (no GPU): rf_face_value_table -- the value map the kernel runs, compiled for the host -- must equal the
numpy restatement tests/face_batch_ref.py bit for bit, rf_face_batch_plan must give the packed offsets of the definition and
refuse every bad spec, and face_batch_ref itself is pinned to align_ref."""
import ctypes as C

import numpy as np
import pytest

import align_ref
import face_batch_ref as fbr
from conftest import golden
from retinaface_amd import _lib, face_batch_plan, face_value_table

PARAM_SETS = {
    "default": (None, None),
    "imagenet": ((103.53, 116.28, 123.675), (1 / 57.375, 1 / 57.12, 1 / 58.395)),
    "unit": ((0.0, 0.0, 0.0), (1 / 255, 1 / 255, 1 / 255)),
}


def spec(fmt=fbr.F16_CHW, crop=112, rgb=0, mean=None, scale=None, max_faces=0, capacity=1, struct_size=None):
    sp = _lib.rf_face_batch_spec()
    sp.struct_size = C.sizeof(_lib.rf_face_batch_spec) if struct_size is None else struct_size
    sp.crop_size, sp.format, sp.rgb, sp.max_faces, sp.capacity = crop, fmt, rgb, max_faces, capacity
    if mean is not None:
        sp.mean = (C.c_float * 3)(*mean)
    if scale is not None:
        sp.scale = (C.c_float * 3)(*scale)
    return sp


def native_table(lib, sp, channel):
    out = np.full(256, 77, fbr.DTYPES[sp.format])
    assert lib.rf_face_value_table(C.byref(sp), channel, out.ctypes.data) == 0
    return out


@pytest.mark.parametrize("name", sorted(PARAM_SETS))
@pytest.mark.parametrize("rgb", (0, 1))
@pytest.mark.parametrize("fmt", (fbr.U8_HWC, fbr.F16_CHW, fbr.F32_CHW))
def test_value_table_equals_the_reference_bit_for_bit(built_lib, fmt, rgb, name):
    mean, scale = PARAM_SETS[name]
    for c in range(3):
        got = native_table(built_lib, spec(fmt, rgb=rgb, mean=mean, scale=scale), c)
        want = fbr.value_table(fmt, c, mean, scale)
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (fmt, rgb, name, c)


@pytest.mark.parametrize("name", sorted(PARAM_SETS))
def test_values_stay_clear_of_the_half_subnormal_range(built_lib, name):
    """every non-zero value of the three sets is >= 3.9e-3 in magnitude (half subnormals start below 6.2e-5), and the default set
    is exact in half: no denormal-mode question can arise between host and device"""
    mean, scale = PARAM_SETS[name]
    for c in range(3):
        f32 = native_table(built_lib, spec(fbr.F32_CHW, mean=mean, scale=scale), c)
        f16 = native_table(built_lib, spec(fbr.F16_CHW, mean=mean, scale=scale), c)
        for t in (f32, f16.astype(np.float32)):
            nz = np.abs(t[t != 0])
            assert len(nz) >= 255 and nz.min() >= 3.9e-3, (name, c, nz.min())
        if name == "default":
            assert np.array_equal(f16.astype(np.float32), f32)
            assert np.array_equal(f32, (np.arange(256) - 127.5) / 128)


def test_python_value_table_wrapper(built_lib):
    mean, scale = PARAM_SETS["imagenet"]
    for dtype in ("u8", "f16", "f32"):
        got = face_value_table(2, dtype=dtype, mean=mean, scale=scale)
        assert got.tobytes() == fbr.value_table(fbr.FORMAT_OF[dtype], 2, mean, scale).tobytes()
    assert face_value_table(0).tobytes() == fbr.value_table(fbr.F16_CHW, 0).tobytes()
    sp = spec()
    out = np.zeros(256, np.float16)
    for ch in (-1, 3):
        assert built_lib.rf_face_value_table(C.byref(sp), ch, out.ctypes.data) == _lib.RF_ERR_INVALID_ARG
    assert built_lib.rf_face_value_table(None, 0, out.ctypes.data) == _lib.RF_ERR_INVALID_ARG
    assert built_lib.rf_face_value_table(C.byref(sp), 0, None) == _lib.RF_ERR_INVALID_ARG


def plan(lib, sp, counts):
    n = len(counts)
    cnt = (C.c_int * max(n, 1))(*counts)
    off = (C.c_int * (n + 1))(*([-7] * (n + 1)))
    bpf = C.c_size_t(0)
    total = lib.rf_face_batch_plan(C.byref(sp) if sp is not None else None, cnt, n, off, C.byref(bpf))
    return total, list(off), bpf.value


@pytest.mark.parametrize("counts,max_faces", (([3, 0, 0, 5, 1, 0], 8), ([9, 2, 40, 0, 4], 4), ([1], 1), ([4096, 5000], 4096)))
def test_plan_packs_in_call_order(built_lib, counts, max_faces):
    want = fbr.offsets(counts, max_faces)
    total = int(want[-1])
    for capacity in (max(1, total - 1), total, total + 3):                 # total above, at and below the capacity: never clamped
        got, off, bpf = plan(built_lib, spec(fbr.F16_CHW, 112, max_faces=max_faces, capacity=capacity), counts)
        assert got == total and off == list(want)
        assert bpf == 3 * 112 * 112 * 2
    assert built_lib.rf_face_batch_plan(C.byref(spec(max_faces=max_faces)), (C.c_int * len(counts))(*counts), len(counts), None, None) == total


def test_plan_without_images_and_bytes_per_face(built_lib):
    assert plan(built_lib, spec(), []) == (0, [0], 3 * 112 * 112 * 2)
    for fmt, es in ((fbr.U8_HWC, 1), (fbr.F16_CHW, 2), (fbr.F32_CHW, 4)):
        for crop, S in ((0, 112), (16, 16), (101, 101), (512, 512)):
            assert plan(built_lib, spec(fmt, crop), [2])[2] == 3 * S * S * es
    assert plan(built_lib, spec(max_faces=0), [300, 7])[:2] == (263, [0, 256, 263])      # 0 = the default max_detections
    total, off, bpf = face_batch_plan([3, 0, 9, 2], max_faces=4, capacity=5, dtype="f32", crop_size=96)
    assert total == 9 and list(off) == [0, 3, 3, 7, 9] and bpf == 3 * 96 * 96 * 4


def test_plan_refuses_every_invalid_spec(built_lib):
    nan, inf = float("nan"), float("inf")
    bad = [spec(struct_size=0), spec(struct_size=C.sizeof(_lib.rf_face_batch_spec) - 4), spec(struct_size=C.sizeof(_lib.rf_face_batch_spec) + 4),
           spec(crop=8), spec(crop=15), spec(crop=513), spec(crop=-112), spec(fmt=3), spec(fmt=-1),
           spec(max_faces=-1), spec(max_faces=4097), spec(capacity=0), spec(capacity=-5),
           spec(mean=(nan, 0, 0), scale=(1, 1, 1)), spec(mean=(0, 0, 0), scale=(1, inf, 1)), spec(mean=(0, -inf, 0), scale=(1, 1, 1)),
           spec(fmt=fbr.U8_HWC, mean=(0, 0, 0), scale=(nan, 1, 1))]
    for sp in bad:
        total, off, bpf = plan(built_lib, sp, [1, 2])
        assert total == _lib.RF_ERR_INVALID_ARG
        assert off == [-7, -7, -7] and bpf == 0                                # nothing written
        out = np.zeros(256, np.float32)
        if sp.capacity == 1:                                                   # (the table does not depend on the capacity)
            assert built_lib.rf_face_value_table(C.byref(sp), 0, out.ctypes.data) == _lib.RF_ERR_INVALID_ARG
    assert plan(built_lib, None, [1])[0] == _lib.RF_ERR_INVALID_ARG
    assert plan(built_lib, spec(), [1, -1, 2])[0] == _lib.RF_ERR_INVALID_ARG   # a negative count
    assert built_lib.rf_face_batch_plan(C.byref(spec()), None, 2, None, None) == _lib.RF_ERR_INVALID_ARG
    assert built_lib.rf_face_batch_plan(C.byref(spec()), None, -1, None, None) == _lib.RF_ERR_INVALID_ARG
    for sp in (spec(crop=16), spec(crop=512), spec(max_faces=1), spec(max_faces=4096), spec(fmt=fbr.F32_CHW, rgb=1)):
        assert plan(built_lib, sp, [1, 2])[0] >= 2
    with pytest.raises(_lib.RFError):
        face_batch_plan([1], crop_size=8)


def test_face_batch_ref_is_pinned_to_align_ref(base_frame, crop448):
    """U8_HWC in frame order is the concatenation of align_ref's crops; the other layouts are permutations / the value map of it"""
    fa, fb = golden("fixture_mnet25.npz")["det"], golden("crop448_mnet25.npz")["det"]
    frames, faces = [base_frame, None, crop448, crop448], [fa, fa, fb[:0], fb]
    ca, ma = align_ref.crops(base_frame, fa, 1.0, 112)
    cb, mb = align_ref.crops(crop448, fb, 1.0, 112)
    want_c, want_m = np.concatenate([ca, cb]), np.concatenate([ma, mb])
    t, m, off = fbr.batch(frames, faces, fbr.U8_HWC)
    assert list(off) == [0, len(fa), len(fa), len(fa), len(fa) + len(fb)]
    assert t.dtype == np.uint8 and np.array_equal(t, want_c) and np.array_equal(m, want_m)
    t2, _, off2 = fbr.batch(frames, faces, fbr.U8_HWC, rgb=1, max_faces=2, capacity=3)
    assert list(off2) == [0, 2, 2, 2, 2 + min(2, len(fb))]
    assert np.array_equal(t2, np.concatenate([ca[:2], cb[:2]])[:3, :, :, ::-1])
    t3, _, _ = fbr.batch(frames, faces, fbr.F32_CHW, rgb=1)
    assert t3.shape == (len(want_c), 3, 112, 112) and t3.dtype == np.float32
    assert np.array_equal(t3[:, 0], (want_c[..., 2].astype(np.float32) - np.float32(127.5)) * np.float32(1 / 128))
    t4, _, _ = fbr.batch(frames, faces, fbr.F16_CHW, mean=(1, 2, 3), scale=(0.5, 0.25, 2))
    assert np.array_equal(t4[:, 1].astype(np.float32), (want_c[..., 1].astype(np.float32) - 2) * 0.25)
