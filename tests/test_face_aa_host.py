"""Antialiased face crops, host side (no GPU): tests/face_aa_ref.py is pinned to align_ref (k = 1 is the plain crop bit for bit),
rf_face_aa_factor -- the factor the kernels run, compiled for the host -- must equal it, the two appended spec fields are validated
and the struct of the size before them is still accepted, and the reference has the properties the feature exists for: a one-pixel
checkerboard under a 2:1 or 4:1 face comes out flat grey instead of black, and noise loses its variance."""
import ctypes as C

import numpy as np
import pytest

import align_ref
import face_aa_ref as far
import face_batch_ref as fbr
import face_quality_ref as fqr
from conftest import golden
from retinaface_amd import _lib, face_aa_factor, face_batch_spec

OLD_SIZE = 48                                                              # rf_face_batch_spec up to and including capacity
GOLDEN_SETS = ("fixture_mnet25.npz", "fixture_mnet-deconv-0517.npz", "crop448_mnet25.npz", "crop448_mnet-deconv-0517.npz")


def native_factor(lib, face, cs, size, aa_max):
    f = _lib.rf_face.from_buffer_copy(np.asarray(face, np.float32).tobytes())
    return lib.rf_face_aa_factor(C.byref(f), C.c_float(cs), size, aa_max)


def checkerboard(n=160):
    board = (((np.arange(n)[:, None] + np.arange(n)[None, :]) & 1) * 255).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(board[:, :, None], 3, axis=2))


def noise_frame():
    return np.random.default_rng(0).integers(0, 256, size=(200, 240, 3), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------- the reference is pinned to align_ref
def test_ref_with_factor_one_is_the_plain_crop(base_frame):
    faces = golden("fixture_mnet25.npz")["det"]
    for size in (16, 101):
        for f in faces[:3]:
            want, wm = align_ref.crop(base_frame, f, 1.0, size)
            got, gm = far.crop_aa(base_frame, f, 1.0, size, aa_max=1)      # aa_max 1: k = 1 whatever the face
            assert np.array_equal(got, want) and np.array_equal(gm, wm)
    frame = noise_frame()
    for size in (16, 17):
        for f, rot, ox, oy in ((0.5, 0.3, 60.0, 50.0), (1.0, 0.3, 20.0, 15.0), (1.4, -1.1, 100.0, 90.0), (1.0, 0.0, -5.0, -4.0)):
            face = far.build_face(f, rot, ox, oy, size)
            assert far.aa_factor(face, 1.0, size, 8) == 1                  # a face of k = 1 under the largest aa_max
            want, _ = align_ref.crop(frame, face, 1.0, size)
            assert want.any() and np.array_equal(far.crop_aa(frame, face, 1.0, size, aa_max=8)[0], want)
    bad = np.zeros(15, np.float32)
    assert not far.crop_aa(frame, bad, 1.0, 16, 8)[0].any()                # an invalid face: a zero crop
    # the batch / quality restatements with aa_max = 1 are face_batch_ref's / face_quality_ref's
    rows = [far.build_face(3.0, 0.3, 20.0, 15.0, 16), far.build_face(1.0, 0.0, 30.0, 30.0, 16), bad]
    t, m, off = far.batch([frame, None], [rows, rows], fbr.F16_CHW, size=16, rgb=1, aa_max=1)
    wt, wm, woff = fbr.batch([frame, None], [rows, rows], fbr.F16_CHW, size=16, rgb=1)
    assert t.tobytes() == wt.tobytes() and np.array_equal(m, wm) and list(off) == list(woff) == [0, 3, 3]
    gate = dict(min_sharpness=1.0)
    got, want = far.records([frame], [rows], gate, size=16, aa_max=1), fqr.records([frame], [rows], gate, size=16)
    assert got[0].tobytes() == want[0].tobytes()


# ---------------------------------------------------------------------------------------------- rf_face_aa_factor
@pytest.mark.parametrize("name", GOLDEN_SETS)
def test_factor_equals_the_reference_on_the_golden_detections(built_lib, name):
    faces = golden(name)["det"]
    assert len(faces) >= 1
    seen = set()
    for f in faces:
        for size in (16, 112, 512):
            for cs in (1.0, 2.5, float(np.float32(1280) / np.float32(448))):
                for aa_max in (1, 2, 4, 8):
                    want = far.aa_factor(f, cs, size, aa_max)
                    assert native_factor(built_lib, f, cs, size, aa_max) == want, (name, size, cs, aa_max)
                    seen.add(want)
    assert seen == {1, 2, 4, 8}


def test_factor_of_built_faces_and_defaults(built_lib):
    expect = {0.5: 1, 1.0: 1, 1.5: 2, 2.0: 2, 3.0: 4, 4.0: 4, 6.0: 8, 9.0: 8}
    for size in (16, 17):
        for f, k in expect.items():
            face = far.build_face(f, 0.3, 20.0, 15.0, size)
            assert far.aa_factor(face, 1.0, size, 8) == k, (size, f)
            assert native_factor(built_lib, face, 1.0, size, 8) == k, (size, f)
            assert face_aa_factor(face, 1.0, size, 8) == k
        big = far.build_face(12.0, 0.3, 20.0, 15.0, size)
        assert far.aa_factor(big, 1.0, size, 4) == 4 and native_factor(built_lib, big, 1.0, size, 4) == 4
        assert native_factor(built_lib, big, 1.0, size, 0) == 4            # aa_max 0 = 4
        assert face_aa_factor(big, crop_size=size) == 4
    # crop_size 0 = 112; the coordinate scale multiplies the face
    face = far.build_face(1.0, 0.3, 20.0, 15.0, 112)
    assert native_factor(built_lib, face, 1.0, 0, 8) == 1 and native_factor(built_lib, face, 3.0, 0, 8) == far.aa_factor(face, 3.0, 112, 8) == 4
    # invalid faces: all landmarks equal, NaN
    same = np.zeros(15, np.float32)
    same[5:10], same[10:15] = 100.0, 80.0
    nan = far.build_face(6.0, 0.3, 20.0, 15.0, 16)
    nan[8] = np.nan
    for bad in (same, nan):
        assert far.aa_factor(bad, 1.0, 16, 8) == 1 and native_factor(built_lib, bad, 1.0, 16, 8) == 1
    # bad arguments
    assert built_lib.rf_face_aa_factor(None, C.c_float(1.0), 112, 4) == _lib.RF_ERR_INVALID_ARG
    for size in (8, 15, 513, -112):
        assert native_factor(built_lib, face, 1.0, size, 4) == _lib.RF_ERR_INVALID_ARG
    for aa_max in (3, 5, 16, -1):
        assert native_factor(built_lib, face, 1.0, 112, aa_max) == _lib.RF_ERR_INVALID_ARG
    with pytest.raises(_lib.RFError):
        face_aa_factor(face, aa_max=3)


# ---------------------------------------------------------------------------------------------- spec validation
def plan(lib, sp, counts=(3, 0, 9, 2)):
    n = len(counts)
    off = (C.c_int * (n + 1))(*([-7] * (n + 1)))
    bpf = C.c_size_t(0)
    total = lib.rf_face_batch_plan(C.byref(sp), (C.c_int * n)(*counts), n, off, C.byref(bpf))
    return total, list(off), bpf.value


def table(lib, sp, channel=1):
    out = np.full(256, 77, fbr.DTYPES[sp.format])
    return lib.rf_face_value_table(C.byref(sp), channel, out.ctypes.data), out.tobytes()


def test_both_struct_sizes_are_accepted_and_bad_fields_refused(built_lib):
    assert C.sizeof(_lib.rf_face_batch_spec) == 56 and _lib.rf_face_batch_spec.antialias.offset == OLD_SIZE
    for dtype in ("u8", "f16", "f32"):
        new = face_batch_spec(96, dtype, True, (1.0, 2.0, 3.0), (0.5, 0.25, 2.0), max_faces=4, capacity=5)
        assert new.struct_size == 56 and new.antialias == 0 and new.aa_max == 0
        old = face_batch_spec(96, dtype, True, (1.0, 2.0, 3.0), (0.5, 0.25, 2.0), max_faces=4, capacity=5)
        old.struct_size = OLD_SIZE
        old.antialias, old.aa_max = 7, 99                                  # beyond the old size: never read
        on = face_batch_spec(96, dtype, True, (1.0, 2.0, 3.0), (0.5, 0.25, 2.0), max_faces=4, capacity=5, antialias=True, aa_max=8)
        want = plan(built_lib, new)
        assert want == (9, [0, 3, 3, 7, 9], 3 * 96 * 96 * np.dtype(fbr.DTYPES[new.format]).itemsize)
        assert plan(built_lib, old) == want and plan(built_lib, on) == want
        st, tab = table(built_lib, new)
        assert st == 0 and tab == fbr.value_table(new.format, 1, (1.0, 2.0, 3.0), (0.5, 0.25, 2.0)).tobytes()
        assert table(built_lib, old) == (0, tab) and table(built_lib, on) == (0, tab)
    for aa_max in (0, 1, 2, 4, 8):
        for aa in (False, True):
            assert plan(built_lib, face_batch_spec(capacity=2, antialias=aa, aa_max=aa_max))[0] == 14   # (max_faces 0 = 256)
    bad = [face_batch_spec(antialias=aa, aa_max=v) for v in (3, 5, 16, -1) for aa in (False, True)]   # validated even when off
    two = face_batch_spec()
    two.antialias = 2
    neg = face_batch_spec()
    neg.antialias = -1
    for size in (OLD_SIZE - 4, OLD_SIZE + 4, 56 + 4, 0):
        sp = face_batch_spec()
        sp.struct_size = size
        bad.append(sp)
    for sp in bad + [two, neg]:
        total, off, bpf = plan(built_lib, sp, (1, 2))
        assert total == _lib.RF_ERR_INVALID_ARG and off == [-7, -7, -7] and bpf == 0       # nothing written
        st, tab = table(built_lib, sp)
        assert st == _lib.RF_ERR_INVALID_ARG and tab == np.full(256, 77, np.float16).tobytes()


# ---------------------------------------------------------------------------------------------- what the feature is for
def test_checkerboard_becomes_flat_grey():
    frame = checkerboard()
    for size in (16, 17):
        for f in (2.0, 4.0):
            face = far.build_face(f, 0.0, 40.0, 30.0, size)
            assert far.aa_factor(face, 1.0, size, 8) == int(f)
            plain, _ = align_ref.crop(frame, face, 1.0, size)
            aa, _ = far.crop_aa(frame, face, 1.0, size, aa_max=8)
            assert (plain == 0).all() and (aa == 128).all(), (size, f, np.unique(plain), np.unique(aa))
            q = far.quality(frame, face, 1.0, size, aa_max=8)
            assert q["sharpness"].tobytes() == np.float64(0.0).tobytes() and int(q["sum_luma"]) == 128 * size * size
            assert int(q["covered"]) == size * size
            assert fqr.quality(frame, face, 1.0, size)["sharpness"] == 0.0                 # (all black: flat too)
        face = far.build_face(4.0, 0.2, 40.0, 30.0, size)
        plain, _ = align_ref.crop(frame, face, 1.0, size)
        aa, _ = far.crop_aa(frame, face, 1.0, size, aa_max=8)
        assert int(aa.max()) - int(aa.min()) <= 16, (size, aa.min(), aa.max())
        assert int(plain.max()) - int(plain.min()) >= 200, (size, plain.min(), plain.max())
        qa, qp = far.quality(frame, face, 1.0, size, aa_max=8), fqr.quality(frame, face, 1.0, size)
        assert qa["sharpness"] < qp["sharpness"] and qa["covered"] == qp["covered"] == size * size
        assert qa["iod2"] == qp["iod2"] and qa["yaw"] == qp["yaw"] and qa["sin2_roll"] == qp["sin2_roll"]


def test_noise_loses_its_variance():
    frame = noise_frame()
    for size in (16, 17):
        face = far.build_face(4.0, 0.3, 20.0, 15.0, size)
        plain, _ = align_ref.crop(frame, face, 1.0, size)
        aa, _ = far.crop_aa(frame, face, 1.0, size, aa_max=8)
        assert aa.astype(np.float64).std() < 0.5 * plain.astype(np.float64).std(), (aa.std(), plain.std())
